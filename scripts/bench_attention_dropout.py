#!/usr/bin/env python3
"""The price of the dropout mask inside the fused attention kernels, one JSON line per point, on bench_mha.py's protocol: batches of
the two routes alternating, device events, medians of 7 batches of 10 calls, the baseline's fastest and slowest batch as the margin.

    python scripts/bench_attention_dropout.py [--parts a,b] [--families mha,gat] [--workloads scircuit,webbase,nd24k]
                                              [--dtypes f64,f32] [--heads 4,8] [--kd 16x16,64x64] [--gat-kd 1x16,16x16] [--ps 0.1,0.6]

(a) THE DROPPED CALL AGAINST ITS UNDROPPED SIBLING, forward and backward: ``dropoutMha`` / ``dropoutMhaBackward`` against
``mhaEdgeBias`` / ``mhaEdgeBiasBackward`` (B=None, scale 1 / sqrt(k)), and ``dropoutGat`` / ``dropoutGatBackward`` against ``gat`` /
``gatBackward`` (a given for k > 1).  Before any timing the two routes are compared bit for bit at p = 0, where they are defined to
be equal.  The ratio is the price of Philox per entry and head; it has no pass threshold.
(b) THE DROPPED CALL AGAINST THE ROUTE IT REPLACES, forward only, H = 4, (k, d) = (16, 16): per head ``sddmm`` -> ``rowSoftmax`` -> a
torch multiply by the mask (``dropoutMask`` once, outside the timing, scaled by 1 / (1 - p)) -> ``updateValues`` -> ``spmm``, with
nnz-long temporaries and the handle's values overwritten; the two results are compared to rounding before the timing.
The workloads are those of bench_attention.py."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from benchmark_spmv_using_csr5_amd import handle as H  # noqa: E402
from scripts.bench_attention import DEV, WORKLOADS  # noqa: E402
from scripts.bench_mha import same, timed  # noqa: E402

SEED, OFFSET = 0x1234, 7


def ok(rc, what):
    if rc:
        raise RuntimeError(f"{what} failed: {rc}")


def stats(tf, tg, name, base):
    r = lambda v: round(float(v), 2)  # noqa: E731
    return {f"{name}_us": r(np.median(tf)), f"{base}_us": r(np.median(tg)), f"{base}_min_us": r(min(tg)), f"{base}_max_us": r(max(tg)),
            f"{name}_over_{base}": round(float(np.median(tf) / np.median(tg)), 3)}


def part_a(A, mat, dn, tdt, family, heads, k, d, ps, args, gen):
    def rand(rows, width):
        return torch.rand((rows, heads, width), dtype=tdt, device=DEV, generator=gen) * 2 - 1
    Q, K, V, dO = rand(mat.m, k) / k ** 0.5, rand(mat.n, k), rand(mat.n, d), rand(mat.m, d)
    outs = [torch.empty_like(t) for t in (dO, Q, K, V)]
    outs1 = [torch.empty_like(t) for t in (dO, Q, K, V)]
    work, work1 = (torch.empty(4 * mat.m * heads, dtype=tdt, device=DEV) for _ in range(2))
    scale = 1.0 / k ** 0.5
    a = (torch.rand((heads, k), dtype=tdt, device=DEV, generator=gen) * 2 - 1) if family == "gat" and k > 1 else None

    def calls(p, o, w):
        """(forward, backward) of the dropped route at p, or of the undropped one (p None), into o with workspace w"""
        if family == "mha":
            if p is None:
                return (lambda: ok(A.mhaEdgeBias(Q, K, V, o[0], scale=scale), "mhaEdgeBias"),
                        lambda: ok(A.mhaEdgeBiasBackward(Q, K, V, dO, o[1], o[2], o[3], w, scale=scale), "mhaEdgeBiasBackward"))
            return (lambda: ok(A.dropoutMha(Q, K, V, o[0], p, SEED, OFFSET, scale=scale), "dropoutMha"),
                    lambda: ok(A.dropoutMhaBackward(Q, K, V, dO, p, SEED, OFFSET, dQ=o[1], dK=o[2], dV=o[3], work=w, scale=scale),
                               "dropoutMhaBackward"))
        if p is None:
            return (lambda: ok(A.gat(Q, K, V, o[0], a=a, scale=scale), "gat"),
                    lambda: ok(A.gatBackward(Q, K, V, dO, o[1], o[2], o[3], w, a=a, scale=scale), "gatBackward"))
        return (lambda: ok(A.dropoutGat(Q, K, V, o[0], p, SEED, OFFSET, a=a, scale=scale), "dropoutGat"),
                lambda: ok(A.dropoutGatBackward(Q, K, V, dO, p, SEED, OFFSET, dQ=o[1], dK=o[2], dV=o[3], work=w, a=a, scale=scale),
                           "dropoutGatBackward"))
    base_f, base_b = calls(None, outs1, work1)
    for f in calls(0.0, outs, work) + (base_f, base_b):
        f()
    torch.cuda.synchronize()
    equal = all(same(x, y) for x, y in zip(outs, outs1))
    if not equal:
        raise SystemExit(f"p = 0 differs from the undropped call: {family} {mat.name} {dn} heads={heads} k={k} d={d}")
    for p in ps:
        drop_f, drop_b = calls(p, outs, work)
        tf, tg = timed(drop_f, base_f, args.batches, args.per_batch, args.warmup)
        bf, bg = timed(drop_b, base_b, args.batches, args.per_batch, args.warmup)
        line = {"part": "a", "family": family, "workload": mat.name, "dtype": dn, "heads": heads, "k": k, "d": d, "p": p, "nnz": mat.nnz,
                "same_bits_at_p0": equal}
        line.update(stats(tf, tg, "dropped", "undropped"))
        line.update(stats(bf, bg, "dropped_backward", "undropped_backward"))
        print(json.dumps(line), flush=True)


def part_b(A, mat, dn, tdt, ps, args, gen):
    heads, k, d = 4, 16, 16

    def rand(rows, width):
        return torch.rand((rows, heads, width), dtype=tdt, device=DEV, generator=gen) * 2 - 1
    Q, K, V = rand(mat.m, k) / k ** 0.5, rand(mat.n, k), rand(mat.n, d)
    O, O1 = torch.empty((mat.m, heads, d), dtype=tdt, device=DEV), torch.empty((mat.m, heads, d), dtype=tdt, device=DEV)
    s, w = torch.empty(mat.nnz, dtype=tdt, device=DEV), torch.empty(mat.nnz, dtype=tdt, device=DEV)
    keep = torch.empty((mat.nnz, heads), dtype=torch.uint8, device=DEV)
    for p in ps:
        ok(A.dropoutMask(keep, p, SEED, OFFSET), "dropoutMask")
        factor = (keep.to(tdt) * (1.0 / (1.0 - p))).t().contiguous()           # (heads, nnz): one contiguous row per head

        def fused():
            ok(A.dropoutMha(Q, K, V, O, p, SEED, OFFSET), "dropoutMha")

        def unfused():
            for h in range(heads):
                ok(A.sddmm(Q[:, h], K[:, h], s), "sddmm")
                ok(A.rowSoftmax(s, w), "rowSoftmax")
                torch.mul(w, factor[h], out=s)
                ok(A.updateValues(s), "updateValues")
                ok(A.spmm(V[:, h], O1[:, h]), "spmm")
        fused()
        unfused()
        torch.cuda.synchronize()
        tol = 1e-10 if tdt == torch.float64 else 2e-4
        close = bool(torch.allclose(O, O1, rtol=tol, atol=tol))
        if not close:
            raise SystemExit(f"the fused and the unfused route disagree: {mat.name} {dn} p={p}")
        tf, tg = timed(fused, unfused, args.batches, args.per_batch, args.warmup)
        line = {"part": "b", "workload": mat.name, "dtype": dn, "heads": heads, "k": k, "d": d, "p": p, "nnz": mat.nnz, "agree": close,
                "launches": [1, "5 per head and more"]}
        line.update(stats(tf, tg, "fused", "unfused"))
        line["unfused_over_fused"] = round(float(np.median(tg) / np.median(tf)), 3)
        print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="a,b")
    ap.add_argument("--families", default="mha,gat")
    ap.add_argument("--workloads", default="scircuit,webbase,nd24k")
    ap.add_argument("--dtypes", default="f64,f32")
    ap.add_argument("--heads", default="4,8")
    ap.add_argument("--kd", default="16x16,64x64")
    ap.add_argument("--gat-kd", default="1x16,16x16")
    ap.add_argument("--ps", default="0.1,0.6")
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--per-batch", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    kds = {"mha": [tuple(int(v) for v in kd.split("x")) for kd in args.kd.split(",")],
           "gat": [tuple(int(v) for v in kd.split("x")) for kd in args.gat_kd.split(",")]}
    ps = [float(p) for p in args.ps.split(",")]
    for wl in args.workloads.split(","):
        for dn in args.dtypes.split(","):
            dtype = np.float64 if dn == "f64" else np.float32
            mat = WORKLOADS[wl](dtype)
            tdt = torch.float64 if dtype == np.float64 else torch.float32
            rp = torch.from_numpy(mat.row_ptr).to(DEV)
            ci = torch.from_numpy(mat.col).to(DEV)
            va = torch.ones(mat.nnz, dtype=tdt, device=DEV)
            A = H.anonymouslibHandle(mat.m, mat.n, dtype=np.dtype(dtype).name)
            rcs = [A.inputCSR(mat.nnz, rp, ci, va), A.setSigma(H.ANONYMOUSLIB_AUTO_TUNED_SIGMA), A.asCSR5(), A.buildTranspose()]
            if any(rcs):
                raise RuntimeError(f"handle setup failed: {rcs}")
            gen = torch.Generator(device=DEV).manual_seed(5)
            if "a" in args.parts.split(","):
                for family in args.families.split(","):
                    for heads in (int(h) for h in args.heads.split(",")):
                        for k, d in kds[family]:
                            part_a(A, mat, dn, tdt, family, heads, k, d, ps, args, gen)
                            torch.cuda.empty_cache()
            if "b" in args.parts.split(","):
                part_b(A, mat, dn, tdt, ps, args, gen)  # (last: it overwrites the handle's values)
            A.destroy()
            A.close()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
