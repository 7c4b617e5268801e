#!/usr/bin/env python3
"""The edge-bias multi-head calls (csr5hip_mha_edge_bias, csr5hip_mha_edge_bias_backward) against what they generalise and against
what they replace, on the same handle and the same packed tensors; one JSON line per (workload, dtype, heads, k, d).

    python scripts/bench_mha_edge_bias.py [--workloads scircuit,webbase,nd24k] [--dtypes f64,f32] [--heads 4,8] [--kd 16x16,64x64]
                                          [--skip-b]

bench_mha.py's protocol: per pair of routes the batches alternate, a batch is timed by device events, the figure is the median
of 7 batches of 10 calls after a warm-up, and the baseline's fastest and slowest batch are printed with it: their spread is the
margin of any ratio.  BEFORE ANY TIMING THE BITS ARE COMPARED, for both comparisons.

A, THE COST OF GENERALITY: mhaEdgeBias against mhaBiased with the same rank-one bias -- the handle holds integer values a,
the slopes are powers of two, B[e, h] = slopes[h] * a_e is formed in torch (exact), and the two routes must agree in every bit
of O, dQ, dK, dV and dB = dS.  Per line: edge_us against biased_us (forward, one launch each); edge_backward_us against
biased_backward_us (two launches each, all three gradients); edge_backward_db_us against biased_backward_ds_us (the same with the
(nnz, heads) gradient wanted).

B, WHAT IT REPLACES: for a bias that differs per head, H times (updateValues of that head's column + the single-head mhaBiased
on the head's column slices), forward, and the same with mhaBiasedBackward (dS wanted), backward, against ONE mhaEdgeBias /
mhaEdgeBiasBackward (dB wanted).  The columns of B are made contiguous before the timing (the per-head route needs them so; the
copy is not charged to it).  calls: library calls per forward / backward of the two routes; launches: a lower bound for the
per-head route (updateValues refreshes the parent's values, gathers and refreshes the companion's: three launches at least).
The handle's values are overwritten by this route and given back afterwards."""
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


def check(rc, what):
    if rc:
        raise RuntimeError(f"{what} failed: {rc}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="scircuit,webbase,nd24k")
    ap.add_argument("--dtypes", default="f64,f32")
    ap.add_argument("--heads", default="4,8")
    ap.add_argument("--kd", default="16x16,64x64")
    ap.add_argument("--skip-b", action="store_true", help="comparison A only")
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--per-batch", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    kds = [tuple(int(v) for v in kd.split("x")) for kd in args.kd.split(",")]
    r = lambda v: round(float(v), 2)  # noqa: E731
    for wl in args.workloads.split(","):
        for dn in args.dtypes.split(","):
            dtype = np.float64 if dn == "f64" else np.float32
            mat = WORKLOADS[wl](dtype)
            tdt = torch.float64 if dtype == np.float64 else torch.float32
            rp = torch.from_numpy(mat.row_ptr).to(DEV)
            ci = torch.from_numpy(mat.col).to(DEV)
            gen = torch.Generator(device=DEV).manual_seed(5)
            a = torch.randint(-4, 5, (mat.nnz,), device=DEV, generator=gen).to(tdt)  # integers: slope * a is exact
            va = a.clone()
            A = H.anonymouslibHandle(mat.m, mat.n, dtype=np.dtype(dtype).name)
            rcs = [A.inputCSR(mat.nnz, rp, ci, va), A.setSigma(H.ANONYMOUSLIB_AUTO_TUNED_SIGMA), A.asCSR5(), A.buildTranspose()]
            if any(rcs):
                raise RuntimeError(f"handle setup failed: {rcs}")
            for heads in (int(h) for h in args.heads.split(",")):
                slopes = torch.tensor([(2.0, 0.5, -1.0, 1.0)[h % 4] for h in range(heads)], dtype=tdt, device=DEV)
                B1 = a[:, None] * slopes[None, :]
                for k, d in kds:
                    def rand(rows, width):
                        return torch.rand((rows, heads, width), dtype=tdt, device=DEV, generator=gen) * 2 - 1
                    Q, K, V, dO = rand(mat.m, k) / k ** 0.5, rand(mat.n, k), rand(mat.n, d), rand(mat.m, d)
                    O, dQ, dK, dV = (torch.empty_like(t) for t in (dO, Q, K, V))
                    O1, dQ1, dK1, dV1 = (torch.empty_like(t) for t in (dO, Q, K, V))
                    work = torch.empty(4 * mat.m * heads, dtype=tdt, device=DEV)
                    dB, dS = (torch.empty((mat.nnz, heads), dtype=tdt, device=DEV) for _ in range(2))
                    Bt = [B1]  # (the bias the edge route reads: rank one for A, per head for B)

                    def biased():
                        check(A.mhaBiased(Q, K, V, O1, scale=0.25, slopes=slopes), "mhaBiased")

                    def edge():
                        check(A.mhaEdgeBias(Q, K, V, O, B=Bt[0], scale=0.25), "mhaEdgeBias")

                    def biased_bwd():
                        check(A.mhaBiasedBackward(Q, K, V, dO, dQ1, dK1, dV1, work, scale=0.25, slopes=slopes), "mhaBiasedBackward")

                    def edge_bwd():
                        check(A.mhaEdgeBiasBackward(Q, K, V, dO, dQ, dK, dV, work, B=Bt[0], scale=0.25), "mhaEdgeBiasBackward")

                    def biased_bwd_ds():
                        check(A.mhaBiasedBackward(Q, K, V, dO, dQ1, dK1, dV1, work, scale=0.25, slopes=slopes, dS=dS), "mhaBiasedBackward dS")

                    def edge_bwd_db():
                        check(A.mhaEdgeBiasBackward(Q, K, V, dO, dQ, dK, dV, work, B=Bt[0], scale=0.25, dB=dB), "mhaEdgeBiasBackward dB")
                    for f in (biased, edge, biased_bwd_ds, edge_bwd_db):
                        f()
                    torch.cuda.synchronize()
                    equal_a = all(same(x, y) for x, y in ((O, O1), (dQ, dQ1), (dK, dK1), (dV, dV1), (dB, dS)))
                    te, tb = timed(edge, biased, args.batches, args.per_batch, args.warmup)
                    be, bb = timed(edge_bwd, biased_bwd, args.batches, args.per_batch, args.warmup)
                    de, db = timed(edge_bwd_db, biased_bwd_ds, args.batches, args.per_batch, args.warmup)
                    line = {
                        "workload": mat.name, "dtype": dn, "heads": heads, "k": k, "d": d, "m": mat.m, "n": mat.n, "nnz": mat.nnz,
                        "same_bits_a": equal_a,
                        "edge_us": r(np.median(te)), "biased_us": r(np.median(tb)), "biased_min_us": r(min(tb)), "biased_max_us": r(max(tb)),
                        "ratio": round(float(np.median(te) / np.median(tb)), 4), "launches": [1, 1],
                        "edge_backward_us": r(np.median(be)), "biased_backward_us": r(np.median(bb)), "biased_backward_min_us": r(min(bb)),
                        "biased_backward_max_us": r(max(bb)), "ratio_backward": round(float(np.median(be) / np.median(bb)), 4),
                        "edge_backward_db_us": r(np.median(de)), "biased_backward_ds_us": r(np.median(db)),
                        "biased_backward_ds_min_us": r(min(db)), "biased_backward_ds_max_us": r(max(db)),
                        "ratio_backward_db": round(float(np.median(de) / np.median(db)), 4), "launches_backward": [2, 2],
                    }
                    equal_b = None
                    if not args.skip_b:
                        Bp = torch.rand((mat.nnz, heads), dtype=tdt, device=DEV, generator=gen) * 4 - 2
                        cols = [Bp[:, h].contiguous() for h in range(heads)]
                        Bt[0] = Bp
                        work1 = torch.empty(4 * mat.m, dtype=tdt, device=DEV)
                        sl = [slice(h, h + 1) for h in range(heads)]

                        def per_head():
                            for h in range(heads):
                                check(A.updateValues(cols[h]), "updateValues")
                                check(A.mhaBiased(Q[:, sl[h]], K[:, sl[h]], V[:, sl[h]], O1[:, sl[h]], scale=0.25), "mhaBiased of a head")

                        def per_head_bwd():
                            for h in range(heads):
                                check(A.updateValues(cols[h]), "updateValues")
                                check(A.mhaBiasedBackward(Q[:, sl[h]], K[:, sl[h]], V[:, sl[h]], dO[:, sl[h]], dQ1[:, sl[h]], dK1[:, sl[h]],
                                                          dV1[:, sl[h]], work1, scale=0.25, dS=dS[:, sl[h]]), "mhaBiasedBackward of a head")
                        for f in (per_head, edge, per_head_bwd, edge_bwd_db):
                            f()
                        torch.cuda.synchronize()
                        equal_b = all(same(x, y) for x, y in ((O, O1), (dQ, dQ1), (dK, dK1), (dV, dV1), (dB, dS)))
                        te2, tp = timed(edge, per_head, args.batches, args.per_batch, min(args.warmup, 2))
                        de2, dp = timed(edge_bwd_db, per_head_bwd, args.batches, args.per_batch, min(args.warmup, 2))
                        check(A.updateValues(a), "updateValues")  # the handle's values again
                        line.update({
                            "same_bits_b": equal_b,
                            "per_head_us": r(np.median(tp)), "per_head_min_us": r(min(tp)), "per_head_max_us": r(max(tp)),
                            "edge_per_head_bias_us": r(np.median(te2)), "per_head_over_edge": round(float(np.median(tp) / np.median(te2)), 2),
                            "calls": [2 * heads, 1], "launches_at_least": [4 * heads, 1],
                            "per_head_backward_us": r(np.median(dp)), "per_head_backward_min_us": r(min(dp)),
                            "per_head_backward_max_us": r(max(dp)), "edge_per_head_bias_backward_us": r(np.median(de2)),
                            "per_head_backward_over_edge": round(float(np.median(dp) / np.median(de2)), 2),
                            "calls_backward": [2 * heads, 1], "launches_backward_at_least": [5 * heads, 2],
                        })
                        del Bp, cols, work1
                    print(json.dumps(line), flush=True)
                    if not equal_a or equal_b is False:
                        raise SystemExit(f"the edge-bias calls differ from the biased ones: {mat.name} {dn} heads={heads} k={k} d={d} "
                                         f"(A {equal_a}, B {equal_b})")
                    del Q, K, V, dO, O, dQ, dK, dV, O1, dQ1, dK1, dV1, work, dB, dS
                    torch.cuda.empty_cache()
            A.destroy()
            A.close()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
