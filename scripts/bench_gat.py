#!/usr/bin/env python3
"""The additive attention calls (csr5hip_gat, csr5hip_gat_backward) against the route they replace, on the same handle and the same
packed tensors; one JSON line per (workload, dtype, heads, k, d).

    python scripts/bench_gat.py [--workloads scircuit,webbase,nd24k] [--dtypes f64,f32] [--heads 4,8] [--kd 1x16,1x64,16x16,64x64]

bench_mha.py's protocol: per pair of routes the batches alternate, a batch is timed by device events, the figure is the median of
7 batches of 10 calls after a warm-up, and the baseline's fastest and slowest batch are printed with it: their spread is the margin
of any ratio.  BEFORE ANY TIMING THE TWO ROUTES ARE COMPARED under a bound (their summation orders differ, so not bit for bit):
every output within 2**12 unit roundoffs of the largest magnitude of the old route's.

THE ROUTE IT REPLACES goes through (nnz, H) and (nnz, H, k) temporaries in torch: prebuilt int64 row and column index tensors (not
charged), u = Q[rows] + K[cols], l = leaky_relu(u), the (nnz, H) scores scale * (l * a).sum(-1), ONE mhaEdgeBias with k = 0 and those
scores as B; backward: ONE mhaEdgeBiasBackward with k = 0 (dV and dB = ds), then t = scale * ds, w = a * (u > 0 ? 1 : ns) and
index_add of t w over the rows (dQ) and over the columns (dK), and (t l).sum(0) for the gradient of a.  It is measured forward
(old_forward_us against gat_us) and forward + backward (old_step_us against gat_step_us: gat, gatBackward with all of dQ, dK, dV,
dAr, and dAr.sum(0)).  old_step_bytes: the bytes torch's allocator hands out during one step of the old route (the temporaries of
length nnz); gat_step_bytes the same for the new one (dAr.sum(0)'s result).  A point whose old route is ESTIMATED to need more than
--old-limit-gib is reported with old_route "skipped" and the new route's times alone.  The estimate is a rough guess made before
anything runs -- four live (nnz, H, max(k, 1)) temporaries (u, l, the products, t w) -- not what old_step allocates (old_step_bytes,
measured where the route runs, is two to three times as much over a whole step).  FOR A SKIPPED POINT NOTHING IS COMPARED BEFORE THE
TIMING: its times stand without the check of the two routes against each other.

gat_backward_us / gat_backward_no_dar_us: gatBackward alone with dQ, dK, dV and with / without dAr: the cost of the per-row shares
of a's gradient, a write as large as dQ's."""
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
from scripts.bench_mha import timed  # noqa: E402

SLOPE = 0.2


def check(rc, what):
    if rc:
        raise RuntimeError(f"{what} failed: {rc}")


def allocated(f):
    """bytes torch's allocator hands out during one call of f"""
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats()["allocated_bytes.all.allocated"]
    f()
    torch.cuda.synchronize()
    return int(torch.cuda.memory_stats()["allocated_bytes.all.allocated"] - before)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="scircuit,webbase,nd24k")
    ap.add_argument("--dtypes", default="f64,f32")
    ap.add_argument("--heads", default="4,8")
    ap.add_argument("--kd", default="1x16,1x64,16x16,64x64")
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--per-batch", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--old-limit-gib", type=float, default=48.0)
    args = ap.parse_args()
    kds = [tuple(int(v) for v in kd.split("x")) for kd in args.kd.split(",")]
    r = lambda v: round(float(v), 2)  # noqa: E731
    for wl in args.workloads.split(","):
        for dn in args.dtypes.split(","):
            dtype = np.float64 if dn == "f64" else np.float32
            mat = WORKLOADS[wl](dtype)
            tdt = torch.float64 if dtype == np.float64 else torch.float32
            u = float(np.finfo(dtype).eps) / 2
            rp = torch.from_numpy(mat.row_ptr).to(DEV)
            ci = torch.from_numpy(mat.col).to(DEV)
            va = torch.ones(mat.nnz, dtype=tdt, device=DEV)
            A = H.anonymouslibHandle(mat.m, mat.n, dtype=np.dtype(dtype).name)
            rcs = [A.inputCSR(mat.nnz, rp, ci, va), A.setSigma(H.ANONYMOUSLIB_AUTO_TUNED_SIGMA), A.asCSR5(), A.buildTranspose()]
            if any(rcs):
                raise RuntimeError(f"handle setup failed: {rcs}")
            # prebuilt, not charged; from the host arrays: asCSR5 has put the device copy of the columns into tile order
            rows = torch.from_numpy(np.repeat(np.arange(mat.m, dtype=np.int64), np.diff(mat.row_ptr))).to(DEV)
            cols = torch.from_numpy(mat.col[:mat.nnz].astype(np.int64)).to(DEV)
            gen = torch.Generator(device=DEV).manual_seed(5)
            one, slope = torch.ones((), dtype=tdt, device=DEV), torch.full((), SLOPE, dtype=tdt, device=DEV)
            for heads in (int(h) for h in args.heads.split(",")):
                for k, d in kds:
                    def rand(*shape):
                        return torch.rand(shape, dtype=tdt, device=DEV, generator=gen) * 2 - 1
                    Q, K, V, dO = rand(mat.m, heads, k), rand(mat.n, heads, k), rand(mat.n, heads, d), rand(mat.m, heads, d)
                    a = rand(heads, k) if k > 1 else None  # GAT (k = 1): no attention vector; GATv2: (H, k)
                    scale = 1.0 / k ** 0.5
                    O, dQ, dK, dV, dAr = (torch.empty_like(t) for t in (dO, Q, K, V, Q))
                    O1, dV1 = torch.empty_like(dO), torch.empty_like(V)
                    Q0, K0 = (torch.empty((n, heads, 0), dtype=tdt, device=DEV) for n in (mat.m, mat.n))
                    work = torch.empty(4 * mat.m * heads, dtype=tdt, device=DEV)
                    old = {}

                    def gat():
                        check(A.gat(Q, K, V, O, a=a, negative_slope=SLOPE, scale=scale), "gat")

                    def gat_bwd():
                        check(A.gatBackward(Q, K, V, dO, dQ, dK, dV, work, a=a, negative_slope=SLOPE, scale=scale, dAr=dAr), "gatBackward")

                    def gat_bwd_no_dar():
                        check(A.gatBackward(Q, K, V, dO, dQ, dK, dV, work, a=a, negative_slope=SLOPE, scale=scale), "gatBackward")

                    def gat_step():
                        gat()
                        gat_bwd()
                        old["da_new"] = dAr.sum(0)

                    def old_forward():
                        uu = Q[rows] + K[cols]
                        l = torch.nn.functional.leaky_relu(uu, SLOPE)
                        s = (scale * (l * a).sum(-1) if a is not None else scale * l.sum(-1)).contiguous()
                        check(A.mhaEdgeBias(Q0, K0, V, O1, B=s), "mhaEdgeBias k = 0")
                        return uu, l, s

                    def old_step():
                        uu, l, s = old_forward()
                        ds = torch.empty_like(s)
                        check(A.mhaEdgeBiasBackward(Q0, K0, V, dO, dV=dV1, work=work, B=s, dB=ds), "mhaEdgeBiasBackward k = 0")
                        t = (scale * ds)[:, :, None]
                        g = torch.where(uu > 0, one, slope)  # (0-d tensors of the operands' dtype: the slope rounded once, to it)
                        tw = t * (g * a if a is not None else g)
                        old["dQ"] = torch.zeros_like(Q).index_add_(0, rows, tw)
                        old["dK"] = torch.zeros_like(K).index_add_(0, cols, tw)
                        old["da"] = (t * l).sum(0)
                    temporaries = 4 * mat.nnz * heads * max(k, 1) * (8 if dtype == np.float64 else 4)  # (a guess: the docstring)
                    skip = temporaries > args.old_limit_gib * 2 ** 30
                    line = {"workload": mat.name, "dtype": dn, "heads": heads, "k": k, "d": d, "m": mat.m, "n": mat.n, "nnz": mat.nnz}
                    gat_step()
                    if not skip:
                        old_step()
                        torch.cuda.synchronize()
                        worst = {}
                        for name, x, y in (("O", O, O1), ("dQ", dQ, old["dQ"]), ("dK", dK, old["dK"]), ("dV", dV, dV1),
                                           ("da", old["da_new"], old["da"])):
                            worst[name] = float((x - y).abs().max() / y.abs().max().clamp_min(1e-30))
                        line["worst_relative_difference"] = {n: float(f"{v:.3e}") for n, v in worst.items()}
                        if max(worst.values()) > 2 ** 12 * u:
                            print(json.dumps(line), flush=True)
                            raise SystemExit(f"the two routes differ: {mat.name} {dn} heads={heads} k={k} d={d}: {worst}")
                        tn, to = timed(gat, lambda: old_forward() and None, args.batches, args.per_batch, args.warmup)
                        sn, so = timed(gat_step, old_step, args.batches, args.per_batch, args.warmup)
                        line.update({
                            "gat_us": r(np.median(tn)), "old_forward_us": r(np.median(to)), "old_forward_min_us": r(min(to)),
                            "old_forward_max_us": r(max(to)), "old_over_gat": round(float(np.median(to) / np.median(tn)), 2),
                            "gat_step_us": r(np.median(sn)), "old_step_us": r(np.median(so)), "old_step_min_us": r(min(so)),
                            "old_step_max_us": r(max(so)), "old_step_over_gat": round(float(np.median(so) / np.median(sn)), 2),
                            "old_step_bytes": allocated(old_step), "gat_step_bytes": allocated(gat_step),
                        })
                    else:
                        tn, _ = timed(gat, gat, args.batches, args.per_batch, args.warmup)
                        sn, _ = timed(gat_step, gat_step, args.batches, args.per_batch, args.warmup)
                        line.update({"old_route": f"skipped: its temporaries are {temporaries} bytes", "gat_us": r(np.median(tn)),
                                     "gat_step_us": r(np.median(sn)), "gat_step_bytes": allocated(gat_step)})
                    bw, bn = timed(gat_bwd, gat_bwd_no_dar, args.batches, args.per_batch, args.warmup)
                    line.update({"gat_backward_us": r(np.median(bw)), "gat_backward_no_dar_us": r(np.median(bn)),
                                 "gat_backward_no_dar_min_us": r(min(bn)), "gat_backward_no_dar_max_us": r(max(bn)),
                                 "dar_cost": round(float(np.median(bw) / np.median(bn)), 4), "launches": [1, 2]})
                    print(json.dumps(line), flush=True)
                    old.clear()
                    del Q, K, V, dO, O, dQ, dK, dV, dAr, O1, dV1, work
                    torch.cuda.empty_cache()
            A.destroy()
            A.close()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
