#!/usr/bin/env python3
"""csr5hip_spmm_reduce (max over a row's entries of a_e X[col(e), :], with the argmax) and its backward against two baselines on the
same data, one JSON line per (workload, dtype, k).

    python scripts/bench_spmm_reduce.py [--workloads scircuit,webbase,nd24k] [--dtypes f32,f64] [--ks 16,64]

Baseline A, the torch route: prebuilt int64 row and column index tensors, t = X[cols] * val[:, None] (two nnz k temporaries), then
out.scatter_reduce_(0, idx, t, "amax", include_self=False).  Its backward is torch autograd through that expression.
Baseline B, A.spmm on the same handle at the same k: the same gathers with a sum in the maximum's place, the floor to read the kernel
against (it writes no arg).  For the backward B is A.sddmm + A.spmmT, the gradients of the sum.
bench_mha.py's protocol: the routes' batches alternating in one process, device events, medians of 7 batches of 10 calls after a warm-up;
each baseline's fastest and slowest batch are reported (the spread is the margin of any claim).  Before any timing the kernel's values
are compared with baseline A's bit for bit (they are defined to be equal) and its gradients to rounding.
bytes: the algorithmic traffic of the forward -- every entry's column and value once, one gathered row of X per entry, Y and arg
written once -- and roof_pct its rate against 8 TB/s; a gathered row that hits in a cache costs less than this counts."""
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
from scripts.bench_sddmm import batch_us  # noqa: E402

ROOF_BYTES_PER_US = 8e12 / 1e6


def timed(fs, batches, per_batch, warmup):
    """per-batch times (us per call) of every function of fs, their batches alternating"""
    for f in fs:
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    ts = [[] for _ in fs]
    for _ in range(batches):
        for t, f in zip(ts, fs):
            t.append(batch_us(f, per_batch))
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="scircuit,webbase,nd24k")
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--ks", default="16,64")
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--per-batch", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    for wl in args.workloads.split(","):
        for dn in args.dtypes.split(","):
            dtype = np.float64 if dn == "f64" else np.float32
            mat = WORKLOADS[wl](dtype)
            tdt = torch.float64 if dtype == np.float64 else torch.float32
            vs = 8 if dtype == np.float64 else 4
            rows = torch.from_numpy(np.repeat(np.arange(mat.m, dtype=np.int64), np.diff(mat.row_ptr))).to(DEV)
            cols = torch.from_numpy(mat.col[:mat.nnz].astype(np.int64)).to(DEV)
            rp = torch.from_numpy(mat.row_ptr).to(DEV)
            ci = torch.from_numpy(mat.col).to(DEV)
            gen = torch.Generator(device=DEV).manual_seed(5)
            val = torch.rand(mat.nnz, dtype=tdt, device=DEV, generator=gen) + 0.5
            A = H.anonymouslibHandle(mat.m, mat.n, dtype=np.dtype(dtype).name)
            rcs = [A.inputCSR(mat.nnz, rp, ci, val.clone()), A.setSigma(H.ANONYMOUSLIB_AUTO_TUNED_SIGMA), A.asCSR5(), A.buildTranspose()]
            if any(rcs):
                raise RuntimeError(f"handle setup failed: {rcs}")
            for k in (int(v) for v in args.ks.split(",")):
                X = torch.rand((mat.n, k), dtype=tdt, device=DEV, generator=gen) * 2 - 1
                G = torch.rand((mat.m, k), dtype=tdt, device=DEV, generator=gen) * 2 - 1
                Y, Ys = torch.empty((mat.m, k), dtype=tdt, device=DEV), torch.zeros((mat.m, k), dtype=tdt, device=DEV)
                arg = torch.empty((mat.m, k), dtype=torch.int32, device=DEV)
                dX, dXs = torch.empty((mat.n, k), dtype=tdt, device=DEV), torch.zeros((mat.n, k), dtype=tdt, device=DEV)
                dval, dvals = torch.empty(mat.nnz, dtype=tdt, device=DEV), torch.empty(mat.nnz, dtype=tdt, device=DEV)
                idx = rows[:, None].expand(-1, k)
                Xg, vg = X.clone().requires_grad_(True), val.clone().requires_grad_(True)

                def torch_forward(x=X, v=val):
                    out = torch.zeros((mat.m, k), dtype=tdt, device=DEV)
                    return out.scatter_reduce(0, idx, x[cols] * v[:, None], "amax", include_self=False)

                def ours():
                    if A.spmmReduce(X, Y, "max", arg, True):
                        raise RuntimeError("spmmReduce failed")

                def sum_floor():
                    if A.spmm(X, Ys):
                        raise RuntimeError("spmm failed")

                def ours_both():
                    ours()
                    if A.spmmReduceBackward(X, G, arg, dX, dval, True):
                        raise RuntimeError("spmmReduceBackward failed")

                def torch_both():
                    gv, gx = torch.autograd.grad(torch_forward(Xg, vg), (vg, Xg), G)
                    return gv, gx

                def sum_both():
                    sum_floor()
                    if A.sddmm(G, X, dvals) or A.spmmT(G, dXs):
                        raise RuntimeError("sddmm / spmmT failed")
                ours_both()
                want = torch_forward()
                gv, gx = torch_both()
                torch.cuda.synchronize()
                same_bits = torch.equal(Y, want)
                close = bool(torch.allclose(dval, gv, rtol=1e-4 if vs == 4 else 1e-12, atol=1e-5 if vs == 4 else 1e-13) and
                             torch.allclose(dX, gx, rtol=1e-4 if vs == 4 else 1e-12, atol=1e-4 if vs == 4 else 1e-12))
                del want, gv, gx
                tf = timed((ours, torch_forward, sum_floor), args.batches, args.per_batch, args.warmup)
                tb = timed((ours_both, torch_both, sum_both), args.batches, args.per_batch, args.warmup)
                nbytes = 4 * (mat.m + 1) + mat.nnz * (4 + vs) + mat.nnz * k * vs + mat.m * k * (vs + 4)
                r = lambda v: round(float(v), 2)  # noqa: E731
                med = [np.median(t) for t in tf + tb]
                print(json.dumps({
                    "workload": mat.name, "dtype": dn, "k": k, "m": mat.m, "n": mat.n, "nnz": mat.nnz, "same_bits": same_bits,
                    "gradients_close": close,
                    "reduce_us": r(med[0]), "torch_us": r(med[1]), "torch_min_us": r(min(tf[1])), "torch_max_us": r(max(tf[1])),
                    "spmm_us": r(med[2]), "spmm_min_us": r(min(tf[2])), "spmm_max_us": r(max(tf[2])),
                    "reduce_fwd_bwd_us": r(med[3]), "torch_fwd_bwd_us": r(med[4]), "torch_fwd_bwd_min_us": r(min(tb[1])),
                    "torch_fwd_bwd_max_us": r(max(tb[1])), "spmm_fwd_bwd_us": r(med[5]), "spmm_fwd_bwd_min_us": r(min(tb[2])),
                    "spmm_fwd_bwd_max_us": r(max(tb[2])),
                    "bytes": nbytes, "roof_pct": r(100 * nbytes / med[0] / ROOF_BYTES_PER_US),
                }), flush=True)
                if not same_bits:
                    raise SystemExit(f"spmmReduce differs from the torch route: {mat.name} {dn} k={k}")
                del X, G, Y, Ys, arg, dX, dXs, dval, dvals, Xg, vg, idx
                torch.cuda.empty_cache()
            A.destroy()
            A.close()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
