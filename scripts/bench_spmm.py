#!/usr/bin/env python3
"""SpMM (csr5hip_spmm) against k SpMVs, one JSON line per (workload, dtype, k).

    python scripts/bench_spmm.py [--workloads scircuit,webbase,nd24k,rmat22] [--dtypes f64,f32] [--ks 1,2,4,8,16]

Per line: the SpMM time (median of device-event-timed batches after a warm-up), k x the spmv() time at library defaults and
k x the spmv() time on the plain two-pass path (CSR5HIP_OPT_SPMV_MODE = 0, no column slabs) in the same process, GFLOPS =
2 nnz k / t, and the fraction of 8 TB/s on B_spmm = nnz (4 + s) + 4 (m + 1) + s k (n + m), s = sizeof value.  Before any
timing, column 0 of Y is checked bit for bit against the two-pass spmv() of X[:, 0]."""
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
from benchmark_spmv_using_csr5_amd import matrices as M  # noqa: E402

DEV = "cuda:0"
PEAK_BPS = 8e12
WORKLOADS = {
    "scircuit": lambda dt: M.scircuit_like(dtype=dt),
    "webbase": lambda dt: M.webbase_like(dtype=dt),
    "nd24k": lambda dt: M.nd24k_like(dtype=dt),
    "rmat22": lambda dt: M.rmat(22, 16),
}


def timed(fn, batches, per_batch, warmup):
    """median over batches of (device time of per_batch calls) / per_batch, in microseconds"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(batches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(per_batch):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / per_batch)
    return float(np.median(out))


def make(mat, val, sigma, dtype, plain):
    rp = torch.from_numpy(mat.row_ptr).to(DEV)
    ci = torch.from_numpy(mat.col).to(DEV)
    va = torch.from_numpy(val).to(DEV)
    A = H.anonymouslibHandle(mat.m, mat.n, dtype=np.dtype(dtype).name)
    A._arrays = (rp, ci, va)
    rcs = [A.inputCSR(mat.nnz, rp, ci, va), A.setSigma(sigma)]
    if plain:
        rcs.append(A.setSpmvMode(H.SPMV_TWO_PASS))
    rcs.append(A.asCSR5())
    if plain:
        rcs.append(A.setColumnSlabs(0))
    if any(rcs):
        raise RuntimeError(f"handle setup failed: {rcs}")
    return A


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="scircuit,webbase,nd24k,rmat22")
    ap.add_argument("--dtypes", default="f64,f32")
    ap.add_argument("--ks", default="1,2,4,8,16")
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--per-batch", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    ks = [int(k) for k in args.ks.split(",")]
    cache = {}
    for wl in args.workloads.split(","):
        for dn in args.dtypes.split(","):
            dtype = np.float64 if dn == "f64" else np.float32
            key = wl if wl == "rmat22" else (wl, dn)
            if key not in cache:
                cache.clear()
                cache[key] = WORKLOADS[wl](dtype)
            mat = cache[key]
            s = np.dtype(dtype).itemsize
            val, _ = M.fill_values(mat.nnz, mat.n, dtype, seed=1, mode="real")
            D = make(mat, val, H.ANONYMOUSLIB_AUTO_TUNED_SIGMA, dtype, plain=False)
            P = make(mat, val, H.ANONYMOUSLIB_AUTO_TUNED_SIGMA, dtype, plain=True)
            sigma = P.info().sigma
            tdt = torch.float64 if dtype == np.float64 else torch.float32
            gen = torch.Generator(device=DEV).manual_seed(5)
            x = torch.rand(mat.n, dtype=tdt, device=DEV, generator=gen) * 2 - 1
            y = torch.zeros(mat.m, dtype=tdt, device=DEV)
            if D.setX(x) or P.setX(x):
                raise RuntimeError("setX failed")
            t_def = timed(lambda: D.spmv(1.0, y), args.batches, args.per_batch, args.warmup)
            t_plain = timed(lambda: P.spmv(1.0, y), args.batches, args.per_batch, args.warmup)
            info = D.info()
            for k in ks:
                X = torch.rand((mat.n, k), dtype=tdt, device=DEV, generator=gen) * 2 - 1
                Y = torch.full((mat.m, k), 777.0, dtype=tdt, device=DEV)
                # bit identity of column 0 against the two-pass spmv before any timing
                x0 = X[:, 0].contiguous()
                y0 = torch.full((mat.m,), 777.0, dtype=tdt, device=DEV)
                if P.setX(x0) or P.spmv(1.0, y0) or D.spmm(X, Y):
                    raise RuntimeError("spmv / spmm failed")
                torch.cuda.synchronize()
                iv = torch.int64 if s == 8 else torch.int32
                identical = bool(torch.equal(Y[:, 0].contiguous().view(iv), y0.view(iv)))
                t_spmm = timed(lambda: D.spmm(X, Y), args.batches, args.per_batch, args.warmup)
                b_spmm = mat.nnz * (4 + s) + 4 * (mat.m + 1) + s * k * (mat.n + mat.m)
                print(json.dumps({
                    "workload": mat.name, "dtype": dn, "k": k, "m": mat.m, "n": mat.n, "nnz": mat.nnz, "sigma": sigma,
                    "spmm_us": round(t_spmm, 2), "k_spmv_default_us": round(k * t_def, 2),
                    "k_spmv_plain_us": round(k * t_plain, 2),
                    "speedup_vs_plain": round(k * t_plain / t_spmm, 3), "speedup_vs_default": round(k * t_def / t_spmm, 3),
                    "gflops": round(2.0 * mat.nnz * k / (t_spmm * 1e3), 1),
                    "hbm_fraction": round(b_spmm / (t_spmm * 1e-6) / PEAK_BPS, 3),
                    "default_path": {"column_slabs": info.column_slabs, "slab_hot": info.slab_hot},
                    "column0_bit_identical": identical,
                }), flush=True)
                if not identical:
                    raise SystemExit(f"column 0 of SpMM differs from spmv on {mat.name} {dn} k={k}")
            for A in (D, P):
                A.destroy()
                A.close()


if __name__ == "__main__":
    main()
