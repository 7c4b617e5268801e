#!/usr/bin/env python3
"""sddmm (csr5hip_sddmm) against the torch route, one JSON line per (workload, dtype, k).

    python scripts/bench_sddmm.py [--workloads scircuit,webbase,nd24k,rmat22] [--dtypes f64,f32] [--ks 4,8,16,32,64]

Per line: sddmm_us, the median of device-event-timed batches after a warm-up; torch_us, the same for the torch expression
(U[rows] * V[cols]).sum(1) with rows and cols built outside the timed region, in the same process, its batches alternating
with sddmm's; and the fraction of 8 TB/s on the algorithmic bytes nnz (4 + s) + s k (m + n) + tile_desc + tile_ptr, s = sizeof
value (the column word and the output per element, U and V once, the tile structure once).  Before any timing the result is
checked against the torch route on integer data, exactly.  Beyond TORCH_PIECE stored elements the torch expression is evaluated in
pieces of that many elements, one after the other (its index and reduction kernels do not launch on one piece of 67 M rows)."""
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


TORCH_PIECE = 1 << 25


def torch_route(U, V, rows, cols):
    nnz = rows.shape[0]
    if nnz <= TORCH_PIECE:
        return (U[rows] * V[cols]).sum(1)
    return torch.cat([(U[rows[a:a + TORCH_PIECE]] * V[cols[a:a + TORCH_PIECE]]).sum(1) for a in range(0, nnz, TORCH_PIECE)])


def batch_us(fn, per_batch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(per_batch):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / per_batch


def timed_pair(f, g, batches, per_f, per_g, warmup):
    """medians (us per call) of f and of g, their batches alternating"""
    for _ in range(warmup):
        f()
    for _ in range(min(warmup, 2)):
        g()
    torch.cuda.synchronize()
    tf, tg = [], []
    for _ in range(batches):
        tf.append(batch_us(f, per_f))
        tg.append(batch_us(g, per_g))
    return float(np.median(tf)), float(np.median(tg))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="scircuit,webbase,nd24k,rmat22")
    ap.add_argument("--dtypes", default="f64,f32")
    ap.add_argument("--ks", default="4,8,16,32,64")
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--per-batch", type=int, default=10)
    ap.add_argument("--torch-per-batch", type=int, default=3)
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
            tdt = torch.float64 if dtype == np.float64 else torch.float32
            rp = torch.from_numpy(mat.row_ptr).to(DEV)
            ci = torch.from_numpy(mat.col).to(DEV)
            va = torch.ones(mat.nnz, dtype=tdt, device=DEV)
            rows = torch.repeat_interleave(torch.arange(mat.m, device=DEV), (rp[1:] - rp[:-1]).long())
            cols = ci[:mat.nnz].long()  # (before asCSR5 permutes ci in place)
            A = H.anonymouslibHandle(mat.m, mat.n, dtype=np.dtype(dtype).name)
            rcs = [A.inputCSR(mat.nnz, rp, ci, va), A.setSigma(H.ANONYMOUSLIB_AUTO_TUNED_SIGMA), A.asCSR5()]
            if any(rcs):
                raise RuntimeError(f"handle setup failed: {rcs}")
            info = A.info()
            structure = 4 * info.p * info.omega * info.num_packet + 4 * (info.p + 1)
            gen = torch.Generator(device=DEV).manual_seed(5)
            out = torch.empty(mat.nnz, dtype=tdt, device=DEV)
            for k in ks:
                # exact on integer data, before any timing
                Ui = torch.randint(-4, 5, (mat.m, k), device=DEV, generator=gen).to(tdt)
                Vi = torch.randint(-4, 5, (mat.n, k), device=DEV, generator=gen).to(tdt)
                out.fill_(777.0)
                if A.sddmm(Ui, Vi, out):
                    raise RuntimeError("sddmm failed")
                exact = bool(torch.equal(out, torch_route(Ui, Vi, rows, cols)))
                del Ui, Vi
                U = torch.rand((mat.m, k), dtype=tdt, device=DEV, generator=gen) * 2 - 1
                V = torch.rand((mat.n, k), dtype=tdt, device=DEV, generator=gen) * 2 - 1
                t_sddmm, t_torch = timed_pair(lambda: A.sddmm(U, V, out), lambda: torch_route(U, V, rows, cols), args.batches,
                                              args.per_batch, args.torch_per_batch, args.warmup)
                b_alg = mat.nnz * (4 + s) + s * k * (mat.m + mat.n) + structure
                print(json.dumps({
                    "workload": mat.name, "dtype": dn, "k": k, "m": mat.m, "n": mat.n, "nnz": mat.nnz, "sigma": info.sigma,
                    "sddmm_us": round(t_sddmm, 2), "torch_us": round(t_torch, 2), "speedup_vs_torch": round(t_torch / t_sddmm, 2),
                    "gflops": round(2.0 * mat.nnz * k / (t_sddmm * 1e3), 1),
                    "hbm_fraction": round(b_alg / (t_sddmm * 1e-6) / PEAK_BPS, 3),
                    "exact_on_integer_data": exact,
                }), flush=True)
                if not exact:
                    raise SystemExit(f"sddmm differs from the torch route on integer data: {mat.name} {dn} k={k}")
                del U, V
            del rows, cols, out
            A.destroy()
            A.close()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
