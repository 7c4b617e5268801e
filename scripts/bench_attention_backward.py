#!/usr/bin/env python3
"""The fused attention backward (csr5hip_attention_backward) against the "recompute" backward on the same handle, one JSON line per
(workload, dtype, k, d).

    python scripts/bench_attention_backward.py [--workloads scircuit,webbase,nd24k] [--dtypes f64,f32] [--kd 16x16,64x64]

Both routes are timed as autograd runs them: one forward of ``autograd.fused_attention(A, Q, K, V, backward=mode)`` per mode
outside the timed region, then ``torch.autograd.grad(out, (Q, K, V), dO, retain_graph=True)`` -- the backward alone, with all
three gradients wanted, including the allocations each route makes.  fused_us / recompute_us are the medians of
device-event-timed batches after a warm-up (the first backward builds the transposed companion: warm-up), the two routes'
batches alternating in one process.  The recompute route is the previous backward: sddmm, rowSoftmax, updateValues, spmm
recomputed, then differentiated through sddmm, rowSoftmaxGrad, two more updateValues, spmm and two spmmT.
launches: device kernels and memsets per backward, counted by torch's profiler over one backward of each route (null where the
profiler is not available).  Q is uniform(-1, 1) / sqrt(k), K, V and dO uniform(-1, 1).  Before any timing the two routes are
compared: they differ by rounding only, and the check |fused - recompute| <= 8 (Lrow + Lcol + 2 k sqrt(k) + d + 16) u max(1,
max |recompute|) is a sanity check of the measurement, not the accuracy test (tests/test_gpu_attention_backward.py)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from benchmark_spmv_using_csr5_amd import autograd  # noqa: E402
from benchmark_spmv_using_csr5_amd import handle as H  # noqa: E402
from benchmark_spmv_using_csr5_amd import matrices as M  # noqa: E402
from scripts.bench_sddmm import timed_pair  # noqa: E402

DEV = "cuda:0"
WORKLOADS = {
    "scircuit": lambda dt: M.scircuit_like(dtype=dt),
    "webbase": lambda dt: M.webbase_like(dtype=dt),
    "nd24k": lambda dt: M.nd24k_like(dtype=dt),
}


def count_launches(fn):
    """device kernels + memsets of one call of fn, or None"""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
        return n or None
    except Exception:  # noqa: BLE001  (a build of torch without the profiler's device side)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="scircuit,webbase,nd24k")
    ap.add_argument("--dtypes", default="f64,f32")
    ap.add_argument("--kd", default="16x16,64x64")
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--per-batch", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-launch-count", action="store_true")
    args = ap.parse_args()
    kds = [tuple(int(v) for v in kd.split("x")) for kd in args.kd.split(",")]
    for wl in args.workloads.split(","):
        for dn in args.dtypes.split(","):
            dtype = np.float64 if dn == "f64" else np.float32
            mat = WORKLOADS[wl](dtype)
            tdt = torch.float64 if dtype == np.float64 else torch.float32
            u = float(np.finfo(dtype).eps) / 2
            lens = np.diff(mat.row_ptr)
            col_lens = np.bincount(mat.col[:mat.nnz], minlength=mat.n)
            rp = torch.from_numpy(mat.row_ptr).to(DEV)
            ci = torch.from_numpy(mat.col).to(DEV)
            va = torch.ones(mat.nnz, dtype=tdt, device=DEV)
            A = H.anonymouslibHandle(mat.m, mat.n, dtype=np.dtype(dtype).name)
            rcs = [A.inputCSR(mat.nnz, rp, ci, va), A.setSigma(H.ANONYMOUSLIB_AUTO_TUNED_SIGMA), A.asCSR5(), A.buildTranspose()]
            if any(rcs):
                raise RuntimeError(f"handle setup failed: {rcs}")
            info = A.info()
            gen = torch.Generator(device=DEV).manual_seed(5)
            for k, d in kds:
                Q = ((torch.rand((mat.m, k), dtype=tdt, device=DEV, generator=gen) * 2 - 1) / k ** 0.5).requires_grad_(True)
                K = (torch.rand((mat.n, k), dtype=tdt, device=DEV, generator=gen) * 2 - 1).requires_grad_(True)
                V = (torch.rand((mat.n, d), dtype=tdt, device=DEV, generator=gen) * 2 - 1).requires_grad_(True)
                dO = torch.rand((mat.m, d), dtype=tdt, device=DEV, generator=gen) * 2 - 1
                outs = {mode: autograd.fused_attention(A, Q, K, V, backward=mode) for mode in ("fused", "recompute")}

                def fused():
                    return torch.autograd.grad(outs["fused"], (Q, K, V), dO, retain_graph=True)

                def recompute():
                    return torch.autograd.grad(outs["recompute"], (Q, K, V), dO, retain_graph=True)
                gf, gr = fused(), recompute()
                torch.cuda.synchronize()
                base = 8 * (int(lens.max()) + int(col_lens.max()) + 2 * k * k ** 0.5 + d + 16) * u
                worst, agree = 0.0, True
                for f, r in zip(gf, gr):
                    diff, tol = float((f - r).abs().max()), base * max(1.0, float(r.abs().max()))
                    worst, agree = max(worst, diff / tol), agree and diff <= tol
                del gf, gr
                launches = (None, None) if args.no_launch_count else (count_launches(fused), count_launches(recompute))
                t_f, t_r = timed_pair(fused, recompute, args.batches, args.per_batch, args.per_batch, args.warmup)
                print(json.dumps({
                    "workload": mat.name, "dtype": dn, "k": k, "d": d, "m": mat.m, "n": mat.n, "nnz": mat.nnz, "sigma": info.sigma,
                    "t_sigma": info.t_sigma, "mean_row": round(float(lens.mean()), 1), "max_row": int(lens.max()),
                    "max_column": int(col_lens.max()),
                    "fused_us": round(t_f, 2), "recompute_us": round(t_r, 2), "recompute_over_fused": round(t_r / t_f, 2),
                    "launches_fused": launches[0], "launches_recompute": launches[1],
                    "routes_agree": agree, "worst_difference_over_allowed": worst,
                }), flush=True)
                if not agree:
                    raise SystemExit(f"the fused backward differs from the recompute route: {mat.name} {dn} k={k} d={d}: {worst}")
                del Q, K, V, dO, outs
            A.destroy()
            A.close()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
