#!/usr/bin/env python3
"""The one-pass attention (csr5hip_attention) against the unfused chain on the same handle, one JSON line per
(workload, dtype, k, d).

    python scripts/bench_attention.py [--workloads scircuit,webbase,nd24k] [--dtypes f64,f32] [--kd 16x16,64x64]

Per line: fused_us, the median of device-event-timed batches of A.attention(Q, K, V, O) after a warm-up; unfused_us, the same
for the chain the fused call replaces -- O.zero_(), A.sddmm(Q, K, s), A.rowSoftmax(s, p), A.updateValues(p), A.spmm(V, O) -- with
s and p allocated outside the timed region and no autograd bookkeeping, in the same process, its batches alternating with the
fused call's.  Q is uniform(-1, 1) / sqrt(k), K and V uniform(-1, 1).  Before any timing the two routes are compared: they
differ by rounding only (the normalisation comes after the product in the fused call, and the sums run in another order), so
the check is |fused - unfused| <= 4 (Lmax + 2 k sqrt(k) + 16) u, u the unit roundoff and Lmax the longest row -- a sanity check
of the measurement, not the accuracy test (tests/test_gpu_fused_attention.py).  The unfused chain leaves its weights in the
handle; the fused call does not read them."""
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
from scripts.bench_sddmm import timed_pair  # noqa: E402

DEV = "cuda:0"
WORKLOADS = {
    "scircuit": lambda dt: M.scircuit_like(dtype=dt),
    "webbase": lambda dt: M.webbase_like(dtype=dt),
    "nd24k": lambda dt: M.nd24k_like(dtype=dt),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="scircuit,webbase,nd24k")
    ap.add_argument("--dtypes", default="f64,f32")
    ap.add_argument("--kd", default="16x16,64x64")
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--per-batch", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    kds = [tuple(int(v) for v in kd.split("x")) for kd in args.kd.split(",")]
    for wl in args.workloads.split(","):
        for dn in args.dtypes.split(","):
            dtype = np.float64 if dn == "f64" else np.float32
            mat = WORKLOADS[wl](dtype)
            tdt = torch.float64 if dtype == np.float64 else torch.float32
            u = float(np.finfo(dtype).eps) / 2
            lens = np.diff(mat.row_ptr)
            rp = torch.from_numpy(mat.row_ptr).to(DEV)
            ci = torch.from_numpy(mat.col).to(DEV)
            va = torch.ones(mat.nnz, dtype=tdt, device=DEV)
            A = H.anonymouslibHandle(mat.m, mat.n, dtype=np.dtype(dtype).name)
            rcs = [A.inputCSR(mat.nnz, rp, ci, va), A.setSigma(H.ANONYMOUSLIB_AUTO_TUNED_SIGMA), A.asCSR5()]
            if any(rcs):
                raise RuntimeError(f"handle setup failed: {rcs}")
            info = A.info()
            gen = torch.Generator(device=DEV).manual_seed(5)
            s = torch.empty(mat.nnz, dtype=tdt, device=DEV)
            p = torch.empty(mat.nnz, dtype=tdt, device=DEV)
            for k, d in kds:
                Q = (torch.rand((mat.m, k), dtype=tdt, device=DEV, generator=gen) * 2 - 1) / k ** 0.5
                K = torch.rand((mat.n, k), dtype=tdt, device=DEV, generator=gen) * 2 - 1
                V = torch.rand((mat.n, d), dtype=tdt, device=DEV, generator=gen) * 2 - 1
                Of = torch.empty((mat.m, d), dtype=tdt, device=DEV)
                Ou = torch.empty((mat.m, d), dtype=tdt, device=DEV)

                def fused():
                    if A.attention(Q, K, V, Of):
                        raise RuntimeError("attention failed")

                def unfused():
                    Ou.zero_()
                    if A.sddmm(Q, K, s) or A.rowSoftmax(s, p) or A.updateValues(p) or A.spmm(V, Ou):
                        raise RuntimeError("the unfused chain failed")
                Of.fill_(float("nan"))
                fused()
                unfused()
                torch.cuda.synchronize()
                tol = 4 * (int(lens.max()) + 2 * k * k ** 0.5 + 16) * u
                worst = float((Of - Ou).abs().max())
                agree = bool(worst <= tol)
                t_f, t_u = timed_pair(fused, unfused, args.batches, args.per_batch, args.per_batch, args.warmup)
                print(json.dumps({
                    "workload": mat.name, "dtype": dn, "k": k, "d": d, "m": mat.m, "n": mat.n, "nnz": mat.nnz, "sigma": info.sigma,
                    "mean_row": round(float(lens.mean()), 1), "max_row": int(lens.max()),
                    "fused_us": round(t_f, 2), "unfused_us": round(t_u, 2), "unfused_over_fused": round(t_u / t_f, 2),
                    "gflops_fused": round(2.0 * mat.nnz * (k + d) / (t_f * 1e3), 1),
                    "routes_agree": agree, "worst_difference": worst, "allowed_difference": tol,
                }), flush=True)
                if not agree:
                    raise SystemExit(f"the fused call differs from the unfused chain: {mat.name} {dn} k={k} d={d}: {worst} > {tol}")
                del Q, K, V, Of, Ou
            del s, p
            A.destroy()
            A.close()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
