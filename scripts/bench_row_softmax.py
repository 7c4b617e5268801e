#!/usr/bin/env python3
"""row_softmax / row_softmax_grad (csr5hip_row_softmax, csr5hip_row_softmax_grad) against the torch route, one JSON line per
(workload, dtype, operation).

    python scripts/bench_row_softmax.py [--workloads scircuit,webbase,nd24k,rmat22] [--dtypes f64,f32]

Per line: us, the median of device-event-timed batches after a warm-up; torch_us, the same for the torch route -- the maximum by
scatter_reduce("amax") and the sums by index_add over a row index built outside the timed region -- in the same process, its
batches alternating with the library's; and the fraction of 8 TB/s on the algorithmic bytes 2 s nnz + 4 (m + 1) forward,
3 s nnz + 4 (m + 1) gradient, s = sizeof value.  Before any timing the result is checked against the torch route.  Beyond
TORCH_PIECE stored elements the torch route runs in pieces of that many elements, one after the other (its index and reduction
kernels do not launch on one piece of 67 M elements).  With --hub (default for rmat22) the length of the longest row is
reported together with the time of the call on a matrix that holds that row alone: a row is never split across workgroups."""
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


def _pieces(nnz):
    return [(a, min(a + TORCH_PIECE, nnz)) for a in range(0, nnz, TORCH_PIECE)]


def torch_forward(s, rows, m):
    nnz = s.shape[0]
    mx = torch.full((m,), -float("inf"), dtype=s.dtype, device=s.device)
    for a, b in _pieces(nnz):
        mx.scatter_reduce_(0, rows[a:b], s[a:b], "amax")
    e = torch.cat([torch.exp(s[a:b] - mx[rows[a:b]]) for a, b in _pieces(nnz)]) if nnz > TORCH_PIECE else torch.exp(s - mx[rows])
    z = torch.zeros(m, dtype=s.dtype, device=s.device)
    for a, b in _pieces(nnz):
        z.index_add_(0, rows[a:b], e[a:b])
    for a, b in _pieces(nnz):
        e[a:b] /= z[rows[a:b]]
    return e


def torch_grad(p, g, rows, m):
    nnz = p.shape[0]
    d = torch.zeros(m, dtype=p.dtype, device=p.device)
    for a, b in _pieces(nnz):
        d.index_add_(0, rows[a:b], p[a:b] * g[a:b])
    if nnz <= TORCH_PIECE:
        return p * (g - d[rows])
    return torch.cat([p[a:b] * (g[a:b] - d[rows[a:b]]) for a, b in _pieces(nnz)])


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


def csr_handle(rp, nnz, m, n, dtype, tdt):
    """a handle in CSR format: the two calls read row_ptr only (the columns and values are placeholders that are never read)"""
    A = H.anonymouslibHandle(m, n, dtype=np.dtype(dtype).name)
    ci = torch.zeros(1, dtype=torch.int32, device=DEV)
    va = torch.zeros(1, dtype=tdt, device=DEV)
    A._arrays = (rp, ci, va)
    if A.inputCSR(nnz, rp, ci, va):
        raise RuntimeError("inputCSR failed")
    return A


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="scircuit,webbase,nd24k,rmat22")
    ap.add_argument("--dtypes", default="f64,f32")
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--per-batch", type=int, default=10)
    ap.add_argument("--torch-per-batch", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--hub", default="rmat22", help="workloads whose longest row is also timed alone")
    args = ap.parse_args()
    cache = {}
    for wl in args.workloads.split(","):
        for dn in args.dtypes.split(","):
            dtype = np.float64 if dn == "f64" else np.float32
            key = wl if wl == "rmat22" else (wl, dn)
            if key not in cache:
                cache.clear()
                cache[key] = WORKLOADS[wl](dtype)
            mat = cache[key]
            sz = np.dtype(dtype).itemsize
            tdt = torch.float64 if dtype == np.float64 else torch.float32
            m, nnz = mat.m, mat.nnz
            rp = torch.from_numpy(mat.row_ptr.astype(np.int32)).to(DEV)
            rows = torch.repeat_interleave(torch.arange(m, device=DEV), (rp[1:] - rp[:-1]).long())
            A = csr_handle(rp, nnz, m, mat.n, dtype, tdt)
            gen = torch.Generator(device=DEV).manual_seed(5)
            s = torch.randn(nnz, dtype=tdt, device=DEV, generator=gen) * 3
            g = torch.randn(nnz, dtype=tdt, device=DEV, generator=gen)
            p = torch.empty_like(s)
            out = torch.empty_like(s)
            tol = dict(rtol=1e-11, atol=1e-300) if dtype == np.float64 else dict(rtol=2e-4, atol=1e-30)
            if A.rowSoftmax(s, p) or A.rowSoftmaxGrad(p, g, out):
                raise RuntimeError("row_softmax failed")
            ok_f = bool(torch.allclose(p, torch_forward(s, rows, m), **tol))
            ref_g = torch_grad(p, g, rows, m)
            ok_g = bool(((out - ref_g).abs() <= tol["rtol"] * (ref_g.abs() + p)).all())
            del ref_g
            lens = np.diff(mat.row_ptr)
            common = {"workload": mat.name, "dtype": dn, "m": m, "nnz": nnz, "longest_row": int(lens.max())}
            for op, f, t, nbytes, ok in (
                    ("forward", lambda: A.rowSoftmax(s, p), lambda: torch_forward(s, rows, m), 2 * sz * nnz + 4 * (m + 1), ok_f),
                    ("gradient", lambda: A.rowSoftmaxGrad(p, g, out), lambda: torch_grad(p, g, rows, m),
                     3 * sz * nnz + 4 * (m + 1), ok_g)):
                t_lib, t_torch = timed_pair(f, t, args.batches, args.per_batch, args.torch_per_batch, args.warmup)
                print(json.dumps(dict(common, op=op, us=round(t_lib, 2), torch_us=round(t_torch, 2),
                                      speedup_vs_torch=round(t_torch / t_lib, 2),
                                      hbm_fraction=round(nbytes / (t_lib * 1e-6) / PEAK_BPS, 3), matches_torch=ok)), flush=True)
                if not ok:
                    raise SystemExit(f"{op} differs from the torch route: {mat.name} {dn}")
            A.close()
            del rows
            if wl in args.hub.split(","):
                L = int(lens.max())
                rp1 = torch.tensor([0, L], dtype=torch.int32, device=DEV)
                B = csr_handle(rp1, L, 1, mat.n, dtype, tdt)
                s1, g1, p1, o1 = s[:L].clone(), g[:L].clone(), torch.empty(L, dtype=tdt, device=DEV), torch.empty(L, dtype=tdt, device=DEV)
                B.rowSoftmax(s1, p1)
                t_f, t_g = timed_pair(lambda: B.rowSoftmax(s1, p1), lambda: B.rowSoftmaxGrad(p1, g1, o1), args.batches,
                                      args.per_batch, args.per_batch, args.warmup)
                print(json.dumps({"workload": mat.name + ": longest row alone", "dtype": dn, "row_length": L,
                                  "forward_us": round(t_f, 2), "gradient_us": round(t_g, 2)}), flush=True)
                B.close()
            del s, g, p, out
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
