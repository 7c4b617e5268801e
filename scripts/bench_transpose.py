#!/usr/bin/env python3
"""The transposed product (buildTranspose / spmvT) against the route it replaces, one JSON line per (workload, dtype).

    python scripts/bench_transpose.py [--workloads scircuit,webbase,nd24k,rmat22] [--dtypes f64,f32]

Per line, at library defaults:
* spmvT_us against hand_us, the spmv() of a handle built by hand from matrices.transpose_csr (same sigma request, same options):
  both sides alternated in the same process, each timed TWICE (two separate medians of device-event-timed batches after a
  warm-up, the protocol of scripts/bench_spmm.py).  They run the same kernels on the same bytes: the expected ratio is 1 and the
  margin is the relative spread of the hand-built handle against itself plus that of spmvT against itself (`within_spread`).
* build_ms (buildTranspose, host clock around a device synchronise, median over reconversions) against host_route_ms: device-to-
  host copy of the three CSR arrays, transpose_csr in numpy, host-to-device copy, inputCSR + asCSR5 of the second handle; and in
  units of the parent's own asCSR5() (as_csr5_ms, same clock).
* update_us with and without the companion on the same handle.
* device_bytes with and without the companion, next to the expectation nnz (4 + s) + 4 (n + 1) + 4 nnz + s nnz + the companion's
  own CSR5 arrays and tables; s = sizeof value.
Before any timing y = A^T x is checked bit for bit against the hand-built handle."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from benchmark_spmv_using_csr5_amd import handle as H  # noqa: E402
from benchmark_spmv_using_csr5_amd import matrices as M  # noqa: E402

DEV = "cuda:0"
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


def ok(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} -> {rc}")


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def convert(m, n, nnz, rp, ci, va, dtype):
    A = H.anonymouslibHandle(m, n, dtype=np.dtype(dtype).name)
    A._arrays = (rp, ci, va)
    ok(A.inputCSR(nnz, rp, ci, va), "inputCSR")
    ok(A.setSigma(H.ANONYMOUSLIB_AUTO_TUNED_SIGMA), "setSigma")
    ok(A.asCSR5(), "asCSR5")
    return A


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="scircuit,webbase,nd24k,rmat22")
    ap.add_argument("--dtypes", default="f64,f32")
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--per-batch", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--builds", type=int, default=3)
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
            s = np.dtype(dtype).itemsize
            tdt = torch.float64 if dtype == np.float64 else torch.float32
            iv = torch.int64 if s == 8 else torch.int32
            val, _ = M.fill_values(mat.nnz, mat.n, dtype, seed=1, mode="real")
            gen = torch.Generator(device=DEV).manual_seed(5)
            new = torch.rand(mat.nnz, dtype=tdt, device=DEV, generator=gen) * 2 - 1
            x = torch.rand(mat.n, dtype=tdt, device=DEV, generator=gen) * 2 - 1
            xt = torch.rand(mat.m, dtype=tdt, device=DEV, generator=gen) * 2 - 1
            # an untouched device copy of the CSR arrays: what a caller who transposes by hand starts from
            rp0, ci0 = torch.from_numpy(mat.row_ptr).to(DEV), torch.from_numpy(mat.col).to(DEV)
            va0 = torch.from_numpy(val).to(DEV)
            hand = {}

            def host_route():
                hrp, hci, hva = rp0.cpu().numpy(), ci0.cpu().numpy(), va0.cpu().numpy()
                T = M.transpose_csr(M.CsrMatrix(mat.m, mat.n, hrp, hci, hva, mat.name))
                rp, ci, va = (torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (T.row_ptr, T.col, T.val))
                old = hand.pop("B", None)
                if old is not None:
                    old.close()
                hand["B"] = convert(mat.n, mat.m, mat.nnz, rp, ci, va, dtype)

            t_host = float(np.median([wall_ms(host_route) for _ in range(args.builds)]))
            B = hand["B"]
            ok(B.setX(xt), "setX")
            A = convert(mat.m, mat.n, mat.nnz, rp0.clone(), ci0.clone(), va0.clone(), dtype)
            ok(A.setX(x), "setX")
            y = torch.full((mat.m,), 777.0, dtype=tdt, device=DEV)
            yt = torch.full((mat.n,), 777.0, dtype=tdt, device=DEV)
            yt_ref = torch.full((mat.n,), 777.0, dtype=tdt, device=DEV)

            def update():
                ok(A.updateValues(new), "updateValues")

            t_upd_without = timed(update, args.batches, args.per_batch, args.warmup)
            bytes_without = A.info().device_bytes  # (with column slabs: the update's own helper included)
            ok(A.updateValues(va0), "updateValues")
            # build time over reconversions, next to the parent's own asCSR5()
            t_build, t_conv = [], []
            for _ in range(args.builds):
                ok(A.asCSR(), "asCSR")
                t_conv.append(wall_ms(lambda: ok(A.asCSR5(), "asCSR5")))
                t_build.append(wall_ms(lambda: ok(A.buildTranspose(), "buildTranspose")))
            t_build, t_conv = float(np.median(t_build)), float(np.median(t_conv))
            info = A.info()
            binfo = B.info()
            ok(A.spmvT(xt, yt), "spmvT")
            ok(B.spmv(1.0, yt_ref), "spmv")
            torch.cuda.synchronize()
            identical = bool(torch.equal(yt.view(iv), yt_ref.view(iv)))
            if not identical:
                raise SystemExit(f"spmvT differs from the hand-built handle of the transpose on {mat.name} {dn}")

            def f_t():  # (the raw-pointer call, like spmv(): the tensor checks of spmvT() cost a launch-bound SpMV 10 % in host time)
                ok(A.spmvT_ptr(xt, yt), "spmvT")

            def f_hand():
                ok(B.spmv(1.0, yt_ref), "spmv")

            h1 = timed(f_hand, args.batches, args.per_batch, args.warmup)
            t1 = timed(f_t, args.batches, args.per_batch, args.warmup)
            h2 = timed(f_hand, args.batches, args.per_batch, args.warmup)
            t2 = timed(f_t, args.batches, args.per_batch, args.warmup)
            spread_h, spread_t = abs(h1 - h2) / min(h1, h2), abs(t1 - t2) / min(t1, t2)
            ratio = (t1 + t2) / (h1 + h2)
            t_upd_with = timed(update, args.batches, args.per_batch, args.warmup)
            t_spmv = timed(lambda: ok(A.spmv(1.0, y), "spmv"), args.batches, args.per_batch, args.warmup)
            bytes_with = A.info().device_bytes
            print(json.dumps({
                "workload": mat.name, "dtype": dn, "m": mat.m, "n": mat.n, "nnz": mat.nnz,
                "sigma": info.sigma, "t_sigma": info.t_sigma, "t_column_slabs": info.t_column_slabs, "t_slab_hot": info.t_slab_hot,
                "t_x_window_active": info.t_x_window_active,
                "same_variant_as_hand_built": [info.t_sigma, info.t_p, info.t_column_slabs, info.t_slab_hot, info.t_x_window_active]
                == [binfo.sigma, binfo.p, binfo.column_slabs, binfo.slab_hot, binfo.x_window_active],
                "spmvT_us": [round(t1, 2), round(t2, 2)], "hand_us": [round(h1, 2), round(h2, 2)], "ratio": round(ratio, 4),
                "spread_hand": round(spread_h, 4), "spread_spmvT": round(spread_t, 4),
                "within_spread": bool(abs(ratio - 1) <= spread_h + spread_t),
                "spmv_us": round(t_spmv, 2),
                "build_ms": round(t_build, 3), "build_device_ms": round(info.t_transpose_build_ms, 3),
                "host_route_ms": round(t_host, 3), "as_csr5_ms": round(t_conv, 3), "build_in_as_csr5": round(t_build / t_conv, 2),
                "host_route_over_build": round(t_host / t_build, 1),
                "update_us_without": round(t_upd_without, 2), "update_us_with": round(t_upd_with, 2),
                "update_ratio": round(t_upd_with / t_upd_without, 2),
                "device_bytes_without": bytes_without, "device_bytes_with": bytes_with,
                "device_bytes_added": bytes_with - bytes_without,
                "expected_added_floor": mat.nnz * (8 + 2 * s) + 4 * (mat.n + 1),
                "yT_bit_identical_to_hand_built": identical,
            }), flush=True)
            ok(A.destroy(), "destroy")
            A.close()
            ok(B.destroy(), "destroy")
            B.close()
            hand.clear()


if __name__ == "__main__":
    main()
