#!/usr/bin/env python3
"""update_values against the round trip it replaces, one JSON line per (workload, dtype, configuration).

    python scripts/bench_refresh.py [--workloads scircuit,webbase,nd24k,rmat22] [--dtypes f64,f32]

Configurations: the library defaults, and -- where the defaults build no column slabs -- 8 slabs forced.  Per line:
update_us (updateValues), roundtrip_us (asCSR + a device copy of nnz values + asCSR5 on the same handle, steady state: not the
handle's first conversion), their ratio, update_us in units of one spmv() of that handle, and bytes moved / time as a fraction
of 8 TB/s with B = 2 s nnz for a plain handle, B = 2 s nnz + (4 + 2 s) nnz (+ 4 nnz when the values are narrowed) for a slab
handle with its source map; s = sizeof value.  Both are medians of device-event-timed batches after a warm-up (the protocol of
scripts/bench_spmm.py).  Before any timing y after an update is checked bit for bit against y after the round trip."""
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


def ok(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} -> {rc}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="scircuit,webbase,nd24k,rmat22")
    ap.add_argument("--dtypes", default="f64,f32")
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--per-batch", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
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
            default_slabs = None
            for forced in (0, 8):
                if forced and default_slabs:
                    continue  # the defaults already measured a slab handle
                rp, ci = torch.from_numpy(mat.row_ptr).to(DEV), torch.from_numpy(mat.col).to(DEV)
                va = torch.from_numpy(val).to(DEV)
                A = H.anonymouslibHandle(mat.m, mat.n, dtype=np.dtype(dtype).name)
                ok(A.inputCSR(mat.nnz, rp, ci, va), "inputCSR")
                ok(A.setSigma(H.ANONYMOUSLIB_AUTO_TUNED_SIGMA), "setSigma")
                if forced:
                    ok(A.setColumnSlabs(forced), "setColumnSlabs")
                ok(A.asCSR5(), "asCSR5")
                ok(A.setX(x), "setX")
                y = torch.full((mat.m,), 777.0, dtype=tdt, device=DEV)
                y_ref = torch.full((mat.m,), 777.0, dtype=tdt, device=DEV)

                def roundtrip():
                    ok(A.asCSR(), "asCSR")
                    va.copy_(new)
                    ok(A.asCSR5(), "asCSR5")

                def update():
                    ok(A.updateValues(new), "updateValues")

                # y after the round trip is the yardstick; the handle goes back to the old values, then takes the update
                roundtrip()
                ok(A.spmv(1.0, y_ref), "spmv")
                ok(A.asCSR(), "asCSR")
                va.copy_(torch.from_numpy(val).to(DEV))
                ok(A.asCSR5(), "asCSR5")
                update()
                ok(A.spmv(1.0, y), "spmv")
                torch.cuda.synchronize()
                identical = bool(torch.equal(y.view(iv), y_ref.view(iv)))
                info = A.info()
                if not forced:
                    default_slabs = info.column_slabs
                t_spmv = timed(lambda: ok(A.spmv(1.0, y), "spmv"), args.batches, args.per_batch, args.warmup)
                t_upd = timed(update, args.batches, args.per_batch, args.warmup)
                t_rt = timed(roundtrip, args.batches, args.per_batch, args.warmup)
                moved = 2 * s * mat.nnz
                if info.column_slabs:
                    moved += (4 + 2 * s) * mat.nnz + (4 * mat.nnz if info.slab_values_narrowed else 0)
                print(json.dumps({
                    "workload": mat.name, "dtype": dn, "config": f"slabs{forced}" if forced else "default",
                    "m": mat.m, "nnz": mat.nnz, "sigma": info.sigma, "column_slabs": info.column_slabs, "slab_hot": info.slab_hot,
                    "update_us": round(t_upd, 2), "roundtrip_us": round(t_rt, 2), "ratio": round(t_upd / t_rt, 4),
                    "update_in_spmvs": round(t_upd / t_spmv, 2), "roundtrip_in_spmvs": round(t_rt / t_spmv, 2),
                    "spmv_us": round(t_spmv, 2), "bytes_moved": moved,
                    "hbm_fraction": round(moved / (t_upd * 1e-6) / PEAK_BPS, 3),
                    "device_bytes": info.device_bytes, "y_bit_identical_to_roundtrip": identical,
                }), flush=True)
                if not identical:
                    raise SystemExit(f"y after updateValues differs from the round trip on {mat.name} {dn}")
                ok(A.destroy(), "destroy")
                A.close()


if __name__ == "__main__":
    main()
