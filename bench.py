#!/usr/bin/env python3
"""bench.py -- CSR5 SpMV throughput on N MI355X GPUs of one node (one process per GPU).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload rmat24|scircuit|webbase|nd24k|rmat<S>]
                    [--full] [--dump-outputs DIR]

A "step" is one SpMV pass (one ``spmv()`` call: y = A*x) over the rank's matrix shard, with every input already
resident in HBM.  The default workload is BASELINE.json configs[3], the configuration the metric spans: synthetic
R-MAT scale 24 (16.7 M rows, 268 M non-zeros, fp64), STRONG scaling: ONE global matrix cut into N cost-balanced (nnz + 2 * rows) row
blocks, x replicated by ONE RCCL broadcast before the loop, no per-step collective.  At N = 1
the whole matrix sits on one GPU (3.56 GB of algorithmic bytes per SpMV), so the N = 1 value is the first point of
the 1 -> 8 curve.  value = 2 * nnz_total * K / (max-over-ranks wall time of the K steps).

`python bench.py --gpus N` without a launcher starts the N ranks itself (re-exec under torch.distributed.run);
under a launcher (WORLD_SIZE set) it is one rank of N.

A plain run sets up, warms up, times the K steps and prints the JSON line (headline keys, `config`, and `roofline`
computed from the timed steps alone).  --dump-outputs DIR also writes y of the last timed step as DIR/*.npy (see
dump_outputs).  Everything that takes runs or checks of its own is behind --full; with it the JSON line also carries:
  roofline     -- side figures (x captured once per setX, narrowed values), the COLD protocol for a cache-sized working
                  set, and the CSR -> CSR5 conversion figures (median of a few asCSR / asCSR5 rounds)
  cpu_baseline -- the reference's own CSR5_avx2 (oracle/_ref, kind "reference") or our C port of it (kind "port")
                  timed on this node's host cores on the same matrix (rank 0; N > 1: also every rank's exact check and the
                  whole matrix on rank 0's GPU under the same protocol)
  configs      -- (N = 1) the other BASELINE GPU configs (scircuit-like, webbase-like fp64; nd24k-like fp32), each
                  with a cache-WARM figure (back-to-back SpMVs on one matrix, as the reference CLI times them) and
                  a COLD one (the timed loop rotates over copies whose total footprint exceeds the 256-MiB Infinity
                  Cache, so every SpMV streams from HBM), and the locality-bracket points
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import socket
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # /opt/skills/guides/MI355X_MICROARCH.md: 8.0 TB/s spec (6.29 TB/s measured copy)
INFINITY_CACHE_BYTES = 256 * 1024 * 1024
DUMP_BUDGET_BYTES = 60 * 1000 * 1000  # --dump-outputs: all .npy files of one run together (below 64 MB with room to spare)
DUMP_SAMPLE_SEED = 20240928  # fixes the sampled rows of an output larger than the budget


def kernel_source_hash() -> str:
    """Identifies the kernels a traffic measurement belongs to: any change of the HIP sources invalidates it."""
    h = hashlib.sha256()
    csrc = os.path.join(ROOT, "benchmark_spmv_using_csr5_amd", "csrc")
    for name in sorted(os.listdir(csrc)):
        if name.endswith((".hip", ".h")):
            h.update(open(os.path.join(csrc, name), "rb").read())
    return h.hexdigest()[:16]


def profiled_traffic(key: str):
    """HBM-side bytes per step from this round's rocprofv3 PMC passes (profiles/rNN_traffic.json, written by
    scripts/collect_profiles.py from FETCH_SIZE / WRITE_SIZE runs of this same command).  Counters cannot be
    collected inside this process; the entry is used only if it was measured on EXACTLY these kernel sources
    (source hash) and this workload / dtype / sigma / mode / slab setting -- otherwise traffic is null."""
    import glob
    want = kernel_source_hash()
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_traffic.json")), reverse=True):
        try:
            entry = json.load(open(path)).get(key)
        except Exception:
            entry = None
        if entry and entry.get("traffic_bytes_per_launch") and entry.get("kernel_source_hash") == want:
            return int(entry["traffic_bytes_per_launch"]), os.path.basename(path)
    return None, None


def add_traffic(roof: dict, key: str, protocol_note=None):
    """roofline.traffic from the committed PMC profile of exactly these kernel sources, and what it is."""
    roof["traffic"], src = profiled_traffic(key)
    roof["traffic_source"] = src
    if src:
        roof["traffic_note"] = ("looked up, not measured by this process: HBM-side bytes per step (2 x FETCH_SIZE + WRITE_SIZE) from "
                                f"separate rocprofv3 --pmc passes of this command, profiles/{src}, valid for these exact kernel "
                                "sources (source hash match)" + (f"; measured under the {protocol_note}" if protocol_note else ""))
    else:
        roof["traffic_note"] = ("null: no committed PMC profile matches these kernel sources (profiles/r*_traffic.json is keyed "
                                "by a hash of csrc/*.hip and *.h; counters cannot be collected inside this process)")


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None, help="default: 100 for R-MAT >= 22, else 1000 (reference NUM_RUN)")
    ap.add_argument("--warmup", type=int, default=None, help="default: 10 / 50")
    ap.add_argument("--workload", default="rmat24")
    ap.add_argument("--mtx", default=None,
                    help="benchmark a Matrix Market file instead of a synthetic stand-in (single GPU): parsed and turned "
                         "into CSR by the native ingest, values replaced by rand()%%10 integers as the reference CLI does")
    ap.add_argument("--dtype", default=None, choices=[None, "f64", "f32"])
    ap.add_argument("--sigma", default="-1", help="-1 = auto rule (default), N = fixed, 'tuned' = measured autotune")
    ap.add_argument("--mode", default="fused", choices=["fused", "two-pass"])
    ap.add_argument("--launch", default="graph", choices=["graph", "eager"])
    ap.add_argument("--x-window", default="auto", choices=["auto", "off", "force"])
    ap.add_argument("--xcd-remap", type=int, default=1, choices=[0, 1])
    ap.add_argument("--lds-y", default="auto", choices=["auto", "off", "force"])
    ap.add_argument("--stream-nt", default="auto", choices=["auto", "off", "force"])
    ap.add_argument("--slabs", default="auto", help="column slabs: auto (default), 0 = off, 2..64 = that many")
    ap.add_argument("--slab-shift", type=int, default=None)
    ap.add_argument("--slab-hot", default="auto", choices=["auto", "off", "force"], help="LDS hot table of the slab kernel")
    ap.add_argument("--x-snapshot", type=int, default=None, choices=[0, 1],
                    help="hot-table slab kernel: 0 (default = the LIBRARY default) = its permuted copy of x is re-taken by every "
                         "spmv (x is read live, as the reference reads it); 1 = once per setX, which the reference CLI's protocol "
                         "allows (setX once, NUM_RUN spmv calls on the same x: CSR5_cuda/main.cu:63-99) -- reported as the side "
                         "figure roofline.x_snapshot_once_per_setX.  N > 1 defaults to 1: every rank's x is the replica the ONE "
                         "broadcast filled, which nothing writes afterwards -- the multi-GPU contract of csr5hip_multi_set_x")
    ap.add_argument("--defer-carries", default="auto", choices=["auto", "off", "force"],
                    help="plain path: cut rows finished by a second small launch instead of arrival atomics (CSR5HIP_OPT_DEFER_CARRIES)")
    ap.add_argument("--flagged-columns", default="auto", choices=["auto", "off", "force"],
                    help="plain kernel at sigma 4..8: column words with the row-start flag in bit 31 (CSR5HIP_OPT_FLAGGED_COLUMNS)")
    ap.add_argument("--zero-empty", type=int, default=0, choices=[0, 1],
                    help="1 = rows without non-zeros are written as 0 (CSR5HIP_OPT_ZERO_EMPTY_ROWS; the coupled-iteration setting)")
    ap.add_argument("--scaling", default=None, choices=[None, "weak", "strong"],
                    help="N > 1: strong (default for R-MAT) = ONE global matrix cut into cost-balanced (nnz + 2 * rows) row blocks; "
                         "weak = one fixed-size row block per GPU")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--scale", type=float, default=1.0, help="size factor of the synthetic stand-in (experiments)")
    ap.add_argument("--band", type=float, default=None,
                    help="scircuit / webbase: share of near-diagonal entries of the stand-in (defaults 0.5 / 0.3)")
    ap.add_argument("--values", default="int", choices=["int", "real"],
                    help="int = rand()%%10 (reference CLI data, exact); real = uniform(-1, 1)")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything beyond the headline: CPU baseline, sub-configs, locality points, "
                         "cold protocol of cache-sized working sets, side figures, conversion time, N > 1 checks (off by default)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write y of the last step as DIR/*.npy (a fixed seeded sample beyond 60 MB)")
    ap.add_argument("--cold", action="store_true", help="time the headline workload with the cold-cache protocol too")
    ap.add_argument("--no-cold", action="store_true",
                    help="--full: skip the cold-cache protocol that a cache-sized working set gets by default (profiling runs: one protocol per trace)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-sub-configs", action="store_true", help="skip the per-config array (N = 1)")
    ap.add_argument("--no-locality-points", action="store_true", help="skip the four locality-bracket points of the sub-configs")
    ap.add_argument("--no-side-figures", action="store_true",
                    help="skip roofline.x_live / roofline.narrowed_values (profiling runs: only the headline protocol's kernels)")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--no-n1-leg", action="store_true",
                    help="N > 1: skip rank 0's whole-matrix leg (the N = 1 step under the same x protocol + CSR5_avx2 on the whole matrix)")
    return ap.parse_args()


# ----------------------------------------------------------------------------------------------------------
# workloads
# ----------------------------------------------------------------------------------------------------------
# SuiteSparse files the BASELINE configs name (none is obtainable offline): when $CSR5_MTX_DIR holds them they are used
# instead of the synthetic stand-ins, through the native Matrix Market ingest (values replaced by rand()%10 integers as
# the reference CLI does, CSR5_avx2/main.cpp:283-295)
SUB_CONFIGS = ("scircuit", "webbase", "nd24k", "nd24k_f64")  # the other single-GPU BASELINE configs (+ nd24k-like in fp64)
# The two power-law stand-ins at the OTHER end of the locality bracket (profiles/r06_locality.md): no SuiteSparse file exists
# offline, so the line carries where the real matrices would plausibly land next to the harsh stand-ins above.  tag -> (workload,
# share of entries within +-64 of the diagonal, how the far columns are drawn)
LOCALITY_POINTS = {"webbase_b06pl": ("webbase", 0.6, "powerlaw"), "webbase_b09pl": ("webbase", 0.9, "powerlaw"),
                   "scircuit_b08": ("scircuit", 0.8, "uniform"), "scircuit_b095": ("scircuit", 0.95, "uniform")}
REAL_FILES = {"scircuit": "scircuit.mtx", "webbase": "webbase-1M.mtx", "nd24k": "nd24k.mtx"}


def real_file_for(workload: str):
    """Path of the real SuiteSparse file for a BASELINE workload if $CSR5_MTX_DIR provides it, else None."""
    d = os.environ.get("CSR5_MTX_DIR")
    name = REAL_FILES.get(workload)
    if not d or not name:
        return None
    path = os.path.join(d, name)
    return path if os.path.isfile(path) else None


def load_real(path: str, np_dtype):
    """(matrix on the host, label, ingest phase times) of a Matrix Market file through the native ingest."""
    from benchmark_spmv_using_csr5_amd import ingest
    loaded = ingest.load_mtx(path, dtype=np_dtype)
    ingest_ms = {"parse": round(loaded.parse_ms, 3), "h2d": round(loaded.h2d_ms, 3), "coo_to_csr": round(loaded.build_ms, 3)}
    mat = loaded.to_host(name=os.path.basename(path))
    loaded.release()
    return mat, f"{mat.name} (Matrix Market file, native ingest)", ingest_ms


def make_shard(workload: str, rank: int, world: int, seed: int, dtype, device, scale: float, strong: bool, band, far=None):
    """The rank's row block.  Returns (matrix with numpy or device arrays, label)."""
    from benchmark_spmv_using_csr5_amd import matrices as M

    if workload.startswith("rmat"):
        sc = int(workload[4:] or 24)
        if strong or world == 1:
            return M.rmat_device_shard(sc, 16, seed, rank, world, device), f"R-MAT scale {sc} EF16 (synthetic)"
        return M.rmat_device(sc, 16, seed, rank, world, device), f"R-MAT scale {sc} EF16 (synthetic, one block per GPU)"
    gen = {"scircuit": M.scircuit_like, "webbase": M.webbase_like, "nd24k": M.nd24k_like}[workload]
    kw = {} if scale == 1.0 else {"scale": scale}
    if workload in ("webbase", "scircuit") and band is not None:
        kw["band"] = band
    if workload in ("webbase", "scircuit") and far is not None:
        kw["far"] = far
    if strong and world > 1:  # one global matrix, cost-balanced row blocks (sharding.py)
        from benchmark_spmv_using_csr5_amd import sharding as S
        full = gen(seed=seed, dtype=dtype, **kw)
        blk = S.extract_row_block(full.row_ptr, full.col, full.val, full.n,
                                  S.partition_rows_by_cost(full.row_ptr, world), rank)
        return M.CsrMatrix(blk.m, blk.n, blk.row_ptr, blk.col, blk.val, full.name), full.name
    mat = gen(seed=seed + 101 * rank, dtype=dtype, **kw)
    if world > 1:  # weak: spread the block's columns over the global column space of all blocks
        rng = np.random.default_rng(seed + 7 * rank)
        shift = rng.integers(0, world, size=mat.nnz, dtype=np.int64) * mat.n
        keep_local = rng.random(mat.nnz) < 0.5
        col = np.where(keep_local, mat.col.astype(np.int64) + rank * mat.n, mat.col.astype(np.int64) + shift)
        mat.col = col.astype(np.int32)
        mat.n = mat.n * world
    return mat, mat.name


def _ck(rc, what):
    if rc != 0:
        from benchmark_spmv_using_csr5_amd import _capi
        raise RuntimeError(f"{what} -> {rc}: {_capi.last_error()}")


class Problem:
    """One matrix shard resident in HBM with its handle converted to CSR5."""

    def __init__(self, mat, label, dtype_name, args, dev, value_seed, x_dev=None):
        import torch
        from benchmark_spmv_using_csr5_amd import handle as H
        from benchmark_spmv_using_csr5_amd import matrices as M

        self.label, self.dtype_name = label, dtype_name
        self.t_dtype = torch.float64 if dtype_name == "f64" else torch.float32
        self.vsize = 8 if dtype_name == "f64" else 4
        self.m, self.n, self.nnz = mat.m, mat.n, mat.nnz
        g = torch.Generator(device=dev).manual_seed(value_seed)
        if isinstance(mat.row_ptr, np.ndarray):
            self.rp = torch.from_numpy(mat.row_ptr).to(dev)
            self.ci = torch.from_numpy(mat.col).to(dev)
        else:  # generated on the device: the handle permutes column_index in place, keep the caller's copy intact
            self.rp, self.ci = mat.row_ptr, mat.col.clone()
        if args.values == "int":
            self.va = torch.randint(0, 10, (self.nnz,), generator=g, device=dev).to(self.t_dtype)
            self.xd = torch.randint(0, 10, (self.n,), generator=g, device=dev).to(self.t_dtype) if x_dev is None else x_dev
        else:
            self.va = torch.rand(self.nnz, generator=g, device=dev, dtype=self.t_dtype) * 2 - 1
            self.xd = (torch.rand(self.n, generator=g, device=dev, dtype=self.t_dtype) * 2 - 1) if x_dev is None else x_dev
        self.yd = torch.zeros(self.m, dtype=self.t_dtype, device=dev)
        self.b_alg = M.algorithmic_bytes(self.m, self.n, self.nnz, self.vsize)
        A = H.anonymouslibHandle(self.m, self.n, dtype="float64" if dtype_name == "f64" else "float32")
        self.A = A
        _ck(A.inputCSR(self.nnz, self.rp, self.ci, self.va), "inputCSR")
        _ck(A.setX(self.xd), "setX")
        tuned = args.sigma == "tuned"
        _ck(A.setSigma(-1 if tuned else int(args.sigma)), "setSigma")
        _ck(A.setSpmvMode(H.SPMV_FUSED if args.mode == "fused" else H.SPMV_TWO_PASS), "setSpmvMode")
        _ck(A.setXWindow({"off": 0, "auto": 1, "force": 2}[args.x_window]), "setXWindow")
        _ck(A.setOption(2, args.xcd_remap), "xcd remap")
        _ck(A.setLdsY({"off": 0, "auto": 1, "force": 2}[args.lds_y]), "setLdsY")
        _ck(A.setStreamNT({"off": 0, "auto": 1, "force": 2}[args.stream_nt]), "setStreamNT")
        _ck(A.setColumnSlabs(1 if args.slabs == "auto" else int(args.slabs)), "setColumnSlabs")
        if args.slab_shift is not None:
            _ck(A.setSlabShift(args.slab_shift), "setSlabShift")
        _ck(A.setSlabHot({"off": 0, "auto": 1, "force": 2}[args.slab_hot]), "setSlabHot")
        if getattr(args, "defer_carries", "auto") != "auto":  # (auto = the library's default)
            _ck(A.setDeferCarries({"off": 0, "force": 2}[args.defer_carries]), "setDeferCarries")
        if getattr(args, "flagged_columns", "auto") != "auto":
            _ck(A.setFlaggedColumns({"off": 0, "force": 2}[args.flagged_columns]), "setFlaggedColumns")
        rc = A.setXSnapshot(int(getattr(args, "x_snapshot", 0) or 0))
        if rc != 0 and not os.environ.get("CSR5HIP_LIB"):  # (an older library build under A/B test does not know the option)
            _ck(rc, "setXSnapshot")
        if getattr(args, "zero_empty", 0):
            _ck(A.setZeroEmptyRows(1), "setZeroEmptyRows")
        A.warmup()
        torch.cuda.synchronize()
        if tuned:  # setup, outside every timed region (like asCSR5)
            err, _, _ = A.autotuneSigma(self.yd)
            _ck(err, "autotuneSigma")
            _ck(A.asCSR(), "asCSR")
        t0 = time.perf_counter()
        _ck(A.asCSR5(), "asCSR5")
        torch.cuda.synchronize()
        self.convert_first_ms = (time.perf_counter() - t0) * 1e3  # includes allocations and first-use code loading
        # steady-state conversion time: the reference CLI also converts back and forth before it times asCSR5
        # (CSR5_avx2/main.cpp:41-52: five asCSR5/asCSR rounds, then the timed one)
        # -- median of a few rounds, one sample is at the mercy of the host (--full only: not part of the SpMV headline)
        samples = []
        for _ in range((5 if self.nnz < 50_000_000 else 3) if getattr(args, "full", True) else 0):
            _ck(A.asCSR(), "asCSR")
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _ck(A.asCSR5(), "asCSR5")  # returns after its one stream synchronisation
            samples.append((time.perf_counter() - t0) * 1e3)
        self.convert_ms = sorted(samples)[len(samples) // 2] if samples else None
        self.info = A.info()
        if self.info.x_snapshot and hasattr(A, "snapshotX"):
            _ck(A.snapshotX(), "snapshotX")  # the permuted copy of x: once, here (behind the broadcast at N > 1), never inside a step
            torch.cuda.synchronize()

    def close(self):
        self.A.destroy()
        self.A.close()


def run_steps(prob, k, launch):
    if k <= 0:
        return
    if launch == "graph":
        chunk = min(k, 500)
        for _ in range(k // chunk):
            _ck(prob.A.spmv_repeat(1.0, prob.yd, chunk), "spmv_repeat")
        if k % chunk:
            _ck(prob.A.spmv_repeat(1.0, prob.yd, k % chunk), "spmv_repeat")
    else:
        for _ in range(k):
            prob.A.spmv(1.0, prob.yd)


def timed(prob, steps, warmup, launch, dist=None):
    """W untimed steps, then EXACTLY K steps bracketed by barrier + synchronize.  Returns (wall_s, event_ms)."""
    import torch
    run_steps(prob, warmup, launch)
    if launch == "graph":  # instantiate the graphs of the timed region outside it (one launch per distinct chunk length)
        chunk = min(steps, 500)
        run_steps(prob, chunk, launch)
        if steps > chunk and steps % chunk:
            run_steps(prob, steps % chunk, launch)
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    prob.A.timer_start()
    t0 = time.perf_counter()
    run_steps(prob, steps, launch)
    ev_ms = prob.A.timer_stop()
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    return time.perf_counter() - t0, ev_ms


def dump_outputs(out_dir, y, suffix="", budget=DUMP_BUDGET_BYTES) -> list:
    """--dump-outputs: y of the last timed step (what a caller of spmv() receives) as <out_dir>/y<suffix>.npy in its own
    dtype (fp64 / fp32).  A y larger than `budget` bytes is written as a fixed sample instead: the rows drawn without
    replacement by a generator seeded with DUMP_SAMPLE_SEED, ascending, with their indices as y<suffix>_rows.npy (fp64,
    exact below 2^53) -- the same rows in every run with the same arguments.  Returns the paths written."""
    import torch
    os.makedirs(out_dir, exist_ok=True)
    header = 128  # per .npy file (format 1.0, 1-D array)
    arrays = {}
    if y.numel() * y.element_size() + header <= budget:
        arrays["y"] = y.cpu().numpy()
    else:
        k = (budget - 2 * header) // (y.element_size() + 8)
        rows = np.sort(np.random.default_rng(DUMP_SAMPLE_SEED).choice(y.numel(), size=k, replace=False))
        arrays["y"] = y[torch.from_numpy(rows).to(y.device)].cpu().numpy()
        arrays["y_rows"] = rows.astype(np.float64)
    paths = []
    for name, a in arrays.items():
        paths.append(os.path.join(out_dir, name.replace("y", "y" + suffix, 1) + ".npy"))
        np.save(paths[-1], a)
    return paths


def timed_cold(make_copy, base, steps, warmup):
    """Cold-cache protocol: rotate the timed loop over k copies of the problem (matrix, x, y each) whose total
    footprint exceeds twice the Infinity Cache; one hipGraph, event-timed.  Returns (event ms per step, k, steps)."""
    import torch
    from benchmark_spmv_using_csr5_amd import handle as H
    k = max(3, min(64, int(2 * INFINITY_CACHE_BYTES // max(base.b_alg, 1)) + 2))  # (tiny matrices: capped, see cold_dict)
    copies = [base] + [make_copy() for _ in range(k - 1)]
    hs = [c.A for c in copies]
    ys = [c.yd for c in copies]
    steps = max(k, (steps + k - 1) // k * k)
    _ck(H.anonymouslibHandle.spmv_rotate(hs, ys, steps), "spmv_rotate")  # instantiates the graph; warm-up pass
    torch.cuda.synchronize()
    base.A.timer_start()
    _ck(H.anonymouslibHandle.spmv_rotate(hs, ys, steps), "spmv_rotate")
    ev_ms = base.A.timer_stop()
    torch.cuda.synchronize()
    for c in copies[1:]:
        c.close()
    return ev_ms / steps, k, steps


def roofline_dict(prob, ev_ms_per_step, wall_ms_per_step, extra=None):
    achieved = prob.b_alg / (ev_ms_per_step * 1e-3) / 1e9
    info = prob.info
    d = {
        "bound": "hbm",
        "achieved": round(achieved, 2),
        "peak": HBM_PEAK_GBS,
        "unit": "GB/s",
        "frac": round(achieved / HBM_PEAK_GBS, 4),
        "clock": "HIP events on the launch stream around the K timed steps (frac_wall: the same from the wall clock)",
        "frac_wall": round(prob.b_alg / (wall_ms_per_step * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
        "traffic": None,
        "kernel": ((("csr5::k_x_permute + " if info.slab_x_permuted and not info.x_snapshot else "") +
                    "csr5::k_spmv_range + csr5::k_range_finish") if info.slab_hot else "csr5::k_spmv") +
                  (" + csr5::k_calibrate (deferred carries)" if info.carries_deferred and not info.column_slabs else "") +
                  (" + csr5::k_slab_combine" if info.column_slabs else "") +
                  (" (all inside the step time)" if info.column_slabs or info.carries_deferred else ""),
        "algorithmic_bytes_per_launch": prob.b_alg,
        # diagnostic: what the kernels of one step actually move, by array (computed from the structure's sizes,
        # not measured; `traffic` below is the measured total).  B_alg stays the roofline's numerator.
        "stream_bytes_breakdown": stream_breakdown(prob),
        "launch_us": round(ev_ms_per_step * 1e3, 3),
        "cache": ("working set far beyond the 256-MiB Infinity Cache: every step streams from HBM"
                  if prob.b_alg > 2 * INFINITY_CACHE_BYTES else
                  "WARM: the working set stays in the 256-MiB Infinity Cache between back-to-back steps (this figure is "
                  "replaced by the COLD protocol's under --full unless --no-cold)"),
    }
    if extra:
        d.update(extra)
    return d


def stream_breakdown(prob) -> dict:
    """Bytes one SpMV step moves, array by array, for the path the handle runs.  Plain path: the CSR5 format arrays (B_alg with
    row_ptr replaced by tile_ptr + tile_desc).  Column slabs + hot table: what the slab CHILD streams -- 3-byte column codes,
    values, the child's tile_ptr, the LDS table images (once per XCD and slab from HBM; the 32 workgroups of an XCD re-read
    them from L2), the cold region of the permuted x (lower bound: every entry once; a 128-byte line may be fetched again), the
    per-(row, slab) partial sums P written by the range kernel and read by the combine, the combine's row bytes and base words,
    y, and -- x read live -- k_x_permute's read of x and write of the permuted copy."""
    i, v = prob.info, prob.vsize
    if not i.column_slabs:
        d = {("column_codes_16bit" if i.narrow_columns else "column_index"): (2 if i.narrow_columns else 4) * prob.nnz,
             "value": v * prob.nnz, "tile_ptr": 4 * (i.p + 1),
             "tile_desc": 0 if (i.narrow_columns or getattr(i, "flagged_columns", 0)) else 4 * i.p * 64 * i.num_packet,
             "x_once": v * prob.n, "y": v * prob.m}
        if getattr(i, "flagged_columns", 0):
            d["column_index_flag_in_bit31"] = d.pop("column_index")
    elif not i.slab_hot:
        d = {"child_column_index": 4 * prob.nnz, "child_value": v * prob.nnz, "child_tile_ptr": 4 * (i.slab_tiles + 1),
             "child_tile_desc": 4 * i.slab_tiles * 64, "x_once": v * prob.n, "P_written": v * i.slab_segments,
             "P_read": v * i.slab_segments, "combine_row_bytes": i.slab_segments, "y": v * prob.m}
    else:
        cap = 16384 if v == 8 else 32768
        vs = 4 if i.slab_values_narrowed else v
        d = {"child_column_codes": 3 * prob.nnz, "child_value": vs * prob.nnz, "child_tile_ptr": 4 * (i.slab_tiles + 1),
             "table_images_once_per_slab": v * cap * i.column_slabs, "cold_x_region_once": v * i.slab_cold_entries,
             "P_written": v * i.slab_segments, "P_read": v * i.slab_segments, "combine_row_bytes": i.slab_segments,
             "combine_base_words": 4 * (prob.m // 16 + 1) * 2, "y": v * prob.m}
        if not i.x_snapshot:
            d["x_permute_read_x"] = v * prob.n
            d["x_permute_write_copy"] = v * (cap * i.column_slabs + i.slab_cold_entries)
            d["x_permute_column_lists"] = 4 * (cap * i.column_slabs + i.slab_cold_entries)
    d["sum"] = int(sum(d.values()))
    d["note"] = "computed from array sizes; gathers count each distinct entry once (lines may be re-fetched): a lower bound of `traffic`"
    return d


def config_dict(prob, args, ingest_ms=None):
    info = prob.info
    return {
        "m_per_gpu": prob.m, "n": prob.n, "nnz_per_gpu": prob.nnz, "sigma": info.sigma, "tiles": info.p,
        "spmv_mode": args.mode, "launch": args.launch,
        "lds_x_window": bool(info.x_window_active), "x_window_cover_pct": info.x_window_cover_pct,
        "narrow_columns": bool(info.narrow_columns), "flagged_columns": bool(getattr(info, "flagged_columns", 0)),
        "carries_deferred": bool(info.carries_deferred),
        "column_slabs": info.column_slabs, "slab_shift": info.slab_shift, "slab_segments": info.slab_segments,
        "slab_sigma": info.slab_sigma, "slab_build_ms": round(info.t_slab_ms, 3),
        "slab_hot_table": bool(info.slab_hot), "slab_hot_cover_pct": info.slab_hot_cover_pct,
        "x_permuted_copy": bool(info.slab_x_permuted), "x_cold_entries": info.slab_cold_entries,
        "x_snapshot": ("once per setX (CSR5HIP_OPT_X_SNAPSHOT = 1; reference CLI protocol: setX once, then the timed spmv loop)"
                       if info.x_snapshot else "every spmv (library default)") if info.slab_x_permuted else None,
        "values": "rand()%10 integers (reference CLI data, exact in fp)" if args.values == "int" else "uniform(-1,1)",
        "ingest_ms": ingest_ms,
        "csr_to_csr5_ms": None if prob.convert_ms is None else round(prob.convert_ms, 3),
        "csr_to_csr5_first_call_ms": round(prob.convert_first_ms, 3),
    }


def cold_dict(prob, cold_ms, k, steps):
    return {"achieved": round(prob.b_alg / (cold_ms * 1e-3) / 1e9, 2),
            "frac": round(prob.b_alg / (cold_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
            "launch_us": round(cold_ms * 1e3, 3), "copies": k, "steps": steps,
            "protocol": f"timed loop rotates over {k} copies (matrix, x, y each; {k * prob.b_alg / 1e6:.0f} MB in all): " +
                        ("nothing is left in the Infinity Cache from the previous use" if k * prob.b_alg >= 2 * INFINITY_CACHE_BYTES
                         else "NOT cold -- the matrix is so small that 64 copies still fit the Infinity Cache")}


def small_working_set(prob) -> bool:
    """The matrix, x and y stay in the 256-MiB Infinity Cache between back-to-back steps."""
    return prob.b_alg <= 2 * INFINITY_CACHE_BYTES


def cold_is_the_number(prob, roof, ev_step, wall_step, cold_ms, k, cold_steps):
    """For a working set that fits the Infinity Cache the COLD protocol's figure is the roofline figure (achieved / frac /
    launch_us); the cache-warm one -- back-to-back steps, as the reference CLI times them -- moves to `warm`, so that no
    cache-resident number can be read as an HBM fraction."""
    warm = {k2: roof[k2] for k2 in ("achieved", "frac", "launch_us", "frac_wall")}
    warm["protocol"] = "back-to-back SpMVs on one matrix (reference CLI protocol): the working set stays in the Infinity Cache"
    cd = cold_dict(prob, cold_ms, k, cold_steps)
    roof.update({"achieved": cd["achieved"], "frac": cd["frac"], "launch_us": cd["launch_us"], "protocol": "cold: " + cd["protocol"],
                 "copies": cd["copies"], "cold_steps": cd["steps"], "warm": warm,
                 "cache": "COLD protocol (working set < 2 x the 256-MiB Infinity Cache): every step streams from HBM; the "
                          "cache-warm figure is under `warm`"})
    roof.pop("frac_wall", None)
    return roof


def sub_config(name, args, dev, band=None, far=None):
    """One of the other BASELINE GPU configs on this GPU (N = 1 only): the COLD figure is the headline of the entry, the
    cache-warm one sits under roofline.warm.  band / far: the stand-in at another point of the locality axis."""
    import copy
    a = copy.copy(args)
    a.sigma, a.slabs, a.slab_shift, a.values, a.slab_hot = "-1", "auto", None, "int", "auto"
    dtype_name = "f32" if name == "nd24k" else "f64"
    if name == "nd24k_f64":  # the fp64 sibling of BASELINE config 5 (same stand-in, 8-byte values)
        name = "nd24k"
    np_dtype = np.float32 if dtype_name == "f32" else np.float64
    real = real_file_for(name)
    ingest_ms = None
    if real:
        mat, label, ingest_ms = load_real(real, np_dtype)
    else:
        mat, label = make_shard(name, 0, 1, args.seed, np_dtype, dev, 1.0, False, band, far)
    prob = Problem(mat, label, dtype_name, a, dev, args.seed + 13)
    steps = {"scircuit": 1000, "webbase": 400, "nd24k": 200}[name]
    wall_s, ev_ms = timed(prob, steps, 50, "graph")
    ev_step, wall_step = ev_ms / steps, wall_s * 1e3 / steps
    roof = roofline_dict(prob, ev_step, wall_step)
    out = {
        "workload": f"{label}: CSR->CSR5 (omega=64, sigma={prob.info.sigma}) + CSR5 SpMV, single GPU",
        "data": f"suitesparse file {os.path.basename(real)}" if real else "synthetic stand-in",
        "dtype": dtype_name,
        "unit": "GFLOPS",
        "steps": steps,
        "config": config_dict(prob, a, ingest_ms),
    }
    if small_working_set(prob):
        cold_ms, k, cold_steps = timed_cold(lambda: Problem(mat, label, dtype_name, a, dev, args.seed + 13), prob, steps, 20)
        roof = cold_is_the_number(prob, roof, ev_step, wall_step, cold_ms, k, cold_steps)
        out.update({"value": round(2.0 * prob.nnz / (cold_ms * 1e-3) / 1e9, 3), "ms_per_step": round(cold_ms, 6),
                    "protocol": "cold (see roofline.protocol)",
                    "warm": {"value": round(2.0 * prob.nnz / (wall_step * 1e-3) / 1e9, 3), "ms_per_step": round(wall_step, 6),
                             "event_ms_per_step": round(ev_step, 6)}})
    else:
        out.update({"value": round(2.0 * prob.nnz / (wall_step * 1e-3) / 1e9, 3), "ms_per_step": round(wall_step, 6),
                    "event_ms_per_step": round(ev_step, 6)})
    out["roofline"] = roof
    i = prob.info
    key = f"{label}|{dtype_name}|sigma={i.sigma}|{a.mode}|slabs={i.column_slabs}/{i.slab_shift}/hot={i.slab_hot}"
    add_traffic(out["roofline"], key, "warm protocol" if small_working_set(prob) else None)
    prob.close()
    return out


# ----------------------------------------------------------------------------------------------------------
def self_launch(args):
    """`python bench.py --gpus N` without a launcher: start N ranks (one process per GPU) under torch.distributed.run in a
    child process and exit with its status (this process has asked the runtime for the device count: it is not replaced)."""
    import subprocess
    import torch
    ndev = torch.cuda.device_count()
    if ndev < args.gpus and os.environ.get("CSR5_BENCH_SHARE_GPU") != "1":
        raise SystemExit(f"bench.py: --gpus {args.gpus} but only {ndev} GPU(s) are visible; refusing to report n_gpus = 1")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    sys.exit(subprocess.run(cmd, env=env).returncode)


def main():
    args = parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(args)
    import torch

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    assert torch.cuda.is_available(), "bench.py needs a GPU"
    # CSR5_BENCH_SHARE_GPU=1 (test hook for 1-GPU boxes): every rank uses cuda:0 and the collectives go
    # through gloo, so the multi-rank control flow can be exercised without N GPUs.  Never set by default.
    share_gpu = os.environ.get("CSR5_BENCH_SHARE_GPU") == "1"
    if share_gpu:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if share_gpu:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    # long host-side waits (rank 0's CPU baseline and whole-matrix leg) go through a gloo group: an RCCL barrier would keep the
    # other GPUs spinning on rank 0's memory while rank 0 times its own GPU
    host_group = dist.new_group(backend="gloo") if (dist is not None and not share_gpu) else None

    is_rmat = args.workload.startswith("rmat")
    big = is_rmat and int(args.workload[4:] or 24) >= 22
    steps = args.steps if args.steps is not None else (100 if big else 1000)
    warmup = args.warmup if args.warmup is not None else (10 if big else 50)
    scaling = args.scaling or ("strong" if is_rmat else "weak")
    dtype_name = args.dtype or ("f32" if args.workload == "nd24k" else "f64")
    np_dtype = np.float64 if dtype_name == "f64" else np.float32
    if args.x_snapshot is None:
        args.x_snapshot = 1 if world > 1 else 0

    ingest_ms = None
    data = "synthetic"
    real = args.mtx or (real_file_for(args.workload) if world == 1 and args.scale == 1.0 and args.band is None else None)
    if real:
        if world > 1:
            raise SystemExit("--mtx is a single-GPU option")
        mat, label, ingest_ms = load_real(real, np_dtype)
        data = f"matrix market file {os.path.basename(real)}" + ("" if args.mtx else " (suitesparse, from $CSR5_MTX_DIR)")
    else:
        mat, label = make_shard(args.workload, rank, world, args.seed, np_dtype, dev, args.scale,
                                scaling == "strong", args.band)
    if args.scale != 1.0:
        label += f" x{args.scale:g}"

    # x: generated on rank 0 and replicated by the ONE collective of the sharded SpMV (RCCL broadcast over xGMI)
    x_dev = None
    x_broadcast_ms = None
    if world > 1:
        t_dtype = torch.float64 if dtype_name == "f64" else torch.float32
        g = torch.Generator(device=dev).manual_seed(args.seed + 13)
        x_dev = (torch.randint(0, 10, (mat.n,), generator=g, device=dev).to(t_dtype) if args.values == "int"
                 else torch.rand(mat.n, generator=g, device=dev, dtype=t_dtype) * 2 - 1)
        torch.cuda.synchronize()
        dist.barrier()
        t_b = time.perf_counter()
        if share_gpu:
            xc = x_dev.cpu()
            dist.broadcast(xc, src=0)
            x_dev = xc.to(dev)
        else:
            dist.broadcast(x_dev, src=0)  # the ONE collective of the sharded SpMV
        torch.cuda.synchronize()
        x_broadcast_ms = (time.perf_counter() - t_b) * 1e3
    prob = Problem(mat, label, dtype_name, args, dev, args.seed + 13 + rank, x_dev=x_dev)

    # --full: correctness run (kept for the cpu_baseline comparison), then the timed region
    full = args.full
    y_first = None
    if full:
        _ck(prob.A.spmv(1.0, prob.yd), "spmv")
        torch.cuda.synchronize()
        y_first = prob.yd.cpu().numpy() if (rank == 0 or world > 1) else None
    wall_s, ev_ms = timed(prob, steps, warmup, args.launch, dist)
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, prob.yd, "" if world == 1 else f"_rank{rank}", DUMP_BUDGET_BYTES // world)

    # N > 1: EVERY rank checks its own row block against the reference's compiled CSR5_avx2 (oracle/_ref; our C port of it
    # where that binary is absent) on the same block and the same x -- exact on the CLI's integer data -- all ranks at once,
    # each on its share of the host cores; the worst error of any rank goes into the line (all_reduce MAX)
    host = None
    check = None
    if world > 1 and full and not args.no_cpu_baseline:
        host = host_copy(prob)
        threads = max(1, min(32, (os.cpu_count() or 8) // world))
        try:
            err, kind = block_error_vs_cpu(host, y_first, threads)
        except Exception as e:  # (a rank without the checker must not hang the others in the collective below)
            print(f"bench.py: rank {rank}: CPU check failed: {e!r}", file=sys.stderr, flush=True)
            err, kind = float("inf"), "error"
        ck_t = torch.tensor([err, {"reference": 0.0, "port": 1.0}.get(kind, 2.0)], dtype=torch.float64,
                            device="cpu" if share_gpu else dev)
        ck_rows = [torch.zeros_like(ck_t) for _ in range(world)]
        dist.all_gather(ck_rows, ck_t)
        dist.all_reduce(ck_t, op=dist.ReduceOp.MAX)
        check = {"max_rel_err_gpu_vs_cpu": float(ck_t[0]),
                 "checker": {0.0: "reference", 1.0: "port"}.get(float(ck_t[1]), "error"),
                 "per_rank_max_rel_err": [float(r[0]) for r in ck_rows], "threads_per_rank": threads,
                 "note": "every rank's y (first SpMV) against CSR5_avx2 on that rank's own row block and the same x; "
                         "integer data: exact (0.0) expected; all ranks checked at once, then all_reduce(MAX)"}
        dist.barrier(group=host_group)  # rank 0 times its CPU baseline only after every rank's check has left the host cores

    stats = torch.tensor([wall_s, ev_ms, float(prob.nnz), float(prob.b_alg)], dtype=torch.float64,
                         device="cpu" if share_gpu else dev)
    per_rank = None
    if dist is not None:
        mx = stats.clone()
        dist.all_reduce(mx, op=dist.ReduceOp.MAX)
        sm = stats.clone()
        dist.all_reduce(sm, op=dist.ReduceOp.SUM)
        # every rank's own figures, so that a scaling record can be checked rank by rank: the collective really saw
        # `world` ranks (one row each), which rank set the pace, and what every GPU's roofline fraction was
        mine = torch.tensor([float(rank), float(local_rank), float(prob.m), float(prob.nnz), float(prob.nnz + 2 * prob.m),
                             float(prob.b_alg), wall_s * 1e3 / steps, ev_ms / steps, float(x_broadcast_ms or 0.0),
                             float(prob.info.column_slabs), float(prob.info.slab_hot)],
                            dtype=torch.float64, device=stats.device)
        rows = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(rows, mine)
        per_rank = [[float(v) for v in r.cpu()] for r in rows]
        wall_s, ev_ms = float(mx[0]), float(mx[1])
        total_nnz, max_b_alg = float(sm[2]), float(mx[3])
    else:
        total_nnz, max_b_alg = float(prob.nnz), float(prob.b_alg)

    if rank == 0:
        ms_per_step = wall_s * 1e3 / steps
        ev_per_step = ev_ms / steps
        gflops = 2.0 * total_nnz * steps / wall_s / 1e9
        info = prob.info
        roof = roofline_dict(prob, ev_per_step, ms_per_step)
        if world == 1:
            key = (f"{label}|{dtype_name}|sigma={info.sigma}|{args.mode}|slabs={info.column_slabs}/{info.slab_shift}"
                   f"/hot={info.slab_hot}")
            add_traffic(roof, key)
        else:
            roof["per_gpu_note"] = ("achieved/frac: rank 0's shard bytes (incl. the whole x it reads) over the "
                                    "max-over-ranks event time; largest shard = %d bytes; every rank's own figures: multi_gpu.ranks"
                                    % int(max_b_alg))
        if world == 1 and (args.cold or (full and small_working_set(prob) and not args.no_cold)):
            cold_ms, k, cs = timed_cold(lambda: Problem(mat, label, dtype_name, args, dev, args.seed + 13), prob,
                                        steps, warmup)
            if small_working_set(prob):
                roof = cold_is_the_number(prob, roof, ev_per_step, ms_per_step, cold_ms, k, cs)
            else:
                roof["cold"] = cold_dict(prob, cold_ms, k, cs)
        if world == 1 and info.slab_x_permuted and not info.x_snapshot and full and not args.no_side_figures:
            # side figure: the same workload under the reference CLI's protocol -- setX once, then the timed loop -- with the
            # permuted copy of x taken once per setX (CSR5HIP_OPT_X_SNAPSHOT = 1, what ./spmv opts into)
            _ck(prob.A.setXSnapshot(1), "setXSnapshot")
            lsteps = max(5, steps // 4)
            lwall, lev = timed(prob, lsteps, 2, args.launch, None)
            _ck(prob.A.setXSnapshot(0), "setXSnapshot")
            roof["x_snapshot_once_per_setX"] = {
                "launch_us": round(lev / lsteps * 1e3, 3),
                "frac": round(prob.b_alg / (lev / lsteps * 1e-3) / 1e9 / HBM_PEAK_GBS, 4), "steps": lsteps,
                "note": "opt-in CSR5HIP_OPT_X_SNAPSHOT = 1: csr5::k_x_permute runs once per setX instead of inside every step "
                        "(the caller promises not to change x's contents without calling setX again).  NOT the headline: the "
                        "headline runs at the library's defaults (x read live, as rounds 1-3 and the reference's spmv do); "
                        "round 4's headline was this figure"}
        elif world == 1 and info.slab_x_permuted and info.x_snapshot:
            roof["x_protocol"] = ("NON-DEFAULT: CSR5HIP_OPT_X_SNAPSHOT = 1 (--x-snapshot 1): the permuted copy of x is taken once "
                                  "per setX, outside the timed steps")
        if (world == 1 and info.slab_hot and dtype_name == "f64" and not info.slab_values_narrowed and hasattr(prob.A, "setNarrowValues")
                and full and not args.no_side_figures):
            # the same workload with CSR5HIP_OPT_NARROW_VALUES: the reference CLI's rand() % 10 values are exact in fp32, so
            # the slab kernel may stream them as fp32 (same result bit for bit).  NOT the headline: the roofline's algorithmic
            # bytes count the 8-byte value stream.
            try:
                _ck(prob.A.setNarrowValues(1), "setNarrowValues")
                if prob.A.info().slab_values_narrowed:
                    nsteps = max(5, steps // 4)
                    y_before = prob.yd.clone()
                    nwall, nev = timed(prob, nsteps, 2, args.launch, None)
                    same = bool(torch.equal(y_before, prob.yd))
                    nus = nev / nsteps * 1e3
                    roof["narrowed_values"] = {
                        "launch_us": round(nus, 3), "gflops": round(2.0 * prob.nnz / (nus * 1e-6) / 1e9, 1),
                        "stream_bytes_per_launch": prob.b_alg - 4 * prob.nnz, "y_bit_identical_to_headline_run": same, "steps": nsteps,
                        "frac_of_roof_on_the_bytes_it_streams": round((prob.b_alg - 4 * prob.nnz) / (nus * 1e-6) / 1e9 / HBM_PEAK_GBS, 4),
                        "note": "opt-in CSR5HIP_OPT_NARROW_VALUES = 1 (library default 0): every value of this matrix is exactly "
                                "representable in fp32, the hot child's value stream is kept as fp32 and widened in registers"}
                _ck(prob.A.setNarrowValues(0), "setNarrowValues")
            except Exception as exc:  # an older library under CSR5HIP_LIB
                roof["narrowed_values"] = {"error": str(exc)}
        part = ("whole matrix on one GPU" if world == 1 else
                f"{scaling} scaling, {'row blocks of ONE matrix balanced by nnz + 2 * rows' if scaling == 'strong' else 'one fixed-size row block per GPU'}, "
                "x replicated by one RCCL broadcast, no per-step collective")
        cfg = {"workload": f"{label}: CSR->CSR5 (omega=64, sigma={info.sigma}) + CSR5 SpMV, {part}",
               **config_dict(prob, args, ingest_ms)}
        if world > 1:
            cfg["x_protocol"] = ("x is generated on rank 0 and replicated by ONE broadcast before the loop; every rank's kernel-side "
                                 "(permuted) copy of it is taken once, right behind the broadcast (CSR5HIP_OPT_X_SNAPSHOT = 1, the "
                                 "contract of csr5hip_multi_set_x: a replica cannot change under the handle), not inside the steps"
                                 if info.x_snapshot else "x read live by every step (--x-snapshot 0)")
        out = {
            "metric": f"{'fp64' if dtype_name == 'f64' else 'fp32'} SpMV GFLOPS",
            "value": round(gflops, 3),
            "unit": "GFLOPS",
            "n_gpus": world,
            "steps": steps,
            "warmup": warmup,
            "ms_per_step": round(ms_per_step, 6),
            "event_ms_per_step": round(ev_per_step, 6),
            "value_from_event_clock": round(2.0 * total_nnz / (ev_per_step * 1e-3) / 1e9, 3),
            "higher_is_better": True,
            "scaling": scaling,
            "vs_baseline": None,
            "dtype": dtype_name,
            "data": data,
            "config": cfg,
            "roofline": roof,
        }
        if world == 1 and small_working_set(prob) and "warm" in roof:
            # value / ms_per_step stay what the contract defines (K timed back-to-back steps, wall clock); for a cache-sized
            # working set that is the WARM protocol -- the HBM figure is roofline.frac (cold)
            out["value_protocol"] = ("K back-to-back steps (cache-warm: the working set fits the 256-MiB Infinity Cache); "
                                     "roofline.achieved / frac / launch_us are the COLD protocol's")
        if per_rank is not None:
            out["multi_gpu"] = {
                "comm_backend": dist.get_backend(),
                "comm_world_size": dist.get_world_size(),
                "ranks_reporting": len(per_rank),
                "shared_device_test_hook": share_gpu,
                "x_bytes": int(prob.n) * prob.vsize,
                "x_broadcast_ms_max": round(max(r[8] for r in per_rank), 3),
                "collectives_per_step": 0,
                "ranks": [{"rank": int(r[0]), "device": int(r[1]), "rows": int(r[2]), "nnz": int(r[3]), "cost_nnz_plus_2_rows": int(r[4]),
                           "algorithmic_bytes": int(r[5]), "wall_ms_per_step": round(r[6], 6), "event_ms_per_step": round(r[7], 6),
                           "x_broadcast_ms": round(r[8], 3), "column_slabs": int(r[9]), "slab_hot": int(r[10]),
                           "roofline_frac": round(r[5] / (r[7] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if r[7] > 0 else None}
                          for r in per_rank],
            }
        if full:
            roof.update(conversion_roofline(prob, ev_per_step))
        if "x_snapshot_once_per_setX" in roof:
            roof["x_snapshot_frac"] = roof["x_snapshot_once_per_setX"]["frac"]
        if check is not None:
            out["multi_gpu"].update(check)
        if full and not args.no_cpu_baseline:
            try:
                if world == 1:
                    out["cpu_baseline"] = cpu_baseline(prob, y_first, args.cpu_seconds)
                else:  # the other ranks wait in the barrier below: the host cores are rank 0's
                    out["cpu_baseline"] = cpu_baseline(prob, y_first, args.cpu_seconds / 2, host=host,
                                                       what=f"rank 0's row block of {world} ({prob.nnz} of {int(total_nnz)} nnz)")
                    out["cpu_baseline"]["scope"] = "rank 0's row block; the whole matrix: cpu_baseline.whole_matrix"
            except Exception as e:  # the baseline leg must never cost the headline line
                out["cpu_baseline"] = {"error": repr(e)}
        if world == 1 and "x_snapshot_once_per_setX" in roof:
            # the N = 1 point of the curve under the protocol the N > 1 points run (x captured once per setX / broadcast)
            out["value_multi_gpu_protocol"] = round(2.0 * prob.nnz / (roof["x_snapshot_once_per_setX"]["launch_us"] * 1e-6) / 1e9, 3)
        prob.close()
        del prob
        host = None
        torch.cuda.empty_cache()
        if world > 1 and is_rmat and scaling == "strong" and full and not args.no_n1_leg:
            # rank 0 alone (the other ranks wait): the WHOLE matrix on this one GPU under the same protocol -> the speed-up of
            # this N-GPU line over N = 1 with no protocol difference booked as scaling; and CSR5_avx2 on the whole matrix
            try:
                out["multi_gpu"].update(whole_matrix_leg(args, dev, label, dtype_name, x_dev, steps, warmup, ev_per_step,
                                                         out.get("cpu_baseline")))
            except Exception as e:
                out["multi_gpu"]["n1_same_protocol"] = {"error": repr(e)}
        if world == 1 and full and not args.no_sub_configs and not real and args.workload == "rmat24":
            subs = []
            for name in SUB_CONFIGS:
                try:
                    subs.append(sub_config(name, args, dev))
                except Exception as e:  # a sub-config must never cost the headline line
                    subs.append({"workload": name, "error": repr(e)})
            out["configs"] = subs
            # the same figures, compact, where the driver's record keeps them (it drops top-level keys it does not know)
            summary = {}
            for name, sc in zip(SUB_CONFIGS, subs):
                r = sc.get("roofline") or {}
                w = r.get("warm") or {}
                summary[name] = ({"error": sc["error"]} if "error" in sc else
                                 {"dtype": sc["dtype"], "cold_frac": r.get("frac"), "cold_us": r.get("launch_us"),
                                  "warm_frac": w.get("frac"), "warm_us": w.get("launch_us"),
                                  "traffic_ratio": (round(r["traffic"] / r["algorithmic_bytes_per_launch"], 3) if r.get("traffic") else None),
                                  "kernel": r.get("kernel"), "sigma": sc["config"]["sigma"], "column_slabs": sc["config"]["column_slabs"],
                                  "data": sc.get("data")})
            out["roofline"]["configs"] = summary
            # ... and FLAT, as scalar keys of `roofline` (the driver's parsed record keeps scalars only)
            for name, e in summary.items():
                for src, dst in (("cold_frac", "cold_frac"), ("warm_frac", "warm_frac"), ("traffic_ratio", "traffic_ratio"),
                                 ("cold_us", "cold_us")):
                    if e.get(src) is not None:
                        out["roofline"][f"{name}_{dst}"] = e[src]
            # the locality bracket of the two power-law stand-ins: three scalar keys per point (cold / warm fraction, path taken)
            if not args.no_locality_points:
                for tag, (wl, band, far) in LOCALITY_POINTS.items():
                    try:
                        sc = sub_config(wl, args, dev, band=band, far=far)
                        r, c = sc["roofline"], sc["config"]
                        out["roofline"][f"{tag}_cold_frac"] = r.get("frac")
                        out["roofline"][f"{tag}_warm_frac"] = (r.get("warm") or {}).get("frac")
                        out["roofline"][f"{tag}_path"] = ("plain" if not c["column_slabs"] else f"slabs{c['column_slabs']}" +
                                                          ("+table" if c["slab_hot_table"] else "")) + ("+xwindow" if c["lds_x_window"] else "")
                    except Exception as e:  # never at the cost of the headline line
                        out["roofline"][f"{tag}_error"] = repr(e)
                out["roofline"]["locality_note"] = ("<workload>_b<band>[pl]: the stand-in with that share of entries near the diagonal "
                                                    "([pl]: far columns power-law instead of uniform); bracket and forced paths: "
                                                    "profiles/r06_locality.md")
        print(json.dumps(out), flush=True)
    else:
        prob.close()
    if dist is not None:
        dist.barrier(group=host_group)
        dist.destroy_process_group()


def conversion_roofline(prob, spmv_ms: float) -> dict:
    """The conversion is on the hot path (north_star): its own bytes over its own time, as flat scalar keys of `roofline`.
    B_conv = the in-place tile transpose reads and writes column_index and value once each (2 * (4 + sizeof vT) per non-zero,
    format_cuda.h:525-744) + row_ptr read once + the three descriptor arrays written once.  `conversion_ms` is the whole
    asCSR5() call -- host-timed median, kernel-side tables and (R-MAT) the column-slab structure included;
    `conversion_format_ms` is the three format phases alone, from the kernels' wall-clock stamps."""
    i = prob.info
    b_conv = 2 * (4 + prob.vsize) * prob.nnz + 4 * (prob.m + 1) + 4 * (i.p + 1) * 2 + 4 * i.p * 64 * max(i.num_packet, 1)
    fmt_ms = i.t_tile_ptr_ms + i.t_tile_desc_ms + i.t_transpose_ms
    d = {"conversion_ms": round(prob.convert_ms, 4), "conversion_in_spmvs": round(prob.convert_ms / spmv_ms, 2),
         "conversion_bytes": int(b_conv),
         "conversion_frac": round(b_conv / (prob.convert_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
    if fmt_ms > 0:
        d["conversion_format_ms"] = round(fmt_ms, 4)
        d["conversion_format_frac"] = round(b_conv / (fmt_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
    if i.column_slabs:
        d["conversion_slab_structure_ms"] = round(i.t_slab_ms, 4)
    return d


def host_copy(prob):
    """(m, n, nnz, row_ptr, col, val64, x64) on the host, in plain CSR order (the handle's in-place transpose undone)."""
    import torch
    _ck(prob.A.asCSR(), "asCSR")
    torch.cuda.synchronize()
    return (prob.m, prob.n, prob.nnz, prob.rp.cpu().numpy(), prob.ci.cpu().numpy(),
            prob.va.cpu().numpy().astype(np.float64), prob.xd.cpu().numpy().astype(np.float64))


def max_rel_err(y_gpu, y_cpu, row_ptr) -> float:
    nonempty = np.diff(row_ptr) > 0
    if not nonempty.any():
        return 0.0
    denom = np.maximum(np.abs(y_cpu[nonempty]), 1e-300)
    return float(np.max(np.abs(y_gpu[nonempty].astype(np.float64) - y_cpu[nonempty]) / denom))


def block_error_vs_cpu(host, y_gpu, threads: int):
    """One CSR5_avx2 SpMV (oracle/_ref; our C port where it is absent) on the rank's block -> (max relative error, checker)."""
    from oracle.csr5_oracle import Oracle, Reference
    m, n, nnz, row_ptr, col, val64, x64 = host
    if Reference.available():
        ref = Reference()
        ref.avx2_set_threads(max(1, min(threads, ref.avx2_threads())))
        y, _, _ = ref.avx2_spmv(m, n, row_ptr, col, val64, x64, y0=np.zeros(m))
        return max_rel_err(y_gpu, y, row_ptr), "reference"
    orc = Oracle()
    y = orc.spmv(orc.convert(4, 16, m, row_ptr, col, val64), row_ptr, x64)
    return max_rel_err(y_gpu, y, row_ptr), "port"


def whole_matrix_leg(args, dev, label, dtype_name, x_dev, steps, warmup, job_ms_per_step, block_baseline) -> dict:
    """N > 1, rank 0 only, the other ranks idle: the same global matrix WHOLE on this one GPU under the job's x protocol
    (its N = 1 step time -> speedup_vs_n1_same_protocol) and the reference's CSR5_avx2 on the whole matrix on the host."""
    import copy
    import torch
    from benchmark_spmv_using_csr5_amd import matrices as M
    a = copy.copy(args)
    sc = int(args.workload[4:] or 24)
    mat = M.rmat_device_shard(sc, 16, args.seed, 0, 1, dev)
    prob = Problem(mat, label, dtype_name, a, dev, args.seed + 13, x_dev=x_dev)
    _ck(prob.A.spmv(1.0, prob.yd), "spmv")
    torch.cuda.synchronize()
    y1 = prob.yd.cpu().numpy()
    k = max(5, min(steps, 50))
    wall_s, ev_ms = timed(prob, k, min(warmup, 5), args.launch, None)
    n1_ms = ev_ms / k
    out = {"n1_same_protocol": {"ms_per_step": round(n1_ms, 6), "steps": k, "gflops": round(2.0 * prob.nnz / (n1_ms * 1e-3) / 1e9, 3),
                                "roofline_frac": round(prob.b_alg / (n1_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                                "column_slabs": prob.info.column_slabs, "slab_hot": int(prob.info.slab_hot),
                                "x_snapshot": int(prob.info.x_snapshot),
                                "note": "the whole matrix on rank 0's GPU alone, same x, same x protocol, same options, timed in this run "
                                        "while the other ranks wait"},
           "speedup_vs_n1_same_protocol": round(n1_ms / job_ms_per_step, 3)}
    if not args.no_cpu_baseline:
        try:
            whole = cpu_baseline(prob, y1, args.cpu_seconds / 2, what=f"the WHOLE matrix ({prob.nnz} nnz)")
            if isinstance(block_baseline, dict) and "error" not in block_baseline:
                block_baseline["whole_matrix"] = whole
                block_baseline["whole_matrix_value"] = whole["value"]
            else:
                out["cpu_baseline_whole_matrix"] = whole
        except Exception as e:
            out["cpu_baseline_whole_matrix"] = {"error": repr(e)}
    prob.close()
    return out


def cpu_baseline(prob, y_gpu, budget_s: float, host=None, what=None) -> dict:
    """CSR5 at omega=4 / sigma=16, fp64, OpenMP on this node's host cores, same matrix and vectors (copied back
    from the device).  Prefers the reference's own CSR5_avx2 build (oracle/_ref); falls back to our C port of it."""
    from oracle.csr5_oracle import Oracle, Reference

    m, n, nnz, row_ptr, col, val64, x64 = host if host is not None else host_copy(prob)
    big = nnz > 50_000_000
    if Reference.available():
        ref = Reference()
        # The reference runs with the ambient OpenMP thread count; on a 2-socket host the full count is far from
        # its best for a small matrix, so give it the best of a few counts (short probe each), then time that one.
        full = ref.avx2_threads()
        # torch.distributed.run exports OMP_NUM_THREADS=1 to its ranks: at N > 1 the ambient count says nothing about the host.
        # Rank 0 times the baseline alone (the other ranks wait in a barrier), so the host's cores are its own: start from half
        # the hardware threads this process may run on, the ambient default of the N = 1 run on the same box.
        try:
            allowed = len(os.sched_getaffinity(0))
        except (AttributeError, OSError):
            allowed = os.cpu_count() or 1
        if os.environ.get("OMP_NUM_THREADS") == "1" and "WORLD_SIZE" in os.environ and allowed > 2:
            full = max(full, allowed // 2)
        tried = {}
        counts = sorted({full, max(full // 2, 1), max(full // 4, 1)} | (set() if big else {max(full // 8, 1), 16, 8}))
        for t in counts:
            if t > full or t < 1:
                continue
            ref.avx2_set_threads(t)
            _, ms_t, _ = ref.avx2_spmv(m, n, row_ptr, col, val64, x64, warm=1 if big else 5, runs=3 if big else 20)
            tried[t] = round(ms_t, 4)
        cores = min(tried, key=tried.get)
        ref.avx2_set_threads(cores)
        ms1 = tried[cores]
        runs = int(max(5 if big else 20, min(2000, budget_s * 1e3 / max(ms1, 1e-3))))
        y, ms, conv_ms = ref.avx2_spmv(m, n, row_ptr, col, val64, x64, warm=2 if big else 50, runs=runs)
        kind = "reference"
    else:
        print("bench.py: oracle/_ref (the reference's own CSR5_avx2 build) is not in this tree -- cpu_baseline.kind = \"port\": "
              "timing our C restatement of it instead (build it where /root/reference exists: make -C oracle ref)",
              file=sys.stderr, flush=True)
        orc = Oracle()
        cores = orc.num_threads()
        fmt = orc.convert(4, 16, m, row_ptr, col, val64)
        t0 = time.perf_counter()
        y = orc.spmv(fmt, row_ptr, x64)
        ms1 = (time.perf_counter() - t0) * 1e3
        runs = int(max(3, min(500, budget_s * 1e3 / max(ms1, 1e-3))))
        t0 = time.perf_counter()
        for _ in range(runs):
            y = orc.spmv(fmt, row_ptr, x64)
        ms = (time.perf_counter() - t0) * 1e3 / runs
        conv_ms = None
        tried = {cores: round(ms, 4)}
        kind = "port"
    max_rel = max_rel_err(y_gpu, y, row_ptr)
    return {
        "value": round(2.0 * nnz / (ms * 1e-3) / 1e9, 3),
        "unit": "GFLOPS",
        "cores": cores,
        "kind": kind,
        "sample": f"{what or f'same matrix ({nnz} nnz)'}, CSR5_avx2 omega=4 sigma=16 fp64 OpenMP, {runs} timed SpMV after warm-up",
        # short probes per thread count (ms per SpMV).  They can be several times faster than the long timed run:
        # the box's container throttles sustained multi-thread CPU use, short bursts escape it.  A reported
        # baseline, not a target: the GPU/CPU ratio says nothing about kernel quality, roofline.frac does.
        "threads_tried_ms": tried,
        "host_threads_available": os.cpu_count(),
        "ms_per_spmv": round(ms, 5),
        # which figure to quote: `value` -- the sustained rate of the long timed loop at `cores` threads;
        # `value_best_probe` is the same thread count's 3-call burst, an UPPER bound of what this host gives the reference
        "value_best_probe": round(2.0 * nnz / (min(tried.values()) * 1e-3) / 1e9, 3),
        "quote": "value (sustained, timed loop); value_best_probe = short burst at the same thread count, upper bound",
        "csr_to_csr5_ms": None if conv_ms is None else round(conv_ms, 3),
        "max_rel_err_gpu_vs_cpu": max_rel,
    }


if __name__ == "__main__":
    main()
