#!/usr/bin/env python3
"""One multi-head call (csr5hip_mha, csr5hip_mha_backward) against the `heads` single-head calls it replaces, on the same handle
and the same packed tensors, one JSON line per (workload, dtype, heads, k, d).

    python scripts/bench_mha.py [--workloads scircuit,webbase,nd24k[,hubs]] [--dtypes f64,f32] [--heads 4,8] [--kd 16x16,64x64]

Per line, forward: mha_us, the median of device-event-timed batches of A.mha(Q, K, V, O) after a warm-up, and per_head_us, the
same for `heads` A.attention calls on the column slices Q[:, h], K[:, h], V[:, h], O[:, h] of the same tensors, in the same
process, the batches of the two alternating; per_head_min_us / per_head_max_us are the baseline's fastest and slowest batch (its
spread is the margin of any claim).  Backward: the same for A.mhaBackward against `heads` A.attentionBackward calls, all three
gradients wanted, the transposed companion built before.  launches counts kernel launches per call.  Q is uniform(-1, 1) /
sqrt(k), K, V and dO uniform(-1, 1).  Before any timing the two routes are compared bit for bit: they are defined to be equal.
The workloads are those of bench_attention.py and, on request, hubs: 2 048 rows of 6 000 entries over 65 536 columns, every row on
the path that holds one chunk of a row at a time (rows beyond 2 048 entries), where each head walks the pattern again."""
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
from scripts.bench_attention import DEV, WORKLOADS  # noqa: E402
from scripts.bench_sddmm import batch_us  # noqa: E402

WORKLOADS = dict(WORKLOADS, hubs=lambda dt: M.csr_from_row_lengths(np.full(2048, 6000), 65536, np.random.default_rng(9),
                                                                   name="hubs(synthetic)", dtype=dt))


def timed(f, g, batches, per_batch, warmup):
    """per-batch times (us per call) of f and of g, their batches alternating"""
    for _ in range(warmup):
        f()
    for _ in range(min(warmup, 2)):
        g()
    torch.cuda.synchronize()
    tf, tg = [], []
    for _ in range(batches):
        tf.append(batch_us(f, per_batch))
        tg.append(batch_us(g, per_batch))
    return tf, tg


def same(a, b):
    return torch.equal(a.view(torch.int64 if a.dtype == torch.float64 else torch.int32),
                       b.view(torch.int64 if b.dtype == torch.float64 else torch.int32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="scircuit,webbase,nd24k")
    ap.add_argument("--dtypes", default="f64,f32")
    ap.add_argument("--heads", default="4,8")
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
            rp = torch.from_numpy(mat.row_ptr).to(DEV)
            ci = torch.from_numpy(mat.col).to(DEV)
            va = torch.ones(mat.nnz, dtype=tdt, device=DEV)
            A = H.anonymouslibHandle(mat.m, mat.n, dtype=np.dtype(dtype).name)
            rcs = [A.inputCSR(mat.nnz, rp, ci, va), A.setSigma(H.ANONYMOUSLIB_AUTO_TUNED_SIGMA), A.asCSR5(), A.buildTranspose()]
            if any(rcs):
                raise RuntimeError(f"handle setup failed: {rcs}")
            gen = torch.Generator(device=DEV).manual_seed(5)
            for heads in (int(h) for h in args.heads.split(",")):
                for k, d in kds:
                    def rand(rows, width):
                        return torch.rand((rows, heads, width), dtype=tdt, device=DEV, generator=gen) * 2 - 1
                    Q, K, V, dO = rand(mat.m, k) / k ** 0.5, rand(mat.n, k), rand(mat.n, d), rand(mat.m, d)
                    O, dQ, dK, dV = (torch.empty_like(t) for t in (dO, Q, K, V))
                    O1, dQ1, dK1, dV1 = (torch.empty_like(t) for t in (dO, Q, K, V))
                    work, work1 = torch.empty(4 * mat.m * heads, dtype=tdt, device=DEV), torch.empty(4 * mat.m, dtype=tdt, device=DEV)

                    def mha():
                        if A.mha(Q, K, V, O):
                            raise RuntimeError("mha failed")

                    def per_head():
                        for h in range(heads):
                            if A.attention(Q[:, h], K[:, h], V[:, h], O1[:, h]):
                                raise RuntimeError("attention failed")

                    def mha_bwd():
                        if A.mhaBackward(Q, K, V, dO, dQ, dK, dV, work):
                            raise RuntimeError("mhaBackward failed")

                    def per_head_bwd():
                        for h in range(heads):
                            if A.attentionBackward(Q[:, h], K[:, h], V[:, h], dO[:, h], dQ1[:, h], dK1[:, h], dV1[:, h], work1):
                                raise RuntimeError("attentionBackward failed")
                    for f in (mha, per_head, mha_bwd, per_head_bwd):
                        f()
                    torch.cuda.synchronize()
                    equal = all(same(a, b) for a, b in ((O, O1), (dQ, dQ1), (dK, dK1), (dV, dV1)))
                    tf, tg = timed(mha, per_head, args.batches, args.per_batch, args.warmup)
                    bf, bg = timed(mha_bwd, per_head_bwd, args.batches, args.per_batch, args.warmup)
                    r = lambda v: round(float(v), 2)  # noqa: E731
                    print(json.dumps({
                        "workload": mat.name, "dtype": dn, "heads": heads, "k": k, "d": d, "m": mat.m, "n": mat.n, "nnz": mat.nnz,
                        "same_bits": equal,
                        "mha_us": r(np.median(tf)), "per_head_us": r(np.median(tg)), "per_head_min_us": r(min(tg)),
                        "per_head_max_us": r(max(tg)), "launches": [1, heads],
                        "mha_backward_us": r(np.median(bf)), "per_head_backward_us": r(np.median(bg)),
                        "per_head_backward_min_us": r(min(bg)), "per_head_backward_max_us": r(max(bg)), "launches_backward": [2, 2 * heads],
                    }), flush=True)
                    if not equal:
                        raise SystemExit(f"mha differs from the per-head calls: {mat.name} {dn} heads={heads} k={k} d={d}")
                    del Q, K, V, dO, O, dQ, dK, dV, O1, dQ1, dK1, dV1, work, work1
                    torch.cuda.empty_cache()
            A.destroy()
            A.close()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
