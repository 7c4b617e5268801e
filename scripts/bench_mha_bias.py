#!/usr/bin/env python3
"""The biased multi-head calls (csr5hip_mha_biased, csr5hip_mha_biased_backward) against the plain ones (csr5hip_mha,
csr5hip_mha_backward) on the same handle and the same packed tensors, and on request against the unfused per-head chain they
replace; one JSON line per (workload, dtype, heads, k, d).

    python scripts/bench_mha_bias.py [--workloads scircuit,webbase,nd24k] [--dtypes f64,f32] [--heads 4,8] [--kd 16x16,64x64]
                                     [--unfused 4:16x16]

bench_mha.py's protocol: per pair of routes the batches alternate, a batch is timed by device events, the figure is the median
of 7 batches of 10 calls after a warm-up, and the baseline's fastest and slowest batch are printed with it: their spread is the
margin of any ratio.  Per line: biased_us against mha_us (forward, one launch each); biased_backward_us against mha_backward_us
(two launches each, all three gradients, the transposed companion built before); biased_backward_ds_us, the same call with the
(nnz, heads) score gradient dS wanted, against the same baseline.  Q is uniform(-1, 1) / sqrt(k), K, V and dO uniform(-1, 1), the
scale 1 and a slope per head.  BEFORE ANY TIMING THE BITS ARE COMPARED: the handle's values are +0, for which the biased calls
are defined to give mha's bits (the time of a call does not depend on the values).

--unfused HEADS:KxD adds, for that one point of every workload and dtype, the chain a biased attention needed before: per head
sddmm, a torch add of slope * bias, rowSoftmax, updateValues, spmm -- five calls per head, two nnz-long temporaries, the handle's
values overwritten (they are restored afterwards) -- as unfused_us, with its fastest and slowest batch; unfused_calls counts the
library and torch calls per forward (each at least one launch; updateValues also refreshes the transposed companion)."""
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
from scripts.bench_mha import same, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="scircuit,webbase,nd24k")
    ap.add_argument("--dtypes", default="f64,f32")
    ap.add_argument("--heads", default="4,8")
    ap.add_argument("--kd", default="16x16,64x64")
    ap.add_argument("--unfused", default="", help="HEADS:KxD, the one point at which the unfused chain is measured too")
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--per-batch", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    kds = [tuple(int(v) for v in kd.split("x")) for kd in args.kd.split(",")]
    unfused_at = None
    if args.unfused:
        hh, kd = args.unfused.split(":")
        unfused_at = (int(hh),) + tuple(int(v) for v in kd.split("x"))
    for wl in args.workloads.split(","):
        for dn in args.dtypes.split(","):
            dtype = np.float64 if dn == "f64" else np.float32
            mat = WORKLOADS[wl](dtype)
            tdt = torch.float64 if dtype == np.float64 else torch.float32
            rp = torch.from_numpy(mat.row_ptr).to(DEV)
            ci = torch.from_numpy(mat.col).to(DEV)
            va = torch.zeros(mat.nnz, dtype=tdt, device=DEV)
            zeros = torch.zeros(mat.nnz, dtype=tdt, device=DEV)
            A = H.anonymouslibHandle(mat.m, mat.n, dtype=np.dtype(dtype).name)
            rcs = [A.inputCSR(mat.nnz, rp, ci, va), A.setSigma(H.ANONYMOUSLIB_AUTO_TUNED_SIGMA), A.asCSR5(), A.buildTranspose()]
            if any(rcs):
                raise RuntimeError(f"handle setup failed: {rcs}")
            gen = torch.Generator(device=DEV).manual_seed(5)
            for heads in (int(h) for h in args.heads.split(",")):
                slopes = torch.linspace(0.5, 2.0, heads, dtype=tdt, device=DEV)
                for k, d in kds:
                    def rand(rows, width):
                        return torch.rand((rows, heads, width), dtype=tdt, device=DEV, generator=gen) * 2 - 1
                    Q, K, V, dO = rand(mat.m, k) / k ** 0.5, rand(mat.n, k), rand(mat.n, d), rand(mat.m, d)
                    O, dQ, dK, dV = (torch.empty_like(t) for t in (dO, Q, K, V))
                    O1, dQ1, dK1, dV1 = (torch.empty_like(t) for t in (dO, Q, K, V))
                    work = torch.empty(4 * mat.m * heads, dtype=tdt, device=DEV)
                    dS = torch.empty((mat.nnz, heads), dtype=tdt, device=DEV)

                    def mha():
                        if A.mha(Q, K, V, O1):
                            raise RuntimeError("mha failed")

                    def biased():
                        if A.mhaBiased(Q, K, V, O, scale=1.0, slopes=slopes):
                            raise RuntimeError("mhaBiased failed")

                    def mha_bwd():
                        if A.mhaBackward(Q, K, V, dO, dQ1, dK1, dV1, work):
                            raise RuntimeError("mhaBackward failed")

                    def biased_bwd():
                        if A.mhaBiasedBackward(Q, K, V, dO, dQ, dK, dV, work, scale=1.0, slopes=slopes):
                            raise RuntimeError("mhaBiasedBackward failed")

                    def biased_bwd_ds():
                        if A.mhaBiasedBackward(Q, K, V, dO, dQ, dK, dV, work, scale=1.0, slopes=slopes, dS=dS):
                            raise RuntimeError("mhaBiasedBackward with dS failed")
                    for f in (mha, biased, mha_bwd, biased_bwd):
                        f()
                    torch.cuda.synchronize()
                    equal = all(same(a, b) for a, b in ((O, O1), (dQ, dQ1), (dK, dK1), (dV, dV1)))
                    tb, tm = timed(biased, mha, args.batches, args.per_batch, args.warmup)
                    bb, bm = timed(biased_bwd, mha_bwd, args.batches, args.per_batch, args.warmup)
                    bd, bm2 = timed(biased_bwd_ds, mha_bwd, args.batches, args.per_batch, args.warmup)
                    r = lambda v: round(float(v), 2)  # noqa: E731
                    line = {
                        "workload": mat.name, "dtype": dn, "heads": heads, "k": k, "d": d, "m": mat.m, "n": mat.n, "nnz": mat.nnz,
                        "same_bits": equal,
                        "biased_us": r(np.median(tb)), "mha_us": r(np.median(tm)), "mha_min_us": r(min(tm)), "mha_max_us": r(max(tm)),
                        "ratio": round(float(np.median(tb) / np.median(tm)), 4), "launches": [1, 1],
                        "biased_backward_us": r(np.median(bb)), "mha_backward_us": r(np.median(bm)), "mha_backward_min_us": r(min(bm)),
                        "mha_backward_max_us": r(max(bm)), "ratio_backward": round(float(np.median(bb) / np.median(bm)), 4),
                        "biased_backward_ds_us": r(np.median(bd)), "mha_backward_again_us": r(np.median(bm2)),
                        "mha_backward_again_min_us": r(min(bm2)), "mha_backward_again_max_us": r(max(bm2)),
                        "ratio_backward_ds": round(float(np.median(bd) / np.median(bm2)), 4), "launches_backward": [2, 2],
                    }
                    if unfused_at == (heads, k, d):
                        s, p = (torch.empty(mat.nnz, dtype=tdt, device=DEV) for _ in range(2))
                        bias = torch.rand(mat.nnz, dtype=tdt, device=DEV, generator=gen)
                        O2 = torch.zeros_like(O)
                        slope_of = [float(x) for x in slopes.tolist()]

                        def unfused():
                            for h in range(heads):
                                if A.sddmm(Q[:, h], K[:, h], s):
                                    raise RuntimeError("sddmm failed")
                                s.add_(bias, alpha=slope_of[h])
                                if A.rowSoftmax(s, p) or A.updateValues(p) or A.spmm(V[:, h], O2[:, h]):
                                    raise RuntimeError("the unfused chain failed")
                        unfused()
                        tu, tb2 = timed(unfused, biased, args.batches, args.per_batch, min(args.warmup, 2))
                        if A.updateValues(zeros):
                            raise RuntimeError("updateValues failed")
                        line.update({"unfused_us": r(np.median(tu)), "unfused_min_us": r(min(tu)), "unfused_max_us": r(max(tu)),
                                     "biased_again_us": r(np.median(tb2)), "unfused_calls": 5 * heads,
                                     "unfused_over_biased": round(float(np.median(tu) / np.median(tb2)), 2)})
                        del s, p, bias, O2
                    print(json.dumps(line), flush=True)
                    if not equal:
                        raise SystemExit(f"the biased calls differ from mha at zero bias: {mat.name} {dn} heads={heads} k={k} d={d}")
                    del Q, K, V, dO, O, dQ, dK, dV, O1, dQ1, dK1, dV1, work, dS
                    torch.cuda.empty_cache()
            A.destroy()
            A.close()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
