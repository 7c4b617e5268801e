#!/usr/bin/env python3
"""The 16-bit-operand multi-head backward (csr5hip_mha_lowp_backward) against the fp32 call it is defined by, on the same fp32
handle and the same numbers; one JSON line per (workload, operand type, heads, k, d, with / without B and dB).

    python scripts/bench_mha_lowp_backward.py [--workloads scircuit,webbase,nd24k] [--types bf16,f16] [--heads 4,8]
                                              [--kd 16x16,64x64] [--bias 1,0]

bench_mha_lowp.py's protocol: per pair of routes the batches alternate, a batch is timed by device events, the figure is the median
of 7 batches of 10 calls after a warm-up, and the baseline's fastest and slowest batch are printed with it: their spread is the
margin of any ratio.  BEFORE ANY TIMING THE OUTPUTS ARE COMPARED by the rounding identity: mhaLowpBackward's dQ, dK, dV and dB must
be, as 16-bit words (NaN positionally), mhaEdgeBiasBackward's on the widened operands cast to the operand type.  Every call asks
for dQ, dK and dV, and with a bias for dB as well.

A, THE KERNELS: one mhaLowpBackward against one mhaEdgeBiasBackward on widened copies of Q, K, V, B and dO that are already in place
(lowp_us, fp32_us, ratio_a = lowp / fp32).
B, WHAT THE AUTOGRAD ROUTE DID BEFORE (the stopgap): one mhaLowpBackward against widening Q, K, V, B and dO to fp32 (five casts),
allocating the fp32 outputs and the workspace, mhaEdgeBiasBackward, and casting the gradients back (four casts with a bias)
(lowp_b_us, measured in this pair's own batches, stopgap_us, ratio_b = lowp / stopgap).
temporaries_bytes: what route B allocates per step and the 16-bit call does not -- the widened Q, K, V and dO and the three fp32
gradients, with a bias the widened B and the fp32 dB as well.  The workspace is float on both routes and is not counted.
There is no pass threshold: the figures are reported as they come, a ratio above 1 included."""
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
from scripts.bench_mha import timed  # noqa: E402
from scripts.bench_mha_lowp import TYPES, check, same_words  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="scircuit,webbase,nd24k")
    ap.add_argument("--types", default="bf16,f16")
    ap.add_argument("--heads", default="4,8")
    ap.add_argument("--kd", default="16x16,64x64")
    ap.add_argument("--bias", default="1,0", help="1: with B and dB, 0: without")
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--per-batch", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    kds = [tuple(int(v) for v in kd.split("x")) for kd in args.kd.split(",")]
    r = lambda v: round(float(v), 2)  # noqa: E731
    for wl in args.workloads.split(","):
        mat = WORKLOADS[wl](np.float32)
        rp = torch.from_numpy(mat.row_ptr).to(DEV)
        ci = torch.from_numpy(mat.col).to(DEV)
        va = torch.ones(mat.nnz, dtype=torch.float32, device=DEV)
        A = H.anonymouslibHandle(mat.m, mat.n, dtype="float32")
        rcs = [A.inputCSR(mat.nnz, rp, ci, va), A.setSigma(H.ANONYMOUSLIB_AUTO_TUNED_SIGMA), A.asCSR5(), A.buildTranspose()]
        if any(rcs):
            raise RuntimeError(f"handle setup failed: {rcs}")
        gen = torch.Generator(device=DEV).manual_seed(5)
        for tn in args.types.split(","):
            low = TYPES[tn]
            for heads in (int(h) for h in args.heads.split(",")):
                for k, d in kds:
                    def rand(rows, *shape):
                        return (torch.rand((rows,) + shape, dtype=torch.float32, device=DEV, generator=gen) * 2 - 1)
                    Q, K, V = (rand(mat.m, heads, k) / k ** 0.5).to(low), rand(mat.n, heads, k).to(low), rand(mat.n, heads, d).to(low)
                    dO, Bl = rand(mat.m, heads, d).to(low), (rand(mat.nnz, heads) * 2).to(low)
                    wide = [t.float() for t in (Q, K, V, dO, Bl)]
                    outs = [torch.empty_like(t) for t in (Q, K, V, Bl)]
                    outs32 = [torch.empty_like(t) for t in (wide[0], wide[1], wide[2], wide[4])]
                    work = torch.empty(4 * mat.m * heads, dtype=torch.float32, device=DEV)
                    work32 = torch.empty_like(work)
                    for with_b in (int(b) for b in args.bias.split(",")):
                        back = [None]

                        def lowp():
                            check(A.mhaLowpBackward(Q, K, V, dO, outs[0], outs[1], outs[2], work, B=Bl if with_b else None, scale=0.25,
                                                    dB=outs[3] if with_b else None), "mhaLowpBackward")

                        def fp32():
                            check(A.mhaEdgeBiasBackward(wide[0], wide[1], wide[2], wide[3], outs32[0], outs32[1], outs32[2], work32,
                                                        B=wide[4] if with_b else None, scale=0.25, dB=outs32[3] if with_b else None),
                                  "mhaEdgeBiasBackward")

                        def stopgap():  # autograd._LowpMultiheadAttention.backward's route on an fp64 handle, in fp32
                            q, kk, v, g = Q.float(), K.float(), V.float(), dO.float()
                            b = Bl.float() if with_b else None
                            o = [torch.empty_like(t) for t in (q, kk, v)]
                            w = torch.empty(4 * mat.m * heads, dtype=torch.float32, device=DEV)
                            db = torch.empty_like(b) if with_b else None
                            check(A.mhaEdgeBiasBackward(q, kk, v, g, o[0], o[1], o[2], w, B=b, scale=0.25, dB=db), "mhaEdgeBiasBackward")
                            back[0] = [t.to(low) for t in o] + ([db.to(low)] if with_b else [])
                        for f in (lowp, fp32, stopgap):
                            f()
                        torch.cuda.synchronize()
                        n_out = 4 if with_b else 3
                        equal = all(same_words(a, b.to(low)) for a, b in zip(outs[:n_out], outs32[:n_out])) and \
                            all(same_words(a, b) for a, b in zip(outs[:n_out], back[0]))
                        temporaries = 4 * sum(t.numel() for t in wide[:4]) + 4 * sum(t.numel() for t in outs32[:3]) + \
                            (4 * 2 * Bl.numel() if with_b else 0)
                        ta, tf = timed(lowp, fp32, args.batches, args.per_batch, args.warmup)
                        tb, tu = timed(lowp, stopgap, args.batches, args.per_batch, args.warmup)
                        print(json.dumps({
                            "workload": mat.name, "type": tn, "heads": heads, "k": k, "d": d, "bias": bool(with_b), "m": mat.m, "n": mat.n,
                            "nnz": mat.nnz, "rounding_identity": equal, "temporaries_bytes": int(temporaries),
                            "lowp_us": r(np.median(ta)), "fp32_us": r(np.median(tf)), "fp32_min_us": r(min(tf)), "fp32_max_us": r(max(tf)),
                            "ratio_a": round(float(np.median(ta) / np.median(tf)), 4),
                            "lowp_b_us": r(np.median(tb)), "stopgap_us": r(np.median(tu)), "stopgap_min_us": r(min(tu)),
                            "stopgap_max_us": r(max(tu)), "ratio_b": round(float(np.median(tb) / np.median(tu)), 4),
                        }), flush=True)
                        if not equal:
                            raise SystemExit(f"mhaLowpBackward is not the rounding of the fp32 call: {mat.name} {tn} heads={heads} k={k} d={d} "
                                             f"bias={with_b}")
                    del Q, K, V, dO, Bl, wide, outs, outs32, work, work32
                    torch.cuda.empty_cache()
        A.destroy()
        A.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
