#!/usr/bin/env python3
"""The 16-bit-operand multi-head call (csr5hip_mha_lowp) against the fp32 call it is defined by, on the same fp32 handle and the
same numbers; one JSON line per (workload, operand type, heads, k, d, with / without B).

    python scripts/bench_mha_lowp.py [--workloads scircuit,webbase,nd24k] [--types bf16,f16] [--heads 4,8] [--kd 16x16,64x64]
                                     [--bias 1,0]

bench_mha.py's protocol: per pair of routes the batches alternate, a batch is timed by device events, the figure is the median
of 7 batches of 10 calls after a warm-up, and the baseline's fastest and slowest batch are printed with it: their spread is the
margin of any ratio.  BEFORE ANY TIMING THE OUTPUTS ARE COMPARED by the rounding identity: mhaLowp's O must be, as 16-bit words
(NaN positionally), mhaEdgeBias's O on the widened operands cast to the operand type.

A, THE KERNEL: one mhaLowp against one mhaEdgeBias on widened copies of Q, K, V, B that are already in place (lowp_us, fp32_us,
ratio_a = lowp / fp32).
B, WHAT A CALLER DOES TODAY: one mhaLowp against widening Q, K, V, B to fp32 (four casts), mhaEdgeBias, and casting O back
(lowp_us again, measured in this pair's own batches, upcast_us, ratio_b = lowp / upcast).
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

TYPES = {"bf16": torch.bfloat16, "f16": torch.float16}


def check(rc, what):
    if rc:
        raise RuntimeError(f"{what} failed: {rc}")


def same_words(a, b):
    """equal 16-bit words, or NaN in both"""
    return bool(((a.view(torch.int16) == b.view(torch.int16)) | (torch.isnan(a) & torch.isnan(b))).all())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="scircuit,webbase,nd24k")
    ap.add_argument("--types", default="bf16,f16")
    ap.add_argument("--heads", default="4,8")
    ap.add_argument("--kd", default="16x16,64x64")
    ap.add_argument("--bias", default="1,0", help="1: with B, 0: without")
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
        rcs = [A.inputCSR(mat.nnz, rp, ci, va), A.setSigma(H.ANONYMOUSLIB_AUTO_TUNED_SIGMA), A.asCSR5()]
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
                    Bl = (rand(mat.nnz, heads) * 2).to(low)
                    Q32, K32, V32, B32 = (t.float() for t in (Q, K, V, Bl))
                    O = torch.empty((mat.m, heads, d), dtype=low, device=DEV)
                    O32 = torch.empty((mat.m, heads, d), dtype=torch.float32, device=DEV)
                    for with_b in (int(b) for b in args.bias.split(",")):
                        Bt, Bw = (Bl, B32) if with_b else (None, None)
                        back = [None]

                        def lowp():
                            check(A.mhaLowp(Q, K, V, O, B=Bt, scale=0.25), "mhaLowp")

                        def fp32():
                            check(A.mhaEdgeBias(Q32, K32, V32, O32, B=Bw, scale=0.25), "mhaEdgeBias")

                        def upcast():
                            q, kk, v = Q.float(), K.float(), V.float()
                            check(A.mhaEdgeBias(q, kk, v, O32, B=Bt.float() if with_b else None, scale=0.25), "mhaEdgeBias")
                            back[0] = O32.to(low)
                        for f in (lowp, fp32, upcast):
                            f()
                        torch.cuda.synchronize()
                        equal = same_words(O, O32.to(low)) and same_words(O, back[0])
                        ta, tf = timed(lowp, fp32, args.batches, args.per_batch, args.warmup)
                        tb, tu = timed(lowp, upcast, args.batches, args.per_batch, args.warmup)
                        print(json.dumps({
                            "workload": mat.name, "type": tn, "heads": heads, "k": k, "d": d, "bias": bool(with_b), "m": mat.m, "n": mat.n,
                            "nnz": mat.nnz, "rounding_identity": equal,
                            "lowp_us": r(np.median(ta)), "fp32_us": r(np.median(tf)), "fp32_min_us": r(min(tf)), "fp32_max_us": r(max(tf)),
                            "ratio_a": round(float(np.median(ta) / np.median(tf)), 4),
                            "lowp_b_us": r(np.median(tb)), "upcast_us": r(np.median(tu)), "upcast_min_us": r(min(tu)),
                            "upcast_max_us": r(max(tu)), "ratio_b": round(float(np.median(tb) / np.median(tu)), 4),
                        }), flush=True)
                        if not equal:
                            raise SystemExit(f"mhaLowp is not the rounding of the fp32 call: {mat.name} {tn} heads={heads} k={k} d={d} bias={with_b}")
                    del Q, K, V, Bl, Q32, K32, V32, B32, O, O32
                    torch.cuda.empty_cache()
        A.destroy()
        A.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
