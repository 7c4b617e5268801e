#!/usr/bin/env python3
"""The dropped 16-bit-operand attention calls (csr5hip_dropout_mha_lowp and its backward) against their three neighbours, on the same
fp32 handle and the same numbers; one JSON line per (workload, operand type, heads, k, d, direction), always with a bias (and dB).

    python scripts/bench_attention_dropout_lowp.py [--workloads scircuit,webbase,nd24k] [--types bf16,f16] [--heads 4,8]
                                                   [--kd 16x16,64x64] [--directions forward,backward] [--p 0.6]

bench_mha_lowp_backward.py's protocol: per pair of routes the batches alternate, a batch is timed by device events, the figure is the
median of 7 batches of 10 calls after a warm-up, and the baseline's fastest and slowest batch are printed with it: their spread is
the margin of any ratio.  BEFORE ANY TIMING OF A POINT EVERY WANTED OUTPUT IS COMPARED by the rounding identity: the dropped 16-bit
call's O (forward) or dQ, dK, dV and dB (backward) must be, as 16-bit words (NaN positionally), the fp32 dropped call's on the widened
operands cast to the operand type, and the replaced route's result must be those words too.

A, THE PRICE OF THE MASK: the dropped 16-bit call against the undropped 16-bit call, mhaLowp / mhaLowpBackward (drop_us, lowp_us,
ratio_a = drop / lowp).
B, THE KERNELS: against the fp32 dropped call, dropoutMha / dropoutMhaBackward, on widened copies of the operands that are already in
place (drop_b_us, fp32_us, ratio_b = drop / fp32).
C, THE ROUTE IT REPLACES: against widening Q, K, V, B (and dO) to fp32, allocating the fp32 outputs (and the workspace), the fp32
dropped call, and casting the results back (drop_c_us, widen_us, ratio_c = drop / widen).  temporaries_mib: what that route
allocates per step and the 16-bit call does not -- the widened operands and the fp32 outputs; the workspace is float on both routes
and is not counted.
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

SCALE, SEED, OFFSET = 0.25, 2 ** 63 + 5, 2 ** 32 + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="scircuit,webbase,nd24k")
    ap.add_argument("--types", default="bf16,f16")
    ap.add_argument("--heads", default="4,8")
    ap.add_argument("--kd", default="16x16,64x64")
    ap.add_argument("--directions", default="forward,backward")
    ap.add_argument("--p", type=float, default=0.6)
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--per-batch", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    kds = [tuple(int(v) for v in kd.split("x")) for kd in args.kd.split(",")]
    drop = (args.p, SEED, OFFSET, 0)
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
                    O, O32 = torch.empty_like(dO), torch.empty_like(wide[3])
                    outs = [torch.empty_like(t) for t in (Q, K, V, Bl)]
                    outs32 = [torch.empty_like(t) for t in (wide[0], wide[1], wide[2], wide[4])]
                    work = torch.empty(4 * mat.m * heads, dtype=torch.float32, device=DEV)
                    work32 = torch.empty_like(work)
                    for direction in args.directions.split(","):
                        back = [None]
                        if direction == "forward":
                            def dropped():
                                check(A.dropoutMhaLowp(Q, K, V, O, *drop, B=Bl, scale=SCALE), "dropoutMhaLowp")

                            def undropped():
                                check(A.mhaLowp(Q, K, V, O, B=Bl, scale=SCALE), "mhaLowp")

                            def fp32():
                                check(A.dropoutMha(wide[0], wide[1], wide[2], O32, *drop, B=wide[4], scale=SCALE), "dropoutMha")

                            def widen():  # what a caller with 16-bit tensors and dropout did before: widen, the fp32 call, cast
                                q, kk, v, b = Q.float(), K.float(), V.float(), Bl.float()
                                o = torch.empty((mat.m, heads, d), dtype=torch.float32, device=DEV)
                                check(A.dropoutMha(q, kk, v, o, *drop, B=b, scale=SCALE), "dropoutMha")
                                back[0] = [o.to(low)]
                            got, got32 = lambda: [O], lambda: [O32]  # noqa: E731
                            temporaries = 4 * (Q.numel() + K.numel() + V.numel() + Bl.numel() + O.numel())
                        else:
                            def dropped():
                                check(A.dropoutMhaLowpBackward(Q, K, V, dO, *drop, dQ=outs[0], dK=outs[1], dV=outs[2], work=work, B=Bl,
                                                               scale=SCALE, dB=outs[3]), "dropoutMhaLowpBackward")

                            def undropped():
                                check(A.mhaLowpBackward(Q, K, V, dO, outs[0], outs[1], outs[2], work, B=Bl, scale=SCALE, dB=outs[3]),
                                      "mhaLowpBackward")

                            def fp32():
                                check(A.dropoutMhaBackward(wide[0], wide[1], wide[2], wide[3], *drop, dQ=outs32[0], dK=outs32[1], dV=outs32[2],
                                                           work=work32, B=wide[4], scale=SCALE, dB=outs32[3]), "dropoutMhaBackward")

                            def widen():
                                q, kk, v, g, b = Q.float(), K.float(), V.float(), dO.float(), Bl.float()
                                o = [torch.empty_like(t) for t in (q, kk, v, b)]
                                w = torch.empty(4 * mat.m * heads, dtype=torch.float32, device=DEV)
                                check(A.dropoutMhaBackward(q, kk, v, g, *drop, dQ=o[0], dK=o[1], dV=o[2], work=w, B=b, scale=SCALE, dB=o[3]),
                                      "dropoutMhaBackward")
                                back[0] = [t.to(low) for t in o]
                            got, got32 = lambda: outs, lambda: outs32  # noqa: E731
                            temporaries = 4 * (2 * (Q.numel() + K.numel() + V.numel() + Bl.numel()) + dO.numel())
                        for f in (fp32, widen, dropped):  # (the dropped call last: its outputs are the ones compared)
                            f()
                        torch.cuda.synchronize()
                        equal = all(same_words(a, b.to(low)) for a, b in zip(got(), got32())) and \
                            all(same_words(a, b) for a, b in zip(got(), back[0]))
                        ta, tl = timed(dropped, undropped, args.batches, args.per_batch, args.warmup)
                        tb, tf = timed(dropped, fp32, args.batches, args.per_batch, args.warmup)
                        tc, tw = timed(dropped, widen, args.batches, args.per_batch, args.warmup)
                        med = lambda t: float(np.median(t))  # noqa: E731
                        print(json.dumps({
                            "workload": mat.name, "type": tn, "heads": heads, "k": k, "d": d, "direction": direction, "p": args.p, "m": mat.m,
                            "n": mat.n, "nnz": mat.nnz, "rounding_identity": equal, "temporaries_mib": round(temporaries / 2 ** 20, 1),
                            "drop_us": r(med(ta)), "lowp_us": r(med(tl)), "lowp_min_us": r(min(tl)), "lowp_max_us": r(max(tl)),
                            "ratio_a": round(med(ta) / med(tl), 4),
                            "drop_b_us": r(med(tb)), "fp32_us": r(med(tf)), "fp32_min_us": r(min(tf)), "fp32_max_us": r(max(tf)),
                            "ratio_b": round(med(tb) / med(tf), 4),
                            "drop_c_us": r(med(tc)), "widen_us": r(med(tw)), "widen_min_us": r(min(tw)), "widen_max_us": r(max(tw)),
                            "ratio_c": round(med(tc) / med(tw), 4),
                        }), flush=True)
                        if not equal:
                            raise SystemExit(f"the dropped 16-bit call is not the rounding of the fp32 dropped call: {mat.name} {tn} "
                                             f"heads={heads} k={k} d={d} {direction}")
                    del Q, K, V, dO, Bl, wide, O, O32, outs, outs32, work, work32
                    torch.cuda.empty_cache()
        A.destroy()
        A.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
