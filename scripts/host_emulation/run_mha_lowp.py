#!/usr/bin/env python3
"""The 16-bit-operand multi-head entry (csr5_attention_lowp.hip) on the CPU, without a GPU: the kernel source is compiled for the
host against the stand-in for the HIP runtime (fake/hip/hip_runtime.h) with -fsanitize=address,undefined and run as a stand-alone
program (attention_driver.cpp with that unit and csr5_attention_edge.hip; emulation.py) on matrices of tests/zoo.py converted by
the oracle.  THE PATTERNS CARRY NO VALUE ARRAY (null pointers).

    python scripts/host_emulation/run_mha_lowp.py [--matrices kat0,duplicates,aligned1024,class-edges] [--types bf16,f16]
                                                  [--heads 1,3] [--kd 3x5,16x16] [--cxx clang++]

Q, K, V, B AND O ARE HEAP BLOCKS OF EXACTLY rows * ld 2-BYTE ELEMENTS, so an index computed in 4-byte units, or a 16-byte load past
a row's end, is an out-of-bounds access the address sanitizer reports.  Every padding element holds NaN: reading one poisons a
row.  Every (entry, head) has a distinct bias (emulation.py ``distinct_bias``, rounded to the operand type).

Per matrix, operand type, heads and (k, d), with scale 0.37:
  * O against a numpy float64 reference of softmax(scale Q K^T + B) V on the widened operands: the edge-bias emulation's fp32 bound
    (emulation.py ``within`` with the unit roundoff of float) plus one rounding to the operand type
    (tests/lowp_reference.round_allowance);
  * O's words against the ROUNDING OF csr5_attention_edge.hip's float launcher on the widened operands, which the program runs on the
    same case: the rounding is made here, in integer arithmetic (tests/lowp_reference.to_words), not by the compiler;
  * rows without entries exactly +0 (the word 0x0000), nothing written beyond column heads * d;
  * equal words for sigma = 4 with the head groups of the rule, sigma = 7 with padded leading dimensions (odd: element loads,
    rows on 2-byte boundaries) and ONE group, and sigma = 16 with one group (16-byte loads where k >= 16);
  * a null B has the words of a B of +0.
This exercises the indexing, the row classes and the arithmetic of the source; it says nothing about the gfx950 build."""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle.csr5_oracle import Oracle  # noqa: E402
from scripts.host_emulation import emulation as EMU  # noqa: E402
from tests import lowp_reference as L  # noqa: E402

DEFAULT = "kat0,duplicates"
HEADS = (1, 3)
KD = ((3, 5), (16, 16))
PADS = dict(ldv=3)  # odd rows of 2-byte elements


def main():
    args = EMU.arguments(DEFAULT, HEADS, KD, kinds="types")
    orc = Oracle()
    mats = EMU.matrices()
    u32 = float(np.finfo(np.float32).eps) / 2
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "mha_lowp_host")
        EMU.build(args.cxx, exe, ("attention_edge", "attention_lowp"))
        for name in args.matrices:
            pat = EMU.Patterns(orc, mats(name), companion=False)
            mat = pat.mat
            for kind in args.types:
                for H in args.heads:
                    for k, d in args.kd:
                        Q, K, V, _ = (L.to_words(t, kind) for t in EMU.operands(mat, H, k, d, np.float32))
                        B = L.to_words(EMU.distinct_bias(mat.nnz, H).astype(np.float32), kind)
                        Bf, Qf, Kf, Vf = (L.widen(t, kind) for t in (B, Q, K, V))
                        (ref, *_), (mag, *_), smag = EMU.edge_reference(mat, Bf, Qf, Kf, Vf, np.zeros((mat.m, H, d), dtype=np.float32))
                        where = (name, kind, H, k, d)
                        float_call = []

                        def forward(sigma, sigma_t, pad, groups, B=B):
                            """[O's words]; the float launcher's O on the widened operands goes to float_call"""
                            O, O32 = EMU.launch(exe, tmp, EMU.LOWP, EMU.FORWARD, pat, (sigma, sigma_t), (Q, K, V), pad, groups, kind=kind, B=B,
                                                scalars=(EMU.SCALE, 0.0, 0.0, 0, 0), pads=PADS)
                            float_call[:] = [O32]
                            return [O]

                        def judge(i, O):
                            O32, got = float_call[0], L.widen(O, kind).astype(np.float64)
                            assert EMU.within(O32.astype(np.float64), ref, mag, smag, u32).all(), where + ("the float launcher",)
                            assert L.same_words(O, L.to_words(O32, kind), kind), where + ("not the rounding of the float call",)
                            ok = np.abs(got - ref) <= 1e3 * u32 * (1 + smag) * np.maximum(mag, 1e-30) + L.round_allowance(ref, kind)
                            return ok, EMU.worst_of(got, ref)
                        _, worst = EMU.check_configs(forward, ("O",), (pat.empty_r,), where, judge, isnan=lambda w: L.is_nan(w, kind))
                        EMU.check_same(forward(7, 4, True, 0, B=None), forward(7, 4, True, 0, B=np.zeros_like(B)), ("O",), where,
                                       "a null B against a B of +0")
                        print(f"{name} {kind} heads={H} k={k} d={d}: ok, worst |error| {worst:.2e}", flush=True)


if __name__ == "__main__":
    main()
