#!/usr/bin/env python3
"""The dropped 16-bit-operand attention calls (csr5_attention_drop_lowp.hip, csr5_attention_bwd_drop_lowp.hip) on the CPU, without a
GPU: the kernel sources are compiled for the host against the stand-in for the HIP runtime (fake/hip/hip_runtime.h) with
-fsanitize=address,undefined and run as ONE stand-alone program (attention_driver.cpp with those two units and the float dropped
ones, csr5_attention_drop.hip and csr5_attention_bwd_drop.hip; emulation.py) on matrices of tests/zoo.py converted by the oracle; the
transpose, converted at another sigma, plays the transposed companion and the stable sort by column that forms it is the source map.
THE PATTERNS CARRY NO VALUE ARRAY (null pointers).

    python scripts/host_emulation/run_dropout_lowp.py [--matrices kat0,duplicates,class-edges,class-edges^T,dealt] [--types bf16,f16]
                                                      [--heads 1,3] [--kd 3x5,16x16] [--cxx clang++]

Q, K, V, dO, B, O, dQ, dK, dV AND dB ARE HEAP BLOCKS OF EXACTLY rows * ld 2-BYTE ELEMENTS, the workspace one of exactly 4 m heads floats
and the map one of exactly nnz words, so an index computed in 4-byte units, a 16-byte load past a row's end or a wrong rank is an
out-of-bounds access the address sanitizer reports.  Every padding element holds NaN.  Every (entry, head) has a distinct bias
(emulation.py ``distinct_bias``, rounded to the operand type).

Per matrix, operand type, heads and (k, d), with scale 0.37, p = 0.4, seed 2^63 + 5, offset 2^32 + 1 and head0 = 2 (three heads then
straddle a Philox block):
  * O, dQ, dK, dV and dB against the numpy float64 reference on the widened operands WITH THE REFERENCE MASK
    (tests/dropout_reference.py ``mask``, ``numpy_reference``; cd the float (float)(1 / (1 - p))): the dropped emulation's fp32 bound
    (tests/gat_reference.py ``within`` with the unit roundoff of float) plus one rounding to the operand type
    (tests/lowp_reference.round_allowance);
  * their words against the ROUNDING OF THE FLOAT DROPPED LAUNCHERS' results on the widened operands, which the program runs on the
    same case: the rounding is made here, in integer arithmetic (tests/lowp_reference.to_words), not by the compiler; and the workspace
    values M, 1 / Z and D against that launcher's, as float bits;
  * lines without entries exactly +0 (the word 0x0000), nothing written beyond the last column of an output;
  * equal words for sigma = 4 with the head groups of the rule, sigma = 7 with padded leading dimensions (odd: element loads, rows on
    2-byte boundaries) and ONE group, and sigma = 16 with one group (16-byte loads where k and d allow them);
  * a null B has the words of a B of +0; dQ and dB alone, without workspace, companion and map, have the words they have with them;
  * with p = 0 the words are those of the undropped float launchers' rounded results (run through the same program with p = 0: thr = 0,
    cd = 1), and they differ from the dropped ones wherever a row has entries.
This exercises the indexing, the line classes and the arithmetic of the source; it says nothing about the gfx950 build."""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle.csr5_oracle import Oracle  # noqa: E402
from scripts.host_emulation import emulation as EMU  # noqa: E402
from tests import dropout_reference as DR  # noqa: E402
from tests import gat_reference as G  # noqa: E402
from tests import lowp_reference as L  # noqa: E402

DEFAULT = "kat0,duplicates"
HEADS = (1, 3)
KD = ((3, 5), (16, 16))
SCALE, P = EMU.SCALE, 0.4
SEED, OFFSET, HEAD0 = 2 ** 63 + 5, 2 ** 32 + 1, 2
NAMES = DR.NAMES
PADS = dict(ldv=3, ldo=1, lddk=3)  # odd rows of 2-byte elements


def main():
    args = EMU.arguments(DEFAULT, HEADS, KD, kinds="types")
    orc = Oracle()
    mats = EMU.matrices()
    u32 = float(np.finfo(np.float32).eps) / 2
    c, cd = float(np.float32(SCALE)), DR.cd_of(P, np.float32)
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "dropout_lowp_host")
        EMU.build(args.cxx, exe, ("attention_drop", "attention_bwd_drop", "attention_drop_lowp", "attention_bwd_drop_lowp"))
        for name in args.matrices:
            pat = EMU.Patterns(orc, mats(name))
            mat = pat.mat
            empties = (pat.empty_r, pat.empty_r, pat.empty_c, pat.empty_c, None)
            for kind in args.types:
                for H in args.heads:
                    keep = DR.mask(mat.nnz, H, P, SEED, OFFSET, HEAD0)
                    for k, d in args.kd:
                        ops = tuple(L.to_words(t, kind) for t in EMU.operands(mat, H, k, d, np.float32))
                        B = L.to_words(EMU.distinct_bias(mat.nnz, H).astype(np.float32), kind)
                        Bf, Qf, Kf, Vf, dOf = (L.widen(t, kind) for t in (B,) + ops)
                        ref, mag = DR.numpy_reference(mat, c, Bf, Qf, Kf, Vf, dOf, keep, cd)
                        smag = float(abs(c) * (np.abs(Qf).sum(2).max() + 1) * (np.abs(Kf).sum(2).max() + 1) + 2) if mat.nnz else 0.0
                        where = (name, kind, H, k, d)
                        float_call = []

                        def both(sigma, sigma_t, pad, groups, want=None, B=B, p=P):
                            """[O, dQ, dK, dV, dB] as words (O: None with `want`); the float dropped launchers' five on the widened
                            operands go to float_call, and the two workspaces agree"""
                            common = dict(kind=kind, B=B, scalars=(SCALE, 0.0, p, SEED, OFFSET), head0=HEAD0, pads=PADS)
                            O = O32 = None
                            if not want:
                                O, O32 = EMU.launch(exe, tmp, EMU.DROP_LOWP, EMU.FORWARD, pat, (sigma, sigma_t), ops[:3], pad, groups, **common)
                            (Gr, W), (G32, W32) = EMU.launch(exe, tmp, EMU.DROP_LOWP, EMU.BACKWARD, pat, (sigma, sigma_t), ops, pad, groups,
                                                            want, **common)
                            if W is not None:
                                assert np.array_equal(W[:, :, :3].view(np.uint32), W32[:, :, :3].view(np.uint32)), where + (sigma, "the workspace")
                            float_call[:] = [O32] + G32
                            return [O] + Gr

                        def judge(i, g):
                            g32, r, a, got = float_call[i], ref[i], mag[i], L.widen(g, kind).astype(np.float64)
                            assert G.within(g32.astype(np.float64), r, a, smag, u32).all(), where + (NAMES[i], "the float launcher")
                            assert L.same_words(g, L.to_words(g32, kind), kind), where + (NAMES[i], "not the rounding of the float call")
                            ok = np.abs(got - r) <= 1e3 * u32 * (1 + smag) * np.maximum(a, 1e-30) + L.round_allowance(r, kind)
                            return ok, EMU.worst_of(got, r)
                        first, worst = EMU.check_configs(both, NAMES, empties, where, judge, isnan=lambda w: L.is_nan(w, kind))
                        EMU.check_same(both(7, 4, True, 0, B=None), both(7, 4, True, 0, B=np.zeros_like(B)), NAMES, where,
                                       "a null B against a B of +0")
                        EMU.check_same(both(7, 4, True, 1, want=9), first, NAMES, where, "dQ and dB alone")
                        plain = both(4, 16, False, 0, p=0.0)  # (thr = 0, cd = 1: the float launchers' are the undropped call's bits)
                        for i, g in enumerate(plain):
                            assert L.same_words(g, L.to_words(float_call[i], kind), kind), where + (NAMES[i], "p = 0")
                        if mat.nnz and 0 < keep.mean() < 1:
                            assert not EMU.same(plain[0], first[0]), where + ("the mask changes nothing",)
                        print(f"{name} {kind} heads={H} k={k} d={d}: ok, worst |error| {worst:.2e}", flush=True)


if __name__ == "__main__":
    main()
