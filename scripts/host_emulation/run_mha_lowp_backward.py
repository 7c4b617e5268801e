#!/usr/bin/env python3
"""The 16-bit-operand multi-head backward (csr5_attention_bwd_lowp.hip) on the CPU, without a GPU: the kernel source is compiled for
the host against the stand-in for the HIP runtime (fake/hip/hip_runtime.h) with -fsanitize=address,undefined and run as a
stand-alone program (attention_driver.cpp with that unit and csr5_attention_bwd_edge.hip; emulation.py) on matrices of tests/zoo.py
converted by the oracle; the transpose, converted at another sigma, plays the transposed companion and the stable sort by column
that forms it is the source map.  THE PATTERNS CARRY NO VALUE ARRAY (null pointers).

    python scripts/host_emulation/run_mha_lowp_backward.py [--matrices kat0,duplicates,class-edges,class-edges^T,dealt] [--types bf16,f16]
                                                           [--heads 1,3] [--kd 3x5,16x16] [--cxx clang++] [--wrong]

Q, K, V, dO, B, dQ, dK, dV AND dB ARE HEAP BLOCKS OF EXACTLY rows * ld 2-BYTE ELEMENTS, the workspace one of exactly 4 m heads floats
and the map one of exactly nnz words, so an index computed in 4-byte units, a 16-byte load past a row's end or a wrong rank is an
out-of-bounds access the address sanitizer reports.  Every padding element holds NaN: reading one poisons a line.  Every
(entry, head) has a distinct bias (emulation.py ``distinct_bias``, rounded to the operand type).

Per matrix, operand type, heads and (k, d), with scale 0.37:
  * dQ, dK, dV and dB against a numpy float64 reference on the widened operands: the edge-bias emulation's fp32 bound (emulation.py
    ``within`` with the unit roundoff of float) plus one rounding to the operand type (tests/lowp_reference.round_allowance);
  * their words against the ROUNDING OF csr5_attention_bwd_edge.hip's float launcher on the widened operands, which the program runs
    on the same case: the rounding is made here, in integer arithmetic (tests/lowp_reference.to_words), not by the compiler; and the
    workspace values M, 1 / Z and D against that launcher's, as float bits;
  * lines without entries exactly +0 (the word 0x0000), nothing written beyond the last column of an output (dB: beyond column
    heads - 1 of its rows of lddb elements);
  * equal words for sigma = 4 with the head groups of the rule, sigma = 7 with padded leading dimensions (odd: element loads, rows on
    2-byte boundaries) and ONE group, and sigma = 16 with one group (16-byte loads where k and d allow them);
  * a null B has the words of a B of +0; dQ and dB alone, without workspace, companion and map, have the words they have with them.
--wrong: the expectations above are also put to two WRONG kernels, modelled in numpy float64 from the reference (their outputs never
come from the program): "exact-once", every output the exact result rounded once to the operand type (a kernel whose last
multiplication or addition is folded into the conversion and skips the float rounding), and "work16", dK and dV from a workspace
whose M, 1 / Z and D were kept in the operand type.  A line per case says in how many words each differs from the expectation, and a
line per operand type and model sums them over the run.  "work16" must differ in every run.  "exact-once" differs from the right
kernel only where the float result lies within a float rounding of a tie of the operand type -- about one bf16 word in 2^15, one
fp16 word in 2^12 -- so on small matrices it may differ nowhere: its sum is asserted only from 2^20 words on (emulation.py's ``round_once``
is itself checked on constructed ties in tests/test_mha_lowp_backward_host.py).
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
from tests import lowp_reference as L  # noqa: E402

DEFAULT = "kat0,duplicates"
HEADS = (1, 3)
KD = ((3, 5), (16, 16))
SCALE = EMU.SCALE
NAMES = ("dQ", "dK", "dV", "dB")
PADS = dict(ldv=3, ldo=1, lddk=3)  # odd rows of 2-byte elements


def wrong_models(mat, kind, Bf, Qf, Kf, Vf, dOf, ref):
    """name -> [dQ, dK, dV, dB] words (None: that model says nothing about the output) of the two wrong kernels of the docstring"""
    Q, K, V, dO, B = (t.astype(np.float64) for t in (Qf, Kf, Vf, dOf, Bf))
    rows = np.repeat(np.arange(mat.m), np.diff(mat.row_ptr))
    cols = mat.col[:mat.nnz].astype(np.int64)
    H = Q.shape[1]
    s = SCALE * (Q[rows] * K[cols]).sum(2) + B
    M = np.full((mat.m, H), -np.inf)
    np.maximum.at(M, rows, s)
    Z = np.zeros((mat.m, H))
    np.add.at(Z, rows, np.exp(s - M[rows]))
    p = np.exp(s - M[rows]) / Z[rows]
    dp = (dO[rows] * V[cols]).sum(2)
    D = np.zeros((mat.m, H))
    np.add.at(D, rows, p * dp)
    narrow = lambda t: L.widen(L.to_words(t.astype(np.float32), kind), kind).astype(np.float64)  # noqa: E731
    with np.errstate(invalid="ignore", divide="ignore"):
        M16, r16, D16 = narrow(M), narrow(1 / Z), narrow(D)
        pc = np.exp(s - M16[rows]) * r16[rows]
    dsc = pc * (dp - D16[rows])
    dK, dV = np.zeros(K.shape), np.zeros(V.shape)
    np.add.at(dK, cols, SCALE * dsc[:, :, None] * Q[rows])
    np.add.at(dV, cols, pc[:, :, None] * dO[rows])
    return {"exact-once": [EMU.round_once(r, kind) for r in ref[1:]],
            "work16": [None, L.to_words(dK.astype(np.float32), kind), L.to_words(dV.astype(np.float32), kind), None]}


def main():
    args = EMU.arguments(DEFAULT, HEADS, KD, kinds="types", extra=(
        ("--wrong", dict(action="store_true", help="also show that the word comparison rejects the two modelled wrong kernels")),))
    orc = Oracle()
    mats = EMU.matrices()
    u32 = float(np.finfo(np.float32).eps) / 2
    rejected = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "mha_lowp_bwd_host")
        EMU.build(args.cxx, exe, ("attention_bwd_edge", "attention_bwd_lowp"))
        for name in args.matrices:
            pat = EMU.Patterns(orc, mats(name))
            mat = pat.mat
            for kind in args.types:
                for H in args.heads:
                    for k, d in args.kd:
                        ops = tuple(L.to_words(t, kind) for t in EMU.operands(mat, H, k, d, np.float32))
                        B = L.to_words(EMU.distinct_bias(mat.nnz, H).astype(np.float32), kind)
                        Bf, Qf, Kf, Vf, dOf = (L.widen(t, kind) for t in (B,) + ops)
                        ref, mag, smag = EMU.edge_reference(mat, Bf, Qf, Kf, Vf, dOf)
                        where = (name, kind, H, k, d)
                        float_call, expect = [], []

                        def backward(sigma, sigma_t, pad, groups, want=None, B=B):
                            """[dQ, dK, dV, dB] as words; the float launcher's four on the widened operands go to float_call, and the
                            two workspaces agree"""
                            (G, W), (G32, W32) = EMU.launch(exe, tmp, EMU.LOWP, EMU.BACKWARD, pat, (sigma, sigma_t), ops, pad, groups, want,
                                                            kind=kind, B=B, scalars=(SCALE, 0.0, 0.0, 0, 0), pads=PADS)
                            if W is not None:
                                assert np.array_equal(W[:, :, :3].view(np.uint32), W32[:, :, :3].view(np.uint32)), where + (sigma, "the workspace")
                            float_call[:] = G32
                            return G

                        def judge(i, g):
                            g32, r, a, got = float_call[i], ref[1 + i], mag[1 + i], L.widen(g, kind).astype(np.float64)
                            assert EMU.within(g32.astype(np.float64), r, a, smag, u32).all(), where + (NAMES[i], "the float launcher")
                            assert L.same_words(g, L.to_words(g32, kind), kind), where + (NAMES[i], "not the rounding of the float call")
                            if len(expect) < len(NAMES):  # (the first configuration's)
                                expect.append(L.to_words(g32, kind))
                            ok = np.abs(got - r) <= 1e3 * u32 * (1 + smag) * np.maximum(a, 1e-30) + L.round_allowance(r, kind)
                            return ok, EMU.worst_of(got, r)
                        first, worst = EMU.check_configs(backward, NAMES, (pat.empty_r, pat.empty_c, pat.empty_c, None), where, judge,
                                                         isnan=lambda w: L.is_nan(w, kind))
                        EMU.check_same(backward(7, 4, True, 0, B=None), backward(7, 4, True, 0, B=np.zeros_like(B)), NAMES, where,
                                       "a null B against a B of +0")
                        EMU.check_same(backward(7, 4, True, 1, want=9), first, NAMES, where, "dQ and dB alone")
                        print(f"{name} {kind} heads={H} k={k} d={d}: ok, worst |error| {worst:.2e}", flush=True)
                        if args.wrong:
                            for model, outs in wrong_models(mat, kind, Bf, Qf, Kf, Vf, dOf, ref).items():
                                bad = sum(int((~((o == e) | (L.is_nan(o, kind) & L.is_nan(e, kind)))).sum())
                                          for o, e in zip(outs, expect) if o is not None)
                                total = sum(o.size for o in outs if o is not None)
                                was = rejected.get((kind, model), (0, 0))
                                rejected[(kind, model)] = (was[0] + bad, was[1] + total)
                                print(f"{name} {kind} heads={H} k={k} d={d}: wrong kernel {model}, {bad} of {total} words differ", flush=True)
    for (kind, model), (bad, total) in sorted(rejected.items()):
        print(f"wrong kernel {model} {kind}: {'rejected' if bad else 'NOT rejected'}, {bad} of {total} words differ over the run", flush=True)
        assert bad > 0 or (model == "exact-once" and total < 2 ** 20), (kind, model, "a wrong kernel passes the word comparison")


if __name__ == "__main__":
    main()
