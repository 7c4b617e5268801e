#!/usr/bin/env python3
"""The 16-bit-operand multi-head backward (csr5_attention_bwd_lowp.hip) on the CPU, without a GPU: the kernel source is compiled for
the host against the stand-in for the HIP runtime (fake/hip/hip_runtime.h) with -fsanitize=address,undefined and run as a
stand-alone program (mha_lowp_bwd_main.cpp) on matrices of tests/zoo.py converted by the oracle; the transpose, converted at another
sigma, plays the transposed companion and the stable sort by column that forms it is the source map.  THE PATTERNS CARRY NO VALUE
ARRAY (null pointers).

    python scripts/host_emulation/run_mha_lowp_backward.py [--matrices kat0,duplicates,class-edges,class-edges^T,dealt] [--types bf16,f16]
                                                           [--heads 1,3] [--kd 3x5,16x16] [--cxx clang++] [--wrong]

Q, K, V, dO, B, dQ, dK, dV AND dB ARE HEAP BLOCKS OF EXACTLY rows * ld 2-BYTE ELEMENTS, the workspace one of exactly 4 m heads floats
and the map one of exactly nnz words, so an index computed in 4-byte units, a 16-byte load past a row's end or a wrong rank is an
out-of-bounds access the address sanitizer reports.  Every padding element holds NaN: reading one poisons a line.  Every
(entry, head) has a distinct bias (run_mha_edge_bias.distinct_bias, rounded to the operand type).

Per matrix, operand type, heads and (k, d), with scale 0.37:
  * dQ, dK, dV and dB against a numpy float64 reference on the widened operands: run_mha_edge_bias's fp32 bound (``within`` with the
    unit roundoff of float) plus one rounding to the operand type (tests/lowp_reference.round_allowance);
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
fp16 word in 2^12 -- so on small matrices it may differ nowhere: its sum is asserted only from 2^20 words on (``round_once`` itself
is checked on constructed ties in tests/test_mha_lowp_backward_host.py).
This exercises the indexing, the line classes and the arithmetic of the source; it says nothing about the gfx950 build."""
import argparse
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle.csr5_oracle import Oracle  # noqa: E402
from scripts.host_emulation.run_attention_backward import matrices  # noqa: E402
from scripts.host_emulation.run_mha import build  # noqa: E402
from scripts.host_emulation.run_mha_edge_bias import SCALE, distinct_bias, execute, reference, transpose_with_map, within  # noqa: E402
from scripts.host_emulation.run_mha_lowp import wide_words  # noqa: E402
from tests import lowp_reference as L  # noqa: E402

DEFAULT = "kat0,duplicates"
HEADS = (1, 3)
KD = ((3, 5), (16, 16))
CONFIGS = ((4, 16, False, 0), (7, 4, True, 1), (16, 7, False, 1))  # sigma, the companion's sigma, padded, head groups (0: the rule)
NAMES = ("dQ", "dK", "dV", "dB")


def operands(mat, H, k, d, kind, seed=5):
    """(B, Q, K, V, dO) as words of the operand type; run_mha_edge_bias's distributions, rounded once"""
    rng = np.random.default_rng(seed)
    Q = (rng.uniform(-1, 1, (mat.m, H, k)) * 2).astype(np.float32)
    K = rng.uniform(-1, 1, (mat.n, H, k)).astype(np.float32)
    V = rng.uniform(-1, 1, (mat.n, H, d)).astype(np.float32)
    dO = rng.uniform(-1, 1, (mat.m, H, d)).astype(np.float32)
    B = distinct_bias(mat.nnz, H).astype(np.float32)
    return tuple(L.to_words(t, kind) for t in (B, Q, K, V, dO))


def backward(exe, tmp, fmts, mats, sigmas, amap, kind, B, use_b, Q, K, V, dO, pad, groups, want=15):
    """([dQ, dK, dV, dB] as words, the float launcher's four, the two workspaces (m, H, 4)); None where not wanted"""
    (_, H, k), d = Q.shape, V.shape[2]
    wk, wd = H * k, H * d
    lds = (wk + 3, wk + 1, wd + 3, wd + 1, wk + 1, wk + 3, wd + 1) if pad else (wk, wk, wd, wd, wk, wk, wd)
    ldb, lddb = (H + 2, H + 3) if pad else (H, H)
    mat, matT = mats
    header = [mat.m, mat.n, mat.nnz, sigmas[0], fmts[0].p, sigmas[1], fmts[1].p, k, d, *lds, int(kind == "bf16"), want, H, groups,
              int(use_b), ldb, lddb]
    arrays = [amap.astype(np.uint32), wide_words(B, ldb, kind)] + [wide_words(t, ld, kind) for t, ld in zip((Q, K, V, dO), lds[:4])]
    out = execute(exe, tmp, header, SCALE, zip(mats, fmts), arrays, f"{mat.name} sigma {sigmas}")
    raw = np.fromfile(out, dtype=np.uint8)
    shapes = ((1, mat.m, lds[4], wk), (2, mat.n, lds[5], wk), (4, mat.n, lds[6], wd), (8, mat.nnz, lddb, H))
    wn = 4 * mat.m * H
    res, at = [], 0
    for size, dt, poison in ((2, np.uint16, lambda g: g == 0xFFFF), (4, np.float32, np.isnan)):
        outs = []
        for bit, rows, ld, width in shapes:
            g = raw[at:at + size * rows * ld].view(dt).reshape(rows, ld)
            at += size * rows * ld
            assert poison(g[:, width:]).all(), "written beyond the last column"
            if want & bit:
                outs.append(np.ascontiguousarray(g[:, :width]).reshape((rows, H, width // H) if bit != 8 else (rows, H)))
            else:
                assert poison(g).all(), "an output that was not wanted is written"
                outs.append(None)
        res.append(outs)
        res.append(raw[at:at + 4 * wn].view(np.float32).reshape(mat.m, H, 4))
        at += 4 * wn
    assert at == raw.size
    return res[0], res[2], (res[1], res[3])


def round_once(x, kind):
    """float64 -> words of the operand type in ONE rounding to nearest even: through float32 rounded TO ODD, which keeps the sticky
    information the second rounding needs"""
    x = np.asarray(x, dtype=np.float64)
    f = x.astype(np.float32)
    over = np.abs(f.astype(np.float64)) > np.abs(x)
    f = np.where(over, np.nextafter(f, np.float32(0)), f)  # truncated toward zero ...
    inexact = f.astype(np.float64) != x
    f = (f.view(np.uint32) | inexact.astype(np.uint32)).view(np.float32)  # ... and the sticky bit
    return L.to_words(f, kind)


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
    return {"exact-once": [round_once(r, kind) for r in ref[1:]],
            "work16": [None, L.to_words(dK.astype(np.float32), kind), L.to_words(dV.astype(np.float32), kind), None]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrices", default=DEFAULT)
    ap.add_argument("--types", default=",".join(L.KINDS))
    ap.add_argument("--heads", default=",".join(str(h) for h in HEADS))
    ap.add_argument("--kd", default=",".join(f"{k}x{d}" for k, d in KD))
    ap.add_argument("--cxx", default="/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else "clang++")
    ap.add_argument("--wrong", action="store_true", help="also show that the word comparison rejects the two modelled wrong kernels")
    args = ap.parse_args()
    heads = [int(h) for h in args.heads.split(",")]
    kds = [tuple(int(v) for v in kd.split("x")) for kd in args.kd.split(",")]
    orc = Oracle()
    mats = matrices()
    u32 = float(np.finfo(np.float32).eps) / 2
    rejected = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "mha_lowp_bwd_host")
        build(args.cxx, "mha_lowp_bwd_main.cpp", exe)
        for name in args.matrices.split(","):
            mat = mats(name)
            matT, amap = transpose_with_map(mat)
            ones = np.ones(mat.nnz)
            conv = {s: orc.convert(64, s, mat.m, mat.row_ptr, mat.col, ones) for s in (4, 7, 16)}
            convT = {s: orc.convert(64, s, matT.m, matT.row_ptr, matT.col, ones) for s in (4, 7, 16)}
            empty_r, empty_c = np.diff(mat.row_ptr) == 0, np.diff(matT.row_ptr) == 0
            for kind in args.types.split(","):
                for H in heads:
                    for k, d in kds:
                        B, Q, K, V, dO = operands(mat, H, k, d, kind)
                        Bf, Qf, Kf, Vf, dOf = (L.widen(t, kind) for t in (B, Q, K, V, dO))
                        ref, mag, smag = reference(mat, Bf, Qf, Kf, Vf, dOf)
                        first, expect, worst = None, None, 0.0
                        for sigma, sigma_t, pad, groups in CONFIGS:
                            G, G32, (W, W32) = backward(exe, tmp, (conv[sigma], convT[sigma_t]), (mat, matT), (sigma, sigma_t), amap, kind, B,
                                                        True, Q, K, V, dO, pad, groups)
                            where = (name, kind, H, k, d, sigma)
                            for g, g32, r, a, e, what in zip(G, G32, ref[1:], mag[1:], (empty_r, empty_c, empty_c, None), NAMES):
                                assert not L.is_nan(g, kind).any(), where + (what, "unwritten or poisoned")
                                got = L.widen(g, kind).astype(np.float64)
                                assert within(g32.astype(np.float64), r, a, smag, u32).all(), where + (what, "the float launcher")
                                ok = np.abs(got - r) <= 1e3 * u32 * (1 + smag) * np.maximum(a, 1e-30) + L.round_allowance(r, kind)
                                assert ok.all(), where + (what, float(np.abs(got - r).max()))
                                assert L.same_words(g, L.to_words(g32, kind), kind), where + (what, "not the rounding of the float call")
                                if e is not None:
                                    assert not g[e].any(), f"{what}: a line without entries is not +0"
                                worst = max(worst, float(np.abs(got - r).max()) if got.size else 0.0)
                            assert np.array_equal(W[:, :, :3].view(np.uint32), W32[:, :, :3].view(np.uint32)), where + ("the workspace",)
                            first = G if first is None else first
                            expect = [L.to_words(g32, kind) for g32 in G32] if expect is None else expect
                            for g, g0, what in zip(G, first, NAMES):
                                assert np.array_equal(g, g0), where + (what, "words")
                        zero = np.zeros_like(B)
                        run7 = lambda b, use, groups=0, want=15: backward(exe, tmp, (conv[7], convT[4]), (mat, matT), (7, 4), amap, kind, b,  # noqa: E731
                                                                          use, Q, K, V, dO, True, groups, want)[0]
                        for g, g0, what in zip(run7(zero, False), run7(zero, True), NAMES):
                            assert np.array_equal(g, g0), (name, kind, H, k, d, what, "a null B against a B of +0")
                        alone = run7(B, True, 1, 9)
                        assert np.array_equal(alone[0], first[0]) and np.array_equal(alone[3], first[3]), (name, kind, H, k, d, "dQ and dB alone")
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
