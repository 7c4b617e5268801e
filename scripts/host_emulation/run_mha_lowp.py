#!/usr/bin/env python3
"""The 16-bit-operand multi-head entry (csr5_attention_lowp.hip) on the CPU, without a GPU: the kernel source is compiled for the
host against the stand-in for the HIP runtime (fake/hip/hip_runtime.h) with -fsanitize=address,undefined and run as a stand-alone
program (mha_lowp_main.cpp) on matrices of tests/zoo.py converted by the oracle.  THE PATTERNS CARRY NO VALUE ARRAY (null pointers).

    python scripts/host_emulation/run_mha_lowp.py [--matrices kat0,duplicates,aligned1024,class-edges] [--types bf16,f16]
                                                  [--heads 1,3] [--kd 3x5,16x16] [--cxx clang++]

Q, K, V, B AND O ARE HEAP BLOCKS OF EXACTLY rows * ld 2-BYTE ELEMENTS, so an index computed in 4-byte units, or a 16-byte load past
a row's end, is an out-of-bounds access the address sanitizer reports.  Every padding element holds NaN: reading one poisons a
row.  Every (entry, head) has a distinct bias (run_mha_edge_bias.distinct_bias, rounded to the operand type).

Per matrix, operand type, heads and (k, d), with scale 0.37:
  * O against a numpy float64 reference of softmax(scale Q K^T + B) V on the widened operands: run_mha_edge_bias's fp32 bound
    (``within`` with the unit roundoff of float) plus one rounding to the operand type (tests/lowp_reference.round_allowance);
  * O's words against the ROUNDING OF csr5_attention_edge.hip's float launcher on the widened operands, which the program runs on the
    same case: the rounding is made here, in integer arithmetic (tests/lowp_reference.to_words), not by the compiler;
  * rows without entries exactly +0 (the word 0x0000), nothing written beyond column heads * d;
  * equal words for sigma = 4 with the head groups of the rule, sigma = 7 with padded leading dimensions (odd: element loads,
    rows on 2-byte boundaries) and ONE group, and sigma = 16 with one group (16-byte loads where k >= 16);
  * a null B has the words of a B of +0.
This exercises the indexing, the row classes and the arithmetic of the source; it says nothing about the gfx950 build."""
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
from scripts.host_emulation.run_mha_edge_bias import SCALE, distinct_bias, execute, reference, within  # noqa: E402
from tests import lowp_reference as L  # noqa: E402

DEFAULT = "kat0,duplicates"
HEADS = (1, 3)
KD = ((3, 5), (16, 16))
CONFIGS = ((4, False, 0), (7, True, 1), (16, False, 1))  # sigma, padded, head groups (0: the rule)


def wide_words(w, ld, kind):
    """(rows, ...) words packed into rows of ld elements, EXACTLY rows * ld of them, the padding NaN"""
    out = np.full((w.shape[0], ld), L.NAN_WORD[kind], dtype=np.uint16)
    out[:, :int(np.prod(w.shape[1:]))] = w.reshape(w.shape[0], -1)
    return out


def operands(mat, H, k, d, kind, seed=5):
    """(B, Q, K, V) as words of the operand type; run_mha_edge_bias's distributions, rounded once"""
    rng = np.random.default_rng(seed)
    Q = (rng.uniform(-1, 1, (mat.m, H, k)) * 2).astype(np.float32)
    K = rng.uniform(-1, 1, (mat.n, H, k)).astype(np.float32)
    V = rng.uniform(-1, 1, (mat.n, H, d)).astype(np.float32)
    B = distinct_bias(mat.nnz, H).astype(np.float32)
    return tuple(L.to_words(t, kind) for t in (B, Q, K, V))


def forward(exe, tmp, fmt, mat, sigma, kind, B, use_b, Q, K, V, pad, groups):
    """(O's words (m, H, d), the float launcher's O (m, H, d) on the widened operands)"""
    (_, H, k), d = Q.shape, V.shape[2]
    ldq, ldk, ldv, ldo = (H * k + 3, H * k + 1, H * d + 3, H * d + 3) if pad else (H * k, H * k, H * d, H * d)
    ldb = H + 2 if pad else H
    header = [mat.m, mat.n, mat.nnz, sigma, fmt.p, k, d, ldq, ldk, ldv, ldo, int(kind == "bf16"), H, groups, int(use_b), ldb]
    out = execute(exe, tmp, header, SCALE, ((mat, fmt),),
                  (wide_words(B, ldb, kind), wide_words(Q, ldq, kind), wide_words(K, ldk, kind), wide_words(V, ldv, kind)),
                  f"{mat.name} sigma {sigma}")
    raw = np.fromfile(out, dtype=np.uint8)
    O = raw[:2 * mat.m * ldo].view(np.uint16).reshape(mat.m, ldo)
    O32 = raw[2 * mat.m * ldo:].view(np.float32).reshape(mat.m, ldo)
    assert (O[:, H * d:] == 0xFFFF).all() and np.isnan(O32[:, H * d:]).all(), "written beyond column heads * d"
    return np.ascontiguousarray(O[:, :H * d]).reshape(mat.m, H, d), np.ascontiguousarray(O32[:, :H * d]).reshape(mat.m, H, d)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrices", default=DEFAULT)
    ap.add_argument("--types", default=",".join(L.KINDS))
    ap.add_argument("--heads", default=",".join(str(h) for h in HEADS))
    ap.add_argument("--kd", default=",".join(f"{k}x{d}" for k, d in KD))
    ap.add_argument("--cxx", default="/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else "clang++")
    args = ap.parse_args()
    heads = [int(h) for h in args.heads.split(",")]
    kds = [tuple(int(v) for v in kd.split("x")) for kd in args.kd.split(",")]
    orc = Oracle()
    mats = matrices()
    u32 = float(np.finfo(np.float32).eps) / 2
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "mha_lowp_host")
        build(args.cxx, "mha_lowp_main.cpp", exe)
        for name in args.matrices.split(","):
            mat = mats(name)
            conv = {s: orc.convert(64, s, mat.m, mat.row_ptr, mat.col, np.ones(mat.nnz)) for s in (4, 7, 16)}
            empty = np.diff(mat.row_ptr) == 0
            for kind in args.types.split(","):
                for H in heads:
                    for k, d in kds:
                        B, Q, K, V = operands(mat, H, k, d, kind)
                        Bf, Qf, Kf, Vf = (L.widen(t, kind) for t in (B, Q, K, V))
                        (ref, *_), (mag, *_), smag = reference(mat, Bf, Qf, Kf, Vf, np.zeros((mat.m, H, d), dtype=np.float32))
                        first, worst = None, 0.0
                        for sigma, pad, groups in CONFIGS:
                            O, O32 = forward(exe, tmp, conv[sigma], mat, sigma, kind, B, True, Q, K, V, pad, groups)
                            assert not L.is_nan(O, kind).any(), (name, kind, H, k, d, sigma, "unwritten or poisoned")
                            got = L.widen(O, kind).astype(np.float64)
                            ok = np.abs(got - ref) <= 1e3 * u32 * (1 + smag) * np.maximum(mag, 1e-30) + L.round_allowance(ref, kind)
                            assert within(O32.astype(np.float64), ref, mag, smag, u32).all(), (name, kind, H, k, d, sigma, "the float launcher")
                            assert ok.all(), (name, kind, H, k, d, sigma, float(np.abs(got - ref).max()))
                            assert L.same_words(O, L.to_words(O32, kind), kind), (name, kind, H, k, d, sigma, "not the rounding of the float call")
                            assert not O[empty].any(), "a row without entries is not +0"
                            worst = max(worst, float(np.abs(got - ref).max()) if got.size else 0.0)
                            first = O if first is None else first
                            assert np.array_equal(O, first), (name, kind, H, k, d, sigma, "words")
                        zero = np.zeros_like(B)
                        with_zero, _ = forward(exe, tmp, conv[7], mat, 7, kind, zero, True, Q, K, V, True, 0)
                        without, _ = forward(exe, tmp, conv[7], mat, 7, kind, zero, False, Q, K, V, True, 0)
                        assert np.array_equal(without, with_zero), (name, kind, H, k, d, "a null B against a B of +0")
                        print(f"{name} {kind} heads={H} k={k} d={d}: ok, worst |error| {worst:.2e}", flush=True)


if __name__ == "__main__":
    main()
