#!/usr/bin/env python3
"""The dropped attention entries (csr5_attention_drop.hip, csr5_attention_drop_gat.hip, their backwards and the mask kernel) on the
CPU, without a GPU: the kernel sources are compiled for the host against the stand-in for the HIP runtime
(fake/hip/hip_runtime.h) with -fsanitize=address,undefined, and run as ONE stand-alone program (attention_driver.cpp with those
four units; emulation.py) on matrices of tests/zoo.py converted by the oracle; for the backward the transpose, converted at
another sigma, plays the transposed companion and the stable sort by column that forms it is the source map, as in run_gat.py.
THE PATTERNS CARRY NO VALUE ARRAY AT ALL.

    python scripts/host_emulation/run_dropout.py [--matrices kat0,duplicates,class-edges,class-edges^T,dealt] [--dtypes f64,f32]
                                                 [--heads 1,3,5] [--cxx clang++]

EVERY OPERAND, a, B, dB, dAr, THE MASK, THE WORKSPACE AND THE MAP IS A HEAP BLOCK OF EXACTLY ITS DECLARED SIZE, WITH NaN IN ALL
PADDING.  Every (entry, head) has a distinct bias.  Per matrix, precision and head count (5 crosses a Philox word group), with
(k, d) = (3, 5), scale 0.37, p = 0.4, seed 2^63 + 5, offset 2^32 + 1 and head0 = 2:
  * the mask kernel's bytes against tests/dropout_reference.py ``mask``, its padding bytes untouched;
  * the dot-product family: O, dQ, dK, dV and dB against the numpy float64 reference WITH THE REFERENCE MASK
    (``numpy_reference``), judged by tests/gat_reference.py ``within`` (a check of the indexing, not the accuracy test);
  * the additive family (a distinct per head and channel, negative_slope 0.2): O, dQ, dK, dV, dB and dAr against the same
    reference with the additive score and its derivative restated in float64 (``numpy_reference(gat=(a, ns))``);
  * rows and columns without entries exactly +0, nothing written beyond the last column of an output;
  * equal bits for sigma = 4 with the head groups of the rule and packed leading dimensions, sigma = 7 with padded leading
    dimensions and ONE group, and sigma = 16 with one group;
  * dQ and dB alone, without workspace, companion and map, have the bits they have with them.
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
from tests import dropout_reference as DR  # noqa: E402
from tests import gat_reference as G  # noqa: E402

DEFAULT = "kat0,duplicates"
HEADS = (1, 3, 5)
K, D = 3, 5
SCALE, SLOPE, P = EMU.SCALE, 0.2, 0.4
SEED, OFFSET, HEAD0 = 2 ** 63 + 5, 2 ** 32 + 1, 2
NAMES = G.NAMES  # (the dot-product family has no dAr)


def main():
    args = EMU.arguments(DEFAULT, HEADS)
    orc = Oracle()
    mats = EMU.matrices()
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "dropout_host")
        EMU.build(args.cxx, exe, ("attention_drop", "attention_bwd_drop", "attention_drop_gat", "attention_bwd_drop_gat"))
        for name in args.matrices:
            pat = EMU.Patterns(orc, mats(name))
            mat = pat.mat
            empties = (pat.empty_r, pat.empty_r, pat.empty_c, pat.empty_c, None, pat.empty_r)
            for dtype in args.dtypes:
                u = float(np.finfo(dtype).eps) / 2
                ns, c, cd = float(dtype(SLOPE)), float(dtype(SCALE)), DR.cd_of(P, dtype)
                for H in args.heads:
                    B = EMU.distinct_bias(mat.nnz, H).astype(dtype)
                    a = EMU.distinct_a(H, K, dtype)
                    ops = Q, K_, V, dO = EMU.operands(mat, H, K, D, dtype)
                    keep = DR.mask(mat.nnz, H, P, SEED, OFFSET, HEAD0)
                    assert 0 < keep.mean() < 1 or mat.nnz * H < 8
                    smag = float((abs(c) * (np.abs(Q).sum(2).max() + 1) * (np.abs(K_).sum(2).max() + 1) + 2)) if mat.nnz else 0.0
                    worst = 0.0
                    for variant in (EMU.DROP, EMU.DROP_GAT):
                        gat = variant == EMU.DROP_GAT
                        ref, mag = DR.numpy_reference(mat, c, B, Q, K_, V, dO, keep, cd, gat=(a, ns) if gat else None)
                        where = (name, np.dtype(dtype).name, H, variant)
                        common = dict(a=a if gat else None, B=B, scalars=(SCALE, SLOPE, P, SEED, OFFSET), head0=HEAD0)

                        def both(sigma, sigma_t, pad, groups, want=None):
                            O = None if want else EMU.launch(exe, tmp, variant, EMU.FORWARD, pat, (sigma, sigma_t), ops[:3], pad, groups,
                                                             **common)
                            return [O] + EMU.launch(exe, tmp, variant, EMU.BACKWARD, pat, (sigma, sigma_t), ops, pad, groups, want, **common)[0]
                        m_ = EMU.launch(exe, tmp, variant, EMU.MASK, pat, (4, 16), ops, True, **common)
                        assert np.array_equal(m_[:, :H], keep) and (m_[:, H:] == 0xFF).all(), (name, H, "the mask kernel")

                        def judge(i, g):
                            return G.within(g, ref[i], mag[i], smag, u), EMU.worst_of(g, ref[i])
                        first, w = EMU.check_configs(both, NAMES, empties, where, judge)
                        worst = max(worst, w)
                        EMU.check_same(both(7, 4, True, 1, want=9), first, NAMES, where, "dQ and dB alone")
                    print(f"{name} {np.dtype(dtype).name} heads={H} k={K} d={D}: ok, worst |error| {worst:.2e}", flush=True)


if __name__ == "__main__":
    main()
