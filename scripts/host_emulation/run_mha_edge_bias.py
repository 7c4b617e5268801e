#!/usr/bin/env python3
"""The edge-bias multi-head entries (csr5_attention_edge.hip, csr5_attention_bwd_edge.hip) on the CPU, without a GPU: the kernel
sources are compiled for the host against the stand-in for the HIP runtime (fake/hip/hip_runtime.h) with
-fsanitize=address,undefined, and run as a stand-alone program (attention_driver.cpp with those two units; emulation.py) on
matrices of tests/zoo.py converted by the oracle; for the backward the transpose, converted at another sigma, plays the transposed
companion and the stable sort by column that forms it is the source map.  THE PATTERNS CARRY NO VALUE ARRAY AT ALL (null pointers).

    python scripts/host_emulation/run_mha_edge_bias.py [--matrices kat0,one-row,duplicates,aligned64,aligned1024,class-edges,class-edges^T,dealt]
                                                       [--dtypes f64,f32] [--heads 1,3] [--kd 3x5,8x16] [--cxx clang++]

EVERY (ENTRY, HEAD) HAS A DISTINCT BIAS (a permutation of nnz heads equidistant values in [-2, 2)), so a bias taken from another
entry or another head -- at a wrong rank, without the map on the column side, with a wrong row stride -- is an error of order one;
AND B, dB AND THE MAP ARE HEAP BLOCKS OF EXACTLY nnz ldb, nnz lddb AND nnz ELEMENTS, so an index beyond them is an out-of-bounds
access the address sanitizer reports.  The padding columns of B hold NaN: reading one poisons a row.

Per matrix, precision, heads and (k, d), with scale 0.37:
  * O, dQ, dK, dV and dB against a numpy float64 reference of softmax(scale Q K^T + B) (emulation.py ``edge_reference``;
    ``within``: 1e3 unit roundoffs of the expression on absolute values, times one plus the largest score magnitude: a check of
    the indexing, not the accuracy test);
  * rows and columns without entries exactly +0, nothing written beyond the last column of an output (dB: beyond column
    heads - 1 of its rows of lddb values), nothing at all into an output that is not wanted;
  * equal bits for sigma = 4 with the head groups of the rule and ldb = lddb = heads, sigma = 7 with padded leading dimensions
    (ldb = heads + 2, lddb = heads + 3) and ONE group, and sigma = 16 with one group;
  * a null B has the bits of a B of +0;
  * dQ and dB alone, without workspace, companion and map, have the bits they have with them.
Every array is an exact-size heap block.  This exercises the indexing, the row classes and the arithmetic of the source; it says
nothing about the gfx950 build."""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle.csr5_oracle import Oracle  # noqa: E402
from scripts.host_emulation import emulation as EMU  # noqa: E402

DEFAULT = "kat0,one-row,duplicates,aligned64,aligned1024,class-edges,class-edges^T,dealt"
HEADS = (1, 3)
KD = ((3, 5), (8, 16))
NAMES = EMU.EDGE_NAMES


def main():
    args = EMU.arguments(DEFAULT, HEADS, KD)
    orc = Oracle()
    mats = EMU.matrices()
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "mha_edge_host")
        EMU.build(args.cxx, exe, ("attention_edge", "attention_bwd_edge"))
        for name in args.matrices:
            pat = EMU.Patterns(orc, mats(name))
            empties = (pat.empty_r, pat.empty_r, pat.empty_c, pat.empty_c, None)
            for dtype in args.dtypes:
                u = float(np.finfo(dtype).eps) / 2
                for H in args.heads:
                    B = EMU.distinct_bias(pat.mat.nnz, H).astype(dtype)
                    for k, d in args.kd:
                        ops = EMU.operands(pat.mat, H, k, d, dtype)
                        ref, mag, smag = EMU.edge_reference(pat.mat, B, *ops)
                        where = (name, np.dtype(dtype).name, H, k, d)

                        def both(sigma, sigma_t, pad, groups, want=None, B=B):
                            common = dict(B=B, scalars=(EMU.SCALE, 0.0, 0.0, 0, 0))
                            O = None if want else EMU.launch(exe, tmp, EMU.EDGE, EMU.FORWARD, pat, (sigma, sigma_t), ops[:3], pad, groups,
                                                             **common)
                            return [O] + EMU.launch(exe, tmp, EMU.EDGE, EMU.BACKWARD, pat, (sigma, sigma_t), ops, pad, groups, want,
                                                    **common)[0]

                        def judge(i, g):
                            return EMU.within(g, ref[i], mag[i], smag, u), EMU.worst_of(g, ref[i])
                        first, worst = EMU.check_configs(both, NAMES, empties, where, judge)
                        EMU.check_same(both(7, 4, True, 0, B=None), both(7, 4, True, 0, B=np.zeros_like(B)), NAMES, where,
                                       "a null B against a B of +0")
                        EMU.check_same(both(7, 4, True, 1, want=9), first, NAMES, where, "dQ and dB alone")
                        print(f"{name} {np.dtype(dtype).name} heads={H} k={k} d={d}: ok, worst |error| {worst:.2e}", flush=True)


if __name__ == "__main__":
    main()
