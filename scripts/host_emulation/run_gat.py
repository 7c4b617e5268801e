#!/usr/bin/env python3
"""The additive attention entries (csr5_attention_gat.hip, csr5_attention_bwd_gat.hip) on the CPU, without a GPU: the kernel sources
are compiled for the host against the stand-in for the HIP runtime (fake/hip/hip_runtime.h) with -fsanitize=address,undefined, and
run as ONE stand-alone program (attention_driver.cpp with those two units; emulation.py) on matrices of tests/zoo.py converted by
the oracle; for the backward the transpose, converted at another sigma, plays the transposed companion and the stable sort by
column that forms it is the source map, as in run_mha_edge_bias.py.  THE PATTERNS CARRY NO VALUE ARRAY AT ALL (null pointers).

    python scripts/host_emulation/run_gat.py [--matrices kat0,duplicates,class-edges,class-edges^T,dealt] [--dtypes f64,f32]
                                             [--heads 1,3] [--kd 1x5,3x5] [--cxx clang++]

EVERY OPERAND, a, B, dB, dAr, THE WORKSPACE AND THE MAP IS A HEAP BLOCK OF EXACTLY ITS DECLARED SIZE, WITH NaN IN ALL PADDING: an index
beyond a block is an out-of-bounds access the address sanitizer reports, and a padding element that is read poisons a row.  Every
(entry, head) has a distinct bias and every (head, channel) a distinct a, so an element taken from another entry, head or channel
is an error of order one.

Per matrix, precision, heads and (k, d), with scale 0.37 and negative_slope 0.2:
  * O, dQ, dK, dV, dB and dAr against the numpy float64 reference of tests/gat_reference.py (``numpy_reference``; ``within``: a check
    of the indexing, not the accuracy test);
  * rows and columns without entries exactly +0, nothing written beyond the last column of an output, nothing at all into an
    output that is not wanted;
  * equal bits for sigma = 4 with the head groups of the rule and packed leading dimensions, sigma = 7 with padded leading
    dimensions and ONE group, and sigma = 16 with one group;
  * a null a has the bits of an a of ones, a null B those of a B of +0;
  * dQ, dAr and dB alone, without workspace, companion and map, have the bits they have with them; dAr alone too.
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
from tests import gat_reference as G  # noqa: E402

DEFAULT = "kat0,duplicates"
HEADS = (1, 3)
KD = ((1, 5), (3, 5))
SCALE, SLOPE = EMU.SCALE, 0.2
NAMES = G.NAMES


def main():
    args = EMU.arguments(DEFAULT, HEADS, KD)
    orc = Oracle()
    mats = EMU.matrices()
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "gat_host")
        EMU.build(args.cxx, exe, ("attention_gat", "attention_bwd_gat"))
        for name in args.matrices:
            pat = EMU.Patterns(orc, mats(name))
            mat = pat.mat
            empties = (pat.empty_r, pat.empty_r, pat.empty_c, pat.empty_c, None, pat.empty_r)
            for dtype in args.dtypes:
                u = float(np.finfo(dtype).eps) / 2
                ns = float(dtype(SLOPE))
                for H in args.heads:
                    B = EMU.distinct_bias(mat.nnz, H).astype(dtype)
                    for k, d in args.kd:
                        a = EMU.distinct_a(H, k, dtype)
                        ops = EMU.operands(mat, H, k, d, dtype)
                        ref, mag, smag = G.numpy_reference(mat, a, ns, float(dtype(SCALE)), B, *ops)
                        where = (name, np.dtype(dtype).name, H, k, d)

                        def both(sigma, sigma_t, pad, groups, want=None, a=a, B=B):
                            common = dict(a=a, B=B, scalars=(SCALE, SLOPE, 0.0, 0, 0))
                            O = None if want else EMU.launch(exe, tmp, EMU.GAT, EMU.FORWARD, pat, (sigma, sigma_t), ops[:3], pad, groups,
                                                             **common)
                            return [O] + EMU.launch(exe, tmp, EMU.GAT, EMU.BACKWARD, pat, (sigma, sigma_t), ops, pad, groups, want,
                                                    **common)[0]

                        def judge(i, g):
                            return G.within(g, ref[i], mag[i], smag, u), EMU.worst_of(g, ref[i])
                        first, worst = EMU.check_configs(both, NAMES, empties, where, judge)
                        EMU.check_same(both(7, 4, True, 0, a=None, B=None), both(7, 4, True, 0, a=np.ones_like(a), B=np.zeros_like(B)), NAMES,
                                       where, "a null a and a null B against ones and +0")
                        EMU.check_same(both(7, 4, True, 1, want=25), first, NAMES, where, "dQ, dB and dAr alone")
                        EMU.check_same(both(7, 4, True, 1, want=16), first, NAMES, where, "dAr alone")
                        print(f"{name} {np.dtype(dtype).name} heads={H} k={k} d={d}: ok, worst |error| {worst:.2e}", flush=True)


if __name__ == "__main__":
    main()
