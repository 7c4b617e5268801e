#!/usr/bin/env python3
"""The multi-head entries of csr5_attention.hip and csr5_attention_bwd.hip on the CPU, without a GPU: the kernel sources are
compiled for the host against the stand-in for the HIP runtime (fake/hip/hip_runtime.h) with -fsanitize=address,undefined, and run
as a stand-alone program (attention_driver.cpp with those two units; emulation.py) on matrices of tests/zoo.py converted by the
oracle; for the backward the transpose, converted at another sigma, plays the transposed companion.

    python scripts/host_emulation/run_mha.py [--matrices kat0,duplicates,aligned64,aligned1024,one-row] [--dtypes f64,f32]
                                             [--heads 1,3] [--kd 3x5,8x16,5x300] [--cxx clang++]

--matrices also takes class-edges and dealt of tests/attention_edges.py (a line on every class edge, hubs in every workgroup) and
NAME^T for the transpose of any matrix.

Per matrix, precision, heads in {1, 3} and (k, d) in {(3, 5), (8, 16), (5, 300)}, forward and backward:
  * head h of the packed call has the same bits as the SINGLE-HEAD launcher on that head's slices of the same arrays (the driver's
    offk / offd: pointers that start inside the packed rows, heads = 1);
  * nothing is written beyond column heads * d (heads * k) of an output, and nothing at all into an output that is not wanted;
  * equal bits for sigma = 4 with the head groups of the rule, sigma = 7 with padded leading dimensions (element loads, NaN in the
    padding) and ONE group (all heads in one workgroup), and sigma = 16 with one group (16-byte loads where the slices allow them);
  * backward: dQ alone, without workspace and companion, has the bits it has with them.
Every array is an exact-size heap block (the workspace exactly 4 m heads values).  This exercises the indexing, the head loop in
the three row classes and the arithmetic of the source; it says nothing about the gfx950 build."""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle.csr5_oracle import Oracle  # noqa: E402
from scripts.host_emulation import emulation as EMU  # noqa: E402

DEFAULT = "kat0,duplicates,aligned64,aligned1024,one-row"
HEADS = (1, 3)
KD = ((3, 5), (8, 16), (5, 300))
NAMES = ("O", "dQ", "dK", "dV")


def main():
    args = EMU.arguments(DEFAULT, HEADS, KD)
    orc = Oracle()
    mats = EMU.matrices()
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "mha_host")
        EMU.build(args.cxx, exe, ("attention", "attention_bwd"))
        for name in args.matrices:
            pat = EMU.Patterns(orc, mats(name))
            for dtype in args.dtypes:
                for H in args.heads:
                    for k, d in args.kd:
                        ops = EMU.operands(pat.mat, H, k, d, dtype)
                        where = (name, H, k, d)

                        def both(sigma, sigma_t, pad, groups, want=None, single=None):
                            O = None if want else EMU.launch(exe, tmp, EMU.PLAIN, EMU.FORWARD, pat, (sigma, sigma_t), ops[:3], pad, groups,
                                                             single=single)
                            return [O] + EMU.launch(exe, tmp, EMU.PLAIN, EMU.BACKWARD, pat, (sigma, sigma_t), ops, pad, groups, want,
                                                    single=single)[0]
                        first, _ = EMU.check_configs(both, NAMES, (None,) * 4, where)
                        for h in range(H):  # the single-head launcher on head h's slices of the same packed arrays
                            one = [g[:, h] for g in both(7, 4, True, 0, single=h)]
                            EMU.check_same(one, [g[:, h] for g in first], NAMES, where + (h,), "against the single-head call")
                        EMU.check_same(both(7, 4, True, 1, want=1), first, NAMES, where, "dQ alone")
                        print(f"{name} {np.dtype(dtype).name} heads={H} k={k} d={d}: ok", flush=True)


if __name__ == "__main__":
    main()
