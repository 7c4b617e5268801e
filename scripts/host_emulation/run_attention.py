#!/usr/bin/env python3
"""csr5_attention.hip on the CPU, without a GPU: the kernel source is compiled for the host against a stand-in for the HIP runtime
(fake/hip/hip_runtime.h: 256 threads per workgroup, cross-lane operations emulated) with -fsanitize=address,undefined, and run as
a stand-alone program (attention_driver.cpp with that one unit; emulation.py) on matrices of tests/zoo.py converted by the oracle.

    python scripts/host_emulation/run_attention.py [--matrices kat0,duplicates,aligned64,aligned1024,one-row] [--cxx clang++]

--matrices also takes class-edges and dealt of tests/attention_edges.py (a line on every class edge, hubs in every workgroup) and
NAME^T for the transpose of any of them.

Per matrix, precision and (k, d): O against a float64 numpy reference (1e3 unit roundoffs of the largest |V| sum: a check of the
indexing, not the accuracy test), rows without entries exactly +0, nothing written beyond column d, and equal bits for sigma = 4,
sigma = 7 with padded leading dimensions (element loads, NaN in the padding) and sigma = 16 (16-byte loads).  This exercises the
indexing, the row classes and the arithmetic of the source; it says nothing about the gfx950 build."""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle.csr5_oracle import Oracle  # noqa: E402
from scripts.host_emulation import emulation as EMU  # noqa: E402

KD = ((1, 1), (3, 5), (8, 16), (40, 70), (0, 7), (5, 300))
DEFAULT = "kat0,duplicates,aligned64,aligned1024,one-row"


def reference(mat, Q, K, V):
    Q, K, V = (t.astype(np.float64) for t in (Q, K, V))
    out, scale = np.zeros((mat.m, V.shape[1])), 1.0
    for i in range(mat.m):
        a, b = mat.row_ptr[i], mat.row_ptr[i + 1]
        if b > a:
            c = mat.col[a:b]
            s = K[c] @ Q[i]
            w = np.exp(s - s.max())
            out[i] = (w[:, None] * V[c]).sum(0) / w.sum()
            scale = max(scale, float(np.abs(s).max()))
    return out, scale


def main():
    args = EMU.arguments(DEFAULT, kinds=None)
    orc = Oracle()
    mats = EMU.matrices()
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "attention_host")
        EMU.build(args.cxx, exe, ("attention",))
        for name in args.matrices:
            pat = EMU.Patterns(orc, mats(name), companion=False)
            for dtype in (np.float64, np.float32):
                u = float(np.finfo(dtype).eps) / 2
                for k, d in KD:
                    Q, K, V, _ = EMU.operands(pat.mat, 1, k, d, dtype)
                    ref, scale = reference(pat.mat, Q[:, 0], K[:, 0], V[:, 0])

                    def both(sigma, sigma_t, pad, groups):
                        return [EMU.launch(exe, tmp, EMU.PLAIN, EMU.FORWARD, pat, (sigma, sigma_t), (Q, K, V), pad)]

                    def judge(i, g):
                        err = EMU.worst_of(g[:, 0], ref)
                        return np.array(err <= 1e3 * u * scale), err
                    _, worst = EMU.check_configs(both, ("O",), (pat.empty_r,), (name, np.dtype(dtype).name, k, d), judge)
                    print(f"{name} {np.dtype(dtype).name} k={k} d={d}: ok, worst |error| {worst:.2e}", flush=True)


if __name__ == "__main__":
    main()
