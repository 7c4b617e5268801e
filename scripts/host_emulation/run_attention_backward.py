#!/usr/bin/env python3
"""csr5_attention_bwd.hip on the CPU, without a GPU: the kernel source is compiled for the host against the stand-in for the HIP
runtime (fake/hip/hip_runtime.h) with -fsanitize=address,undefined, and run as a stand-alone program (attention_driver.cpp with
that one unit; emulation.py) on matrices of tests/zoo.py and their transposes, both converted by the oracle (the transpose plays
the transposed companion).

    python scripts/host_emulation/run_attention_backward.py [--matrices kat0,duplicates,...] [--kd 3x5,8x16] [--cxx clang++]

--matrices also takes class-edges and dealt of tests/attention_edges.py (a line on every class edge, hubs in every workgroup) and
NAME^T for the transpose of any matrix.

Per matrix, precision and (k, d): dQ, dK and dV against a float64 numpy reference (1e3 unit roundoffs of the gradient expression on
absolute values: a check of the indexing, not the accuracy test), rows and columns without entries exactly +0, nothing written
beyond column k or d, dQ alone without a workspace, and equal bits for sigma = 4, sigma = 7 with padded leading dimensions
(element loads, NaN in the padding) and sigma = 16 (16-byte loads); the companion is converted at another sigma than the parent.
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

KD = ((1, 1), (3, 5), (8, 16), (70, 40), (0, 7), (7, 0), (5, 300), (300, 5))
DEFAULT = "kat0,duplicates,aligned64,aligned1024,one-row,aligned64^T,aligned1024^T,one-row^T"
NAMES = ("dQ", "dK", "dV")


def reference(mat, Q, K, V, dO):
    """(dQ, dK, dV) and the same expressions on absolute values, in float64"""
    Q, K, V, dO = (t.astype(np.float64) for t in (Q, K, V, dO))
    rows = np.repeat(np.arange(mat.m), np.diff(mat.row_ptr))
    cols = mat.col[:mat.nnz].astype(np.int64)
    s = (Q[rows] * K[cols]).sum(1)
    mx = np.full(mat.m, -np.inf)
    np.maximum.at(mx, rows, s)
    w = np.exp(s - mx[rows])
    p = w / np.bincount(rows, w, mat.m)[rows]

    def scatter(idx, n, terms):
        out = np.zeros((n, terms.shape[1]))
        np.add.at(out, idx, terms)
        return out
    dp, adp = (dO[rows] * V[cols]).sum(1), (np.abs(dO[rows]) * np.abs(V[cols])).sum(1)
    ds = p * (dp - np.bincount(rows, p * dp, mat.m)[rows])
    ads = p * (adp + np.bincount(rows, p * adp, mat.m)[rows])
    got = scatter(rows, mat.m, ds[:, None] * K[cols]), scatter(cols, mat.n, ds[:, None] * Q[rows]), scatter(cols, mat.n, p[:, None] * dO[rows])
    mag = (scatter(rows, mat.m, ads[:, None] * np.abs(K[cols])), scatter(cols, mat.n, ads[:, None] * np.abs(Q[rows])),
           scatter(cols, mat.n, p[:, None] * np.abs(dO[rows])))
    return got, mag


def main():
    args = EMU.arguments(DEFAULT, kd=KD, kinds=None)
    orc = Oracle()
    mats = EMU.matrices()
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "attention_bwd_host")
        EMU.build(args.cxx, exe, ("attention_bwd",))
        for name in args.matrices:
            pat = EMU.Patterns(orc, mats(name))
            for dtype in (np.float64, np.float32):
                u = float(np.finfo(dtype).eps) / 2
                for k, d in args.kd:
                    ops = EMU.operands(pat.mat, 1, k, d, dtype)
                    ref, mag = reference(pat.mat, *(t[:, 0] for t in ops))
                    where = (name, np.dtype(dtype).name, k, d)

                    def backward(sigma, sigma_t, pad, groups, want=7):
                        return EMU.launch(exe, tmp, EMU.PLAIN, EMU.BACKWARD, pat, (sigma, sigma_t), ops, pad, want=want)[0]

                    def judge(i, g):
                        err = np.abs(g[:, 0] - ref[i])
                        return err <= 1e3 * u * np.maximum(mag[i], 1e-30) + 1e-300, float(err.max()) if err.size else 0.0
                    first, worst = EMU.check_configs(backward, NAMES, (pat.empty_r, pat.empty_c, pat.empty_c), where, judge)
                    EMU.check_same(backward(7, 4, True, 0, want=1), first, NAMES, where, "dQ alone")  # no workspace, no companion
                    print(f"{name} {np.dtype(dtype).name} k={k} d={d}: ok, worst |error| {worst:.2e}", flush=True)


if __name__ == "__main__":
    main()
