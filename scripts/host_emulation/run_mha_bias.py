#!/usr/bin/env python3
"""The biased multi-head entries (csr5_attention_bias.hip, csr5_attention_bwd_bias.hip) on the CPU, without a GPU: the kernel
sources are compiled for the host against the stand-in for the HIP runtime (fake/hip/hip_runtime.h) with
-fsanitize=address,undefined, and run as a stand-alone program (attention_driver.cpp with those two units; emulation.py) on
matrices of tests/zoo.py converted by the oracle WITH THEIR VALUES; for the backward the transpose, converted at another sigma
with the values in its own order, plays the transposed companion.

    python scripts/host_emulation/run_mha_bias.py [--matrices kat0,one-row,duplicates,aligned64,aligned1024,class-edges,class-edges^T,dealt]
                                                  [--dtypes f64,f32] [--heads 1,3] [--kd 3x5,8x16,12x8] [--skip kat0:12x8] [--cxx clang++]

EVERY ENTRY'S VALUE IS DISTINCT (a permutation of nnz equidistant values in [-2, 2)), so a value taken from another entry's
position -- in a moved tile, a fast-track tile, the CSR tail, a recompute sweep or on the column side -- is an error of order one.

Per matrix, precision, heads and (k, d), with scale 0.37 and a slope per head:
  * O, dQ, dK, dV and dS against a numpy float64 reference of softmax(scale Q K^T + slope_h A) (1e3 unit roundoffs of the
    expression on absolute values, times one plus the largest score magnitude: a check of the indexing, not the accuracy test);
  * rows and columns without entries exactly +0, nothing written beyond the last column of an output (dS: beyond column
    heads - 1 of its rows of ldds values), nothing at all into an output that is not wanted;
  * equal bits for sigma = 4 with the head groups of the rule, sigma = 7 with padded leading dimensions (element loads, NaN in the
    padding, dS with ldds = heads + 2) and ONE group, and sigma = 16 with one group (16-byte loads where the slices allow them);
  * without slopes: the bits of slopes that are all one;
  * dQ and dS alone, without workspace and companion, have the bits they have with them.
The shapes --kd is used with (SHAPES; any KxD is taken): (3, 5) element loads everywhere; (8, 16) and (12, 8) 16-byte loads where
the configuration's leading dimensions allow them, with one head and with three (8, 12 and 16 values are a multiple of 16 bytes in
either type, so every head's slice of every row is aligned); at 12 the fp32 chain is one block of 8 by 16-byte loads and 4
elements.  (12, 8) is the shape tests/test_mha_bias_host.py runs under the sanitizers and tests/test_gpu_mha_bias_edges.py on the
GPU.  The default is the first two.  --skip leaves (matrix, shape) pairs out of one run.
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
SHAPES = KD + ((12, 8),)
SCALE = EMU.SCALE
NAMES = ("O", "dQ", "dK", "dV", "dS")


def reference(mat, val, slopes, Q, K, V, dO):
    """(O, dQ, dK, dV, dS), the same expressions on absolute values, and the largest score magnitude, in float64"""
    Q, K, V, dO, val, slopes = (t.astype(np.float64) for t in (Q, K, V, dO, val, slopes))
    rows = np.repeat(np.arange(mat.m), np.diff(mat.row_ptr))
    cols = mat.col[:mat.nnz].astype(np.int64)
    H = Q.shape[1]

    def scatter(idx, n, terms):
        out = np.zeros((n,) + terms.shape[1:])
        np.add.at(out, idx, terms)
        return out
    s = SCALE * (Q[rows] * K[cols]).sum(2) + slopes[None, :] * val[:, None]                       # (nnz, H)
    smag = float((SCALE * (np.abs(Q[rows]) * np.abs(K[cols])).sum(2) + np.abs(slopes[None, :] * val[:, None])).max()) if mat.nnz else 0.0
    mx = np.full((mat.m, H), -np.inf)
    np.maximum.at(mx, rows, s)
    w = np.exp(s - mx[rows])
    p = w / scatter(rows, mat.m, w)[rows]
    dp, adp = (dO[rows] * V[cols]).sum(2), (np.abs(dO[rows]) * np.abs(V[cols])).sum(2)
    ds = p * (dp - scatter(rows, mat.m, p * dp)[rows])
    ads = p * (adp + scatter(rows, mat.m, p * adp)[rows])
    got = (scatter(rows, mat.m, p[:, :, None] * V[cols]), SCALE * scatter(rows, mat.m, ds[:, :, None] * K[cols]),
           SCALE * scatter(cols, mat.n, ds[:, :, None] * Q[rows]), scatter(cols, mat.n, p[:, :, None] * dO[rows]), ds)
    mag = (scatter(rows, mat.m, p[:, :, None] * np.abs(V[cols])), SCALE * scatter(rows, mat.m, ads[:, :, None] * np.abs(K[cols])),
           SCALE * scatter(cols, mat.n, ads[:, :, None] * np.abs(Q[rows])), scatter(cols, mat.n, p[:, :, None] * np.abs(dO[rows])), ads)
    return got, mag, smag


def main():
    args = EMU.arguments(DEFAULT, HEADS, KD, extra=(("--skip", dict(default="", help="NAME:KxD pairs to leave out, separated by commas")),))
    skip = {tuple(pair.split(":")) for pair in args.skip.split(",") if pair}
    orc = Oracle()
    mats = EMU.matrices()
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "mha_bias_host")
        EMU.build(args.cxx, exe, ("attention_bias", "attention_bwd_bias"))
        for name in args.matrices:
            mat = mats(name)
            val = (np.random.default_rng(11).permutation(mat.nnz) / max(mat.nnz, 1) * 4 - 2).astype(np.float64)  # distinct, also in fp32
            assert len(np.unique(val.astype(np.float32))) == mat.nnz
            pat = EMU.Patterns(orc, mat, val)
            empties = (pat.empty_r, pat.empty_r, pat.empty_c, pat.empty_c, None)
            for dtype in args.dtypes:
                u = float(np.finfo(dtype).eps) / 2
                for H in args.heads:
                    for k, d in args.kd:
                        if (name, f"{k}x{d}") in skip:
                            continue
                        ops = EMU.operands(mat, H, k, d, dtype)
                        slopes = np.array([1.5, -0.75, 0.3125][:H], dtype=dtype)
                        ref, mag, smag = reference(mat, val.astype(dtype), slopes, *ops)
                        where = (name, np.dtype(dtype).name, H, k, d)

                        def both(sigma, sigma_t, pad, groups, want=None, slopes=slopes):
                            common = dict(slopes=slopes, values=True, scalars=(SCALE, 0.0, 0.0, 0, 0), pads=dict(lddb=2))
                            O = None if want else EMU.launch(exe, tmp, EMU.BIASED, EMU.FORWARD, pat, (sigma, sigma_t), ops[:3], pad, groups,
                                                             **common)
                            return [O] + EMU.launch(exe, tmp, EMU.BIASED, EMU.BACKWARD, pat, (sigma, sigma_t), ops, pad, groups, want,
                                                    **common)[0]

                        def judge(i, g):
                            return EMU.within(g, ref[i], mag[i], smag, u), EMU.worst_of(g, ref[i])
                        first, worst = EMU.check_configs(both, NAMES, empties, where, judge)
                        EMU.check_same(both(7, 4, True, 0, slopes=None), both(7, 4, True, 0, slopes=np.ones(H, dtype=dtype)), NAMES, where,
                                       "no slopes against slopes of one")
                        EMU.check_same(both(7, 4, True, 1, want=9), first, NAMES, where, "dQ and dS alone")
                        print(f"{name} {np.dtype(dtype).name} heads={H} k={k} d={d}: ok, worst |error| {worst:.2e}", flush=True)


if __name__ == "__main__":
    main()
