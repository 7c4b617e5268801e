#!/usr/bin/env python3
"""The biased multi-head entries (csr5_attention_bias.hip, csr5_attention_bwd_bias.hip) on the CPU, without a GPU: the kernel
sources are compiled for the host against the stand-in for the HIP runtime (fake/hip/hip_runtime.h) with
-fsanitize=address,undefined, and run as stand-alone programs (mha_bias_main.cpp, mha_bias_bwd_main.cpp) on matrices of
tests/zoo.py converted by the oracle WITH THEIR VALUES; for the backward the transpose, converted at another sigma with the
values in its own order, plays the transposed companion.

    python scripts/host_emulation/run_mha_bias.py [--matrices kat0,one-row,duplicates,aligned64,aligned1024,class-edges,class-edges^T,dealt]
                                                  [--dtypes f64,f32] [--heads 1,3] [--kd 3x5,8x16,12x8] [--skip kat0:12x8] [--cxx clang++]

EVERY ENTRY'S VALUE IS DISTINCT (a permutation of nnz equidistant values in [-2, 2)), so a value taken from another entry's
position -- in a moved tile, a fast-track tile, the CSR tail, a recompute sweep or on the column side -- is an error of order one.

Per matrix, precision, heads and (k, d), with scale 0.37 and a slope per head:
  * O, dQ, dK, dV and dS against a numpy float64 reference of softmax(scale Q K^T + slope_h A) (1e3 unit roundoffs of the
    expression on absolute values, times one plus the largest score magnitude: a check of the indexing, not the accuracy test);
  * rows and columns without entries exactly +0, nothing written beyond the last column of an output (dS: beyond column
    heads - 1 of its rows of ldds values), nothing at all into an output that is not wanted;
  * equal bits for sigma = 4 with the head groups of the rule, sigma = 7 with padded leading dimensions (element loads, dS with
    ldds = heads + 2) and ONE group, and sigma = 16 with one group (16-byte loads where the slices allow them);
  * without slopes: the bits of slopes that are all one;
  * dQ and dS alone, without workspace and companion, have the bits they have with them.
The shapes --kd is used with (SHAPES; any KxD is taken): (3, 5) element loads everywhere; (8, 16) and (12, 8) 16-byte loads where
the configuration's leading dimensions allow them, with one head and with three (8, 12 and 16 values are a multiple of 16 bytes in
either type, so every head's slice of every row is aligned); at 12 the fp32 chain is one block of 8 by 16-byte loads and 4
elements.  (12, 8) is the shape tests/test_mha_bias_host.py runs under the sanitizers and tests/test_gpu_mha_bias_edges.py on the
GPU.  The default is the first two.  --skip leaves (matrix, shape) pairs out of one run.
Every array is an exact-size heap block.  This exercises the indexing, the row classes and the arithmetic of the source; it says
nothing about the gfx950 build."""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from benchmark_spmv_using_csr5_amd import matrices as M  # noqa: E402
from oracle.csr5_oracle import Oracle  # noqa: E402
from scripts.host_emulation.run_attention_backward import matrices  # noqa: E402
from scripts.host_emulation.run_mha import build, same, wide  # noqa: E402

DEFAULT = "kat0,one-row,duplicates,aligned64,aligned1024,class-edges,class-edges^T,dealt"
HEADS = (1, 3)
KD = ((3, 5), (8, 16))
SHAPES = KD + ((12, 8),)
CONFIGS = ((4, 16, False, 0), (7, 4, True, 1), (16, 7, False, 1))  # sigma, the companion's sigma, padded, head groups (0: the rule)
SCALE = 0.37


def transpose_with_values(mat, val):
    """A^T in CSR with every column's entries in A's CSR order (a stable sort by column), and the values in that order"""
    rows = np.repeat(np.arange(mat.m, dtype=np.int64), np.diff(mat.row_ptr))
    cols = mat.col[:mat.nnz].astype(np.int64)
    order = np.argsort(cols, kind="stable")
    rp = np.zeros(mat.n + 1, dtype=np.int32)
    rp[1:] = np.cumsum(np.bincount(cols, minlength=mat.n))
    return M.CsrMatrix(mat.n, mat.m, rp, rows[order].astype(np.int32), np.ones(mat.nnz), mat.name + "^T"), val[order]


def execute(exe, tmp, header, scale, patterns, dtype, slopes, operands, name):
    case, out = os.path.join(tmp, "case.bin"), os.path.join(tmp, "out.bin")
    with open(case, "wb") as f:
        np.array(header, dtype=np.int32).tofile(f)
        np.array([scale], dtype=np.float64).tofile(f)
        for mat, fmt in patterns:
            mat.row_ptr.astype(np.int32).tofile(f)
            fmt.col[:mat.nnz].astype(np.int32).tofile(f)
            fmt.tile_ptr.astype(np.uint32).tofile(f)
            fmt.val[:mat.nnz].astype(dtype).tofile(f)
        slopes.astype(dtype).tofile(f)
        for t in operands:
            t.tofile(f)
    r = subprocess.run([exe, case, out], capture_output=True, text=True)
    if r.returncode:
        raise SystemExit(f"{name}: exit {r.returncode}\n{r.stderr[-4000:]}")
    return out


def forward(exe, tmp, fmt, mat, sigma, slopes, use_slopes, Q, K, V, pad, groups):
    dtype, (_, H, k), d = Q.dtype, Q.shape, V.shape[2]
    ldq, ldk, ldv, ldo = (H * k + 3, H * k + 1, H * d + 2, H * d + 3) if pad else (H * k, H * k, H * d, H * d)
    header = [mat.m, mat.n, mat.nnz, sigma, fmt.p, k, d, ldq, ldk, ldv, ldo, int(dtype == np.float64), H, groups, int(use_slopes)]
    out = execute(exe, tmp, header, SCALE, ((mat, fmt),), dtype, slopes, (wide(Q, ldq), wide(K, ldk), wide(V, ldv)),
                  f"{mat.name} sigma {sigma}")
    O = np.fromfile(out, dtype=dtype).reshape(mat.m, ldo)
    assert np.isnan(O[:, H * d:]).all(), "written beyond column heads * d"
    return np.ascontiguousarray(O[:, :H * d]).reshape(mat.m, H, d)


def backward(exe, tmp, fmts, mats, sigmas, slopes, use_slopes, Q, K, V, dO, pad, groups, want=15):
    """[dQ, dK, dV, dS] (None where not wanted)"""
    dtype, (_, H, k), d = Q.dtype, Q.shape, V.shape[2]
    wk, wd = H * k, H * d
    lds = (wk + 3, wk + 1, wd + 2, wd + 3, wk + 1, wk + 2, wd + 1) if pad else (wk, wk, wd, wd, wk, wk, wd)
    ldds = H + 2 if pad else H
    mat, matT = mats
    header = [mat.m, mat.n, mat.nnz, sigmas[0], fmts[0].p, sigmas[1], fmts[1].p, k, d, *lds, int(dtype == np.float64), want, H, groups,
              int(use_slopes), ldds]
    out = execute(exe, tmp, header, SCALE, zip(mats, fmts), dtype, slopes, [wide(t, ld) for t, ld in zip((Q, K, V, dO), lds[:4])],
                  f"{mat.name} sigma {sigmas}")
    flat = np.fromfile(out, dtype=dtype)
    res, at = [], 0
    for bit, rows, ld, width in ((1, mat.m, lds[4], wk), (2, mat.n, lds[5], wk), (4, mat.n, lds[6], wd), (8, mat.nnz, ldds, H)):
        g = flat[at:at + rows * ld].reshape(rows, ld)
        at += rows * ld
        assert np.isnan(g[:, width:]).all(), "written beyond the last column"
        if want & bit:
            res.append(np.ascontiguousarray(g[:, :width]).reshape((rows, H, width // H) if bit != 8 else (rows, H)))
        else:
            assert np.isnan(g).all(), "an output that was not wanted is written"
            res.append(None)
    return res


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
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrices", default=DEFAULT)
    ap.add_argument("--dtypes", default="f64,f32")
    ap.add_argument("--heads", default=",".join(str(h) for h in HEADS))
    ap.add_argument("--kd", default=",".join(f"{k}x{d}" for k, d in KD), help="a subset lets the slow cases run side by side")
    ap.add_argument("--skip", default="", help="NAME:KxD pairs to leave out, separated by commas")
    ap.add_argument("--cxx", default="/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else "clang++")
    args = ap.parse_args()
    dtypes = [{"f64": np.float64, "f32": np.float32}[t] for t in args.dtypes.split(",")]
    heads = [int(h) for h in args.heads.split(",")]
    kds = [tuple(int(v) for v in kd.split("x")) for kd in args.kd.split(",")]
    skip = {tuple(pair.split(":")) for pair in args.skip.split(",") if pair}
    orc = Oracle()
    mats = matrices()
    with tempfile.TemporaryDirectory() as tmp:
        fwd, bwd = os.path.join(tmp, "mha_bias_host"), os.path.join(tmp, "mha_bias_bwd_host")
        build(args.cxx, "mha_bias_main.cpp", fwd)
        build(args.cxx, "mha_bias_bwd_main.cpp", bwd)
        for name in args.matrices.split(","):
            mat = mats(name)
            val = (np.random.default_rng(11).permutation(mat.nnz) / max(mat.nnz, 1) * 4 - 2).astype(np.float64)  # distinct, also in fp32
            assert len(np.unique(val.astype(np.float32))) == mat.nnz
            matT, valT = transpose_with_values(mat, val)
            conv = {s: orc.convert(64, s, mat.m, mat.row_ptr, mat.col, val) for s in (4, 7, 16)}
            convT = {s: orc.convert(64, s, matT.m, matT.row_ptr, matT.col, valT) for s in (4, 7, 16)}
            empty_r, empty_c = np.diff(mat.row_ptr) == 0, np.diff(matT.row_ptr) == 0
            for dtype in dtypes:
                u = float(np.finfo(dtype).eps) / 2
                for H in heads:
                    for k, d in kds:
                        if (name, f"{k}x{d}") in skip:
                            continue
                        rng = np.random.default_rng(5)
                        Q = (rng.uniform(-1, 1, (mat.m, H, k)) * 2).astype(dtype)
                        K = rng.uniform(-1, 1, (mat.n, H, k)).astype(dtype)
                        V = rng.uniform(-1, 1, (mat.n, H, d)).astype(dtype)
                        dO = rng.uniform(-1, 1, (mat.m, H, d)).astype(dtype)
                        slopes = np.array([1.5, -0.75, 0.3125][:H], dtype=dtype)
                        ref, mag, smag = reference(mat, val.astype(dtype), slopes, Q, K, V, dO)
                        first, worst = None, 0.0
                        for sigma, sigma_t, pad, groups in CONFIGS:
                            O = forward(fwd, tmp, conv[sigma], mat, sigma, slopes, True, Q, K, V, pad, groups)
                            G = backward(bwd, tmp, (conv[sigma], convT[sigma_t]), (mat, matT), (sigma, sigma_t), slopes, True, Q, K, V, dO,
                                         pad, groups)
                            got = [O] + G
                            for g, r, a, e, what in zip(got, ref, mag, (empty_r, empty_r, empty_c, empty_c, None),
                                                        ("O", "dQ", "dK", "dV", "dS")):
                                assert not np.isnan(g).any(), (name, H, k, d, sigma, what, "unwritten")
                                err = np.abs(g - r)
                                ok = err <= 1e3 * u * (1 + smag) * np.maximum(a, 1e-30) + 1e-300
                                assert ok.all(), (name, np.dtype(dtype).name, H, k, d, sigma, what, float(err.max()))
                                worst = max(worst, float(err.max()) if err.size else 0.0)
                                if e is not None:
                                    assert not np.ascontiguousarray(g[e]).view(np.uint8).any(), f"{what}: a line without entries is not +0"
                            first = got if first is None else first
                            for g, g0, what in zip(got, first, ("O", "dQ", "dK", "dV", "dS")):
                                assert same(g, g0), (name, H, k, d, sigma, what, "bits")
                        ones = np.ones(H, dtype=dtype)
                        with_ones = [forward(fwd, tmp, conv[7], mat, 7, ones, True, Q, K, V, True, 0)] + \
                            backward(bwd, tmp, (conv[7], convT[4]), (mat, matT), (7, 4), ones, True, Q, K, V, dO, True, 0)
                        without = [forward(fwd, tmp, conv[7], mat, 7, ones, False, Q, K, V, True, 0)] + \
                            backward(bwd, tmp, (conv[7], convT[4]), (mat, matT), (7, 4), ones, False, Q, K, V, dO, True, 0)
                        for g, g0, what in zip(without, with_ones, ("O", "dQ", "dK", "dV", "dS")):
                            assert same(g, g0), (name, H, k, d, what, "no slopes against slopes of one")
                        alone = backward(bwd, tmp, (conv[7], convT[4]), (mat, matT), (7, 4), slopes, True, Q, K, V, dO, True, 1, want=9)
                        assert same(alone[0], first[1]) and same(alone[3], first[4]), (name, H, k, d, "dQ and dS alone")
                        print(f"{name} {np.dtype(dtype).name} heads={H} k={k} d={d}: ok, worst |error| {worst:.2e}", flush=True)


if __name__ == "__main__":
    main()
