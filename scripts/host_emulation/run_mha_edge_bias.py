#!/usr/bin/env python3
"""The edge-bias multi-head entries (csr5_attention_edge.hip, csr5_attention_bwd_edge.hip) on the CPU, without a GPU: the kernel
sources are compiled for the host against the stand-in for the HIP runtime (fake/hip/hip_runtime.h) with
-fsanitize=address,undefined, and run as stand-alone programs (mha_edge_main.cpp, mha_edge_bwd_main.cpp) on matrices of
tests/zoo.py converted by the oracle; for the backward the transpose, converted at another sigma, plays the transposed companion
and the stable sort by column that forms it is the source map.  THE PATTERNS CARRY NO VALUE ARRAY AT ALL (null pointers).

    python scripts/host_emulation/run_mha_edge_bias.py [--matrices kat0,one-row,duplicates,aligned64,aligned1024,class-edges,class-edges^T,dealt]
                                                       [--dtypes f64,f32] [--heads 1,3] [--kd 3x5,8x16] [--cxx clang++]

EVERY (ENTRY, HEAD) HAS A DISTINCT BIAS (a permutation of nnz heads equidistant values in [-2, 2)), so a bias taken from another
entry or another head -- at a wrong rank, without the map on the column side, with a wrong row stride -- is an error of order one;
AND B, dB AND THE MAP ARE HEAP BLOCKS OF EXACTLY nnz ldb, nnz lddb AND nnz ELEMENTS, so an index beyond them is an out-of-bounds
access the address sanitizer reports.  The padding columns of B hold NaN: reading one poisons a row.

Per matrix, precision, heads and (k, d), with scale 0.37:
  * O, dQ, dK, dV and dB against a numpy float64 reference of softmax(scale Q K^T + B) (``reference``; ``within``: 1e3 unit
    roundoffs of the expression on absolute values, times one plus the largest score magnitude: a check of the indexing, not the
    accuracy test);
  * rows and columns without entries exactly +0, nothing written beyond the last column of an output (dB: beyond column
    heads - 1 of its rows of lddb values), nothing at all into an output that is not wanted;
  * equal bits for sigma = 4 with the head groups of the rule and ldb = lddb = heads, sigma = 7 with padded leading dimensions
    (ldb = heads + 2, lddb = heads + 3) and ONE group, and sigma = 16 with one group;
  * a null B has the bits of a B of +0;
  * dQ and dB alone, without workspace, companion and map, have the bits they have with them.
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
CONFIGS = ((4, 16, False, 0), (7, 4, True, 1), (16, 7, False, 1))  # sigma, the companion's sigma, padded, head groups (0: the rule)
SCALE = 0.37
NAMES = ("O", "dQ", "dK", "dV", "dB")


def transpose_with_map(mat):
    """A^T in CSR with every column's entries in A's CSR order (a stable sort by column), and that sort: position in A^T's CSR ->
    position in A's CSR, the companion's source map"""
    rows = np.repeat(np.arange(mat.m, dtype=np.int64), np.diff(mat.row_ptr))
    cols = mat.col[:mat.nnz].astype(np.int64)
    order = np.argsort(cols, kind="stable")
    rp = np.zeros(mat.n + 1, dtype=np.int32)
    rp[1:] = np.cumsum(np.bincount(cols, minlength=mat.n))
    return M.CsrMatrix(mat.n, mat.m, rp, rows[order].astype(np.int32), np.ones(mat.nnz), mat.name + "^T"), order.astype(np.uint32)


def distinct_bias(nnz, H, seed=11):
    """(nnz, H) float64: a permutation of nnz H equidistant values in [-2, 2), distinct also in fp32"""
    B = (np.random.default_rng(seed).permutation(nnz * H) / max(nnz * H, 1) * 4 - 2).reshape(nnz, H)
    assert len(np.unique(B.astype(np.float32))) == nnz * H
    return B


def wide_bias(B, ldb, fill=np.nan):
    """(nnz, H) in rows of ldb values, EXACTLY nnz ldb elements, the padding columns `fill`"""
    w = np.full((B.shape[0], ldb), fill, dtype=B.dtype)
    w[:, :B.shape[1]] = B
    return w


def execute(exe, tmp, header, scale, patterns, arrays, name):
    case, out = os.path.join(tmp, "case.bin"), os.path.join(tmp, "out.bin")
    with open(case, "wb") as f:
        np.array(header, dtype=np.int32).tofile(f)
        np.array([scale], dtype=np.float64).tofile(f)
        for mat, fmt in patterns:
            mat.row_ptr.astype(np.int32).tofile(f)
            fmt.col[:mat.nnz].astype(np.int32).tofile(f)
            fmt.tile_ptr.astype(np.uint32).tofile(f)
        for t in arrays:
            t.tofile(f)
    r = subprocess.run([exe, case, out], capture_output=True, text=True)
    if r.returncode:
        raise SystemExit(f"{name}: exit {r.returncode}\n{r.stderr[-4000:]}")
    return out


def forward(exe, tmp, fmt, mat, sigma, B, use_b, Q, K, V, pad, groups):
    dtype, (_, H, k), d = Q.dtype, Q.shape, V.shape[2]
    ldq, ldk, ldv, ldo = (H * k + 3, H * k + 1, H * d + 2, H * d + 3) if pad else (H * k, H * k, H * d, H * d)
    ldb = H + 2 if pad else H
    header = [mat.m, mat.n, mat.nnz, sigma, fmt.p, k, d, ldq, ldk, ldv, ldo, int(dtype == np.float64), H, groups, int(use_b), ldb]
    out = execute(exe, tmp, header, SCALE, ((mat, fmt),), (wide_bias(B.astype(dtype), ldb), wide(Q, ldq), wide(K, ldk), wide(V, ldv)),
                  f"{mat.name} sigma {sigma}")
    O = np.fromfile(out, dtype=dtype).reshape(mat.m, ldo)
    assert np.isnan(O[:, H * d:]).all(), "written beyond column heads * d"
    return np.ascontiguousarray(O[:, :H * d]).reshape(mat.m, H, d)


def backward(exe, tmp, fmts, mats, sigmas, amap, B, use_b, Q, K, V, dO, pad, groups, want=15):
    """[dQ, dK, dV, dB] (None where not wanted)"""
    dtype, (_, H, k), d = Q.dtype, Q.shape, V.shape[2]
    wk, wd = H * k, H * d
    lds = (wk + 3, wk + 1, wd + 2, wd + 3, wk + 1, wk + 2, wd + 1) if pad else (wk, wk, wd, wd, wk, wk, wd)
    ldb, lddb = (H + 2, H + 3) if pad else (H, H)
    mat, matT = mats
    header = [mat.m, mat.n, mat.nnz, sigmas[0], fmts[0].p, sigmas[1], fmts[1].p, k, d, *lds, int(dtype == np.float64), want, H, groups,
              int(use_b), ldb, lddb]
    arrays = [amap.astype(np.uint32), wide_bias(B.astype(dtype), ldb)] + [wide(t, ld) for t, ld in zip((Q, K, V, dO), lds[:4])]
    out = execute(exe, tmp, header, SCALE, zip(mats, fmts), arrays, f"{mat.name} sigma {sigmas}")
    flat = np.fromfile(out, dtype=dtype)
    res, at = [], 0
    for bit, rows, ld, width in ((1, mat.m, lds[4], wk), (2, mat.n, lds[5], wk), (4, mat.n, lds[6], wd), (8, mat.nnz, lddb, H)):
        g = flat[at:at + rows * ld].reshape(rows, ld)
        at += rows * ld
        assert np.isnan(g[:, width:]).all(), "written beyond the last column"
        if want & bit:
            res.append(np.ascontiguousarray(g[:, :width]).reshape((rows, H, width // H) if bit != 8 else (rows, H)))
        else:
            assert np.isnan(g).all(), "an output that was not wanted is written"
            res.append(None)
    return res


def reference(mat, B, Q, K, V, dO, B_col=None):
    """(O, dQ, dK, dV, dB), the same expressions on absolute values, and the largest score magnitude, in float64.  B (nnz, H) in
    CSR order.  B_col: the bias the COLUMN side (dK, dV) computes its scores with, when a wrong kernel is modelled whose two sides
    disagree; None for B."""
    Q, K, V, dO, B = (t.astype(np.float64) for t in (Q, K, V, dO, B))
    rows = np.repeat(np.arange(mat.m), np.diff(mat.row_ptr))
    cols = mat.col[:mat.nnz].astype(np.int64)
    H = Q.shape[1]

    def scatter(idx, n, terms):
        out = np.zeros((n,) + terms.shape[1:])
        np.add.at(out, idx, terms)
        return out

    def side(bias):
        s = SCALE * (Q[rows] * K[cols]).sum(2) + bias                                              # (nnz, H)
        mx = np.full((mat.m, H), -np.inf)
        np.maximum.at(mx, rows, s)
        w = np.exp(s - mx[rows])
        p = w / scatter(rows, mat.m, w)[rows]
        dp, adp = (dO[rows] * V[cols]).sum(2), (np.abs(dO[rows]) * np.abs(V[cols])).sum(2)
        ds = p * (dp - scatter(rows, mat.m, p * dp)[rows])
        ads = p * (adp + scatter(rows, mat.m, p * adp)[rows])
        return p, ds, ads
    smag = float((SCALE * (np.abs(Q[rows]) * np.abs(K[cols])).sum(2) + np.abs(B)).max()) if mat.nnz else 0.0
    p, ds, ads = side(B)
    if B_col is None:
        pc, dsc, adsc = p, ds, ads
    else:  # (the workspace of the row side -- M, r, D -- with the column side's scores: modelled as that side's own softmax)
        pc, dsc, adsc = side(B_col.astype(np.float64))
    got = (scatter(rows, mat.m, p[:, :, None] * V[cols]), SCALE * scatter(rows, mat.m, ds[:, :, None] * K[cols]),
           SCALE * scatter(cols, mat.n, dsc[:, :, None] * Q[rows]), scatter(cols, mat.n, pc[:, :, None] * dO[rows]), ds)
    mag = (scatter(rows, mat.m, p[:, :, None] * np.abs(V[cols])), SCALE * scatter(rows, mat.m, ads[:, :, None] * np.abs(K[cols])),
           SCALE * scatter(cols, mat.n, adsc[:, :, None] * np.abs(Q[rows])), scatter(cols, mat.n, pc[:, :, None] * np.abs(dO[rows])), ads)
    return got, mag, smag


def within(g, r, a, smag, u):
    """elementwise: |g - r| inside the bound of the docstring (NaN is outside)"""
    return np.abs(g - r) <= 1e3 * u * (1 + smag) * np.maximum(a, 1e-30) + 1e-300


def operands(mat, H, k, d, dtype):
    rng = np.random.default_rng(5)
    Q = (rng.uniform(-1, 1, (mat.m, H, k)) * 2).astype(dtype)
    K = rng.uniform(-1, 1, (mat.n, H, k)).astype(dtype)
    V = rng.uniform(-1, 1, (mat.n, H, d)).astype(dtype)
    dO = rng.uniform(-1, 1, (mat.m, H, d)).astype(dtype)
    return Q, K, V, dO


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrices", default=DEFAULT)
    ap.add_argument("--dtypes", default="f64,f32")
    ap.add_argument("--heads", default=",".join(str(h) for h in HEADS))
    ap.add_argument("--kd", default=",".join(f"{k}x{d}" for k, d in KD), help="a subset lets the slow cases run side by side")
    ap.add_argument("--cxx", default="/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else "clang++")
    args = ap.parse_args()
    dtypes = [{"f64": np.float64, "f32": np.float32}[t] for t in args.dtypes.split(",")]
    heads = [int(h) for h in args.heads.split(",")]
    kds = [tuple(int(v) for v in kd.split("x")) for kd in args.kd.split(",")]
    orc = Oracle()
    mats = matrices()
    with tempfile.TemporaryDirectory() as tmp:
        fwd, bwd = os.path.join(tmp, "mha_edge_host"), os.path.join(tmp, "mha_edge_bwd_host")
        build(args.cxx, "mha_edge_main.cpp", fwd)
        build(args.cxx, "mha_edge_bwd_main.cpp", bwd)
        for name in args.matrices.split(","):
            mat = mats(name)
            matT, amap = transpose_with_map(mat)
            ones = np.ones(mat.nnz)
            conv = {s: orc.convert(64, s, mat.m, mat.row_ptr, mat.col, ones) for s in (4, 7, 16)}
            convT = {s: orc.convert(64, s, matT.m, matT.row_ptr, matT.col, ones) for s in (4, 7, 16)}
            empty_r, empty_c = np.diff(mat.row_ptr) == 0, np.diff(matT.row_ptr) == 0
            for dtype in dtypes:
                u = float(np.finfo(dtype).eps) / 2
                for H in heads:
                    B = distinct_bias(mat.nnz, H).astype(dtype)
                    for k, d in kds:
                        Q, K, V, dO = operands(mat, H, k, d, dtype)
                        ref, mag, smag = reference(mat, B, Q, K, V, dO)
                        first, worst = None, 0.0
                        for sigma, sigma_t, pad, groups in CONFIGS:
                            O = forward(fwd, tmp, conv[sigma], mat, sigma, B, True, Q, K, V, pad, groups)
                            G = backward(bwd, tmp, (conv[sigma], convT[sigma_t]), (mat, matT), (sigma, sigma_t), amap, B, True, Q, K, V,
                                         dO, pad, groups)
                            got = [O] + G
                            for g, r, a, e, what in zip(got, ref, mag, (empty_r, empty_r, empty_c, empty_c, None), NAMES):
                                assert not np.isnan(g).any(), (name, H, k, d, sigma, what, "unwritten or poisoned")
                                ok = within(g, r, a, smag, u)
                                assert ok.all(), (name, np.dtype(dtype).name, H, k, d, sigma, what, float(np.abs(g - r).max()))
                                worst = max(worst, float(np.abs(g - r).max()) if g.size else 0.0)
                                if e is not None:
                                    assert not np.ascontiguousarray(g[e]).view(np.uint8).any(), f"{what}: a line without entries is not +0"
                            first = got if first is None else first
                            for g, g0, what in zip(got, first, NAMES):
                                assert same(g, g0), (name, H, k, d, sigma, what, "bits")
                        zero = np.zeros_like(B)
                        with_zero = [forward(fwd, tmp, conv[7], mat, 7, zero, True, Q, K, V, True, 0)] + \
                            backward(bwd, tmp, (conv[7], convT[4]), (mat, matT), (7, 4), amap, zero, True, Q, K, V, dO, True, 0)
                        without = [forward(fwd, tmp, conv[7], mat, 7, zero, False, Q, K, V, True, 0)] + \
                            backward(bwd, tmp, (conv[7], convT[4]), (mat, matT), (7, 4), amap, zero, False, Q, K, V, dO, True, 0)
                        for g, g0, what in zip(without, with_zero, NAMES):
                            assert same(g, g0), (name, H, k, d, what, "a null B against a B of +0")
                        alone = backward(bwd, tmp, (conv[7], convT[4]), (mat, matT), (7, 4), amap, B, True, Q, K, V, dO, True, 1, want=9)
                        assert same(alone[0], first[1]) and same(alone[3], first[4]), (name, H, k, d, "dQ and dB alone")
                        print(f"{name} {np.dtype(dtype).name} heads={H} k={k} d={d}: ok, worst |error| {worst:.2e}", flush=True)


if __name__ == "__main__":
    main()
