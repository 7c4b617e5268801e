#!/usr/bin/env python3
"""The additive attention entries (csr5_attention_gat.hip, csr5_attention_bwd_gat.hip) on the CPU, without a GPU: the kernel sources
are compiled for the host against the stand-in for the HIP runtime (fake/hip/hip_runtime.h) with -fsanitize=address,undefined, and
run as ONE stand-alone program (gat_main.cpp, forward and backward) on matrices of tests/zoo.py converted by the oracle; for the
backward the transpose, converted at another sigma, plays the transposed companion and the stable sort by column that forms it is
the source map, as in run_mha_edge_bias.py.  THE PATTERNS CARRY NO VALUE ARRAY AT ALL (null pointers).

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

from oracle.csr5_oracle import Oracle  # noqa: E402
from scripts.host_emulation.run_attention_backward import matrices  # noqa: E402
from scripts.host_emulation.run_mha import build, same  # noqa: E402
from scripts.host_emulation.run_mha_edge_bias import distinct_bias, transpose_with_map, wide_bias  # noqa: E402
from tests import gat_reference as G  # noqa: E402

DEFAULT = "kat0,duplicates"
HEADS = (1, 3)
KD = ((1, 5), (3, 5))
CONFIGS = ((4, 16, False, 0), (7, 4, True, 1), (16, 7, False, 1))  # sigma, the companion's sigma, padded, head groups (0: the rule)
SCALE, SLOPE = 0.37, 0.2
NAMES = G.NAMES


def distinct_a(H, k, dtype):
    """(H, k): H k equidistant values in [-1, 1) without a zero, in an order of their own"""
    v = (np.random.default_rng(13).permutation(H * k) + 0.5) / (H * k) * 2 - 1
    return v.reshape(H, k).astype(dtype)


def wide_nan(t, ld):
    """(rows, heads, width) packed into rows of ld values, EXACTLY rows ld elements, the padding NaN"""
    w = np.full((t.shape[0], ld), np.nan, dtype=t.dtype)
    w[:, :t.shape[1] * t.shape[2]] = t.reshape(t.shape[0], -1)
    return w


def run(exe, tmp, fmts, mats, sigmas, amap, a, use_a, B, use_b, Q, K, V, dO, pad, groups, mode, want=31):
    """mode 0: O; mode 1: [dQ, dK, dV, dB, dAr] (None where not wanted)"""
    dtype, (_, H, k), d = Q.dtype, Q.shape, V.shape[2]
    wk, wd = H * k, H * d
    lds = (wk + 3, wk + 1, wd + 2, wd + 3, wk + 1, wk + 2, wd + 1) if pad else (wk, wk, wd, wd, wk, wk, wd)
    ldb, lddb, lddar = (H + 2, H + 3, wk + 2) if pad else (H, H, wk)
    mat, matT = mats
    header = [mat.m, mat.n, mat.nnz, sigmas[0], fmts[0].p, sigmas[1], fmts[1].p, k, d, *lds, int(dtype == np.float64), want, H, groups,
              int(use_b), ldb, lddb, int(use_a), lddar, mode]
    arrays = [amap.astype(np.uint32), np.ascontiguousarray(a, dtype=dtype), wide_bias(B.astype(dtype), ldb)]
    arrays += [wide_nan(t, ld) for t, ld in zip((Q, K, V), lds[:3])] + ([wide_nan(dO, lds[3])] if mode else [])
    case, out = os.path.join(tmp, "case.bin"), os.path.join(tmp, "out.bin")
    with open(case, "wb") as f:
        np.array(header, dtype=np.int32).tofile(f)
        np.array([SCALE, SLOPE], dtype=np.float64).tofile(f)
        for mt, fmt in zip(mats, fmts):
            mt.row_ptr.astype(np.int32).tofile(f)
            fmt.col[:mt.nnz].astype(np.int32).tofile(f)
            fmt.tile_ptr.astype(np.uint32).tofile(f)
        for t in arrays:
            t.tofile(f)
    r = subprocess.run([exe, case, out], capture_output=True, text=True)
    if r.returncode:
        raise SystemExit(f"{mat.name} sigma {sigmas} mode {mode}: exit {r.returncode}\n{r.stderr[-4000:]}")
    flat = np.fromfile(out, dtype=dtype)
    if not mode:
        O = flat.reshape(mat.m, lds[3])
        assert np.isnan(O[:, wd:]).all(), "written beyond column heads * d"
        return np.ascontiguousarray(O[:, :wd]).reshape(mat.m, H, d)
    res, at = [], 0
    for bit, rows, ld, width in ((1, mat.m, lds[4], wk), (2, mat.n, lds[5], wk), (4, mat.n, lds[6], wd), (8, mat.nnz, lddb, H),
                                 (16, mat.m, lddar, wk)):
        g = flat[at:at + rows * ld].reshape(rows, ld)
        at += rows * ld
        assert np.isnan(g[:, width:]).all(), "written beyond the last column"
        if want & bit:
            res.append(np.ascontiguousarray(g[:, :width]).reshape((rows, H, width // H) if bit != 8 else (rows, H)))
        else:
            assert np.isnan(g).all(), "an output that was not wanted is written"
            res.append(None)
    return res


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
        exe = os.path.join(tmp, "gat_host")
        build(args.cxx, "gat_main.cpp", exe)
        for name in args.matrices.split(","):
            mat = mats(name)
            matT, amap = transpose_with_map(mat)
            ones = np.ones(mat.nnz)
            conv = {s: orc.convert(64, s, mat.m, mat.row_ptr, mat.col, ones) for s in (4, 7, 16)}
            convT = {s: orc.convert(64, s, matT.m, matT.row_ptr, matT.col, ones) for s in (4, 7, 16)}
            empty_r, empty_c = np.diff(mat.row_ptr) == 0, np.diff(matT.row_ptr) == 0
            for dtype in dtypes:
                u = float(np.finfo(dtype).eps) / 2
                ns = float(dtype(SLOPE))
                for H in heads:
                    B = distinct_bias(mat.nnz, H).astype(dtype)
                    for k, d in kds:
                        a = distinct_a(H, k, dtype)
                        Q, K, V, dO = operands(mat, H, k, d, dtype)
                        ref, mag, smag = G.numpy_reference(mat, a, ns, float(dtype(SCALE)), B, Q, K, V, dO)

                        def both(sigma, sigma_t, pad, groups, a_=a, use_a=True, B_=B, use_b=True, want=31):
                            pair = ((conv[sigma], convT[sigma_t]), (mat, matT), (sigma, sigma_t), amap, a_, use_a, B_, use_b, Q, K, V, dO)
                            return [run(exe, tmp, *pair, pad, groups, 0)] + run(exe, tmp, *pair, pad, groups, 1, want)
                        first, worst = None, 0.0
                        for sigma, sigma_t, pad, groups in CONFIGS:
                            got = both(sigma, sigma_t, pad, groups)
                            for g, r, al, e, what in zip(got, ref, mag, (empty_r, empty_r, empty_c, empty_c, None, empty_r), NAMES):
                                assert not np.isnan(g).any(), (name, H, k, d, sigma, what, "unwritten or poisoned")
                                ok = G.within(g, r, al, smag, u)
                                assert ok.all(), (name, np.dtype(dtype).name, H, k, d, sigma, what, float(np.abs(g - r).max()))
                                worst = max(worst, float(np.abs(g - r).max()) if g.size else 0.0)
                                if e is not None:
                                    assert not np.ascontiguousarray(g[e]).view(np.uint8).any(), f"{what}: a line without entries is not +0"
                            first = got if first is None else first
                            for g, g0, what in zip(got, first, NAMES):
                                assert same(g, g0), (name, H, k, d, sigma, what, "bits")
                        one, zero = np.ones_like(a), np.zeros_like(B)
                        for g, g0, what in zip(both(7, 4, True, 0, a_=one, use_a=False, B_=zero, use_b=False),
                                               both(7, 4, True, 0, a_=one, B_=zero), NAMES):
                            assert same(g, g0), (name, H, k, d, what, "a null a and a null B against ones and +0")
                        alone = both(7, 4, True, 1, want=25)
                        assert same(alone[1], first[1]) and same(alone[4], first[4]) and same(alone[5], first[5]), "dQ, dB and dAr alone"
                        only = both(7, 4, True, 1, want=16)
                        assert same(only[5], first[5]), (name, H, k, d, "dAr alone")
                        print(f"{name} {np.dtype(dtype).name} heads={H} k={k} d={d}: ok, worst |error| {worst:.2e}", flush=True)


if __name__ == "__main__":
    main()
