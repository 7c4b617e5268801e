#!/usr/bin/env python3
"""The dropped attention entries (csr5_attention_drop.hip, csr5_attention_drop_gat.hip, their backwards and the mask kernel) on the
CPU, without a GPU: the kernel sources are compiled for the host against the stand-in for the HIP runtime
(fake/hip/hip_runtime.h) with -fsanitize=address,undefined, and run as ONE stand-alone program (dropout_main.cpp) on matrices of
tests/zoo.py converted by the oracle; for the backward the transpose, converted at another sigma, plays the transposed companion
and the stable sort by column that forms it is the source map, as in run_gat.py.  THE PATTERNS CARRY NO VALUE ARRAY AT ALL.

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
from scripts.host_emulation.run_gat import CONFIGS, distinct_a, operands, wide_nan  # noqa: E402
from scripts.host_emulation.run_mha import build, same  # noqa: E402
from scripts.host_emulation.run_mha_edge_bias import distinct_bias, transpose_with_map, wide_bias  # noqa: E402
from tests import dropout_reference as DR  # noqa: E402
from tests import gat_reference as G  # noqa: E402

DEFAULT = "kat0,duplicates"
HEADS = (1, 3, 5)
K, D = 3, 5
SCALE, SLOPE, P = 0.37, 0.2, 0.4
SEED, OFFSET, HEAD0 = 2 ** 63 + 5, 2 ** 32 + 1, 2
NAMES = G.NAMES


def run(exe, tmp, fmts, mats, sigmas, amap, family, a, B, Q, K_, V, dO, pad, groups, mode, want=31):
    """mode 0: O; mode 1: [dQ, dK, dV, dB, dAr] (None where not wanted); mode 2: the mask, (nnz, ldb) bytes"""
    dtype, (_, H, k), d = Q.dtype, Q.shape, V.shape[2]
    wk, wd = H * k, H * d
    lds = (wk + 3, wk + 1, wd + 2, wd + 3, wk + 1, wk + 2, wd + 1) if pad else (wk, wk, wd, wd, wk, wk, wd)
    ldb, lddb, lddar = (H + 2, H + 3, wk + 2) if pad else (H, H, wk)
    mat, matT = mats
    header = [mat.m, mat.n, mat.nnz, sigmas[0], fmts[0].p, sigmas[1], fmts[1].p, k, d, *lds, int(dtype == np.float64), want, H, groups,
              1, ldb, lddb, 1, lddar, mode, family, HEAD0]
    arrays = [amap.astype(np.uint32), np.ascontiguousarray(a, dtype=dtype), wide_bias(B.astype(dtype), ldb)]
    arrays += [wide_nan(t, ld) for t, ld in zip((Q, K_, V), lds[:3])] + ([wide_nan(dO, lds[3])] if mode == 1 else [])
    case, out = os.path.join(tmp, "case.bin"), os.path.join(tmp, "out.bin")
    with open(case, "wb") as f:
        np.array(header, dtype=np.int32).tofile(f)
        np.array([SCALE, SLOPE, P], dtype=np.float64).tofile(f)
        np.array([SEED, OFFSET], dtype=np.uint64).tofile(f)
        for mt, fmt in zip(mats, fmts):
            mt.row_ptr.astype(np.int32).tofile(f)
            fmt.col[:mt.nnz].astype(np.int32).tofile(f)
            fmt.tile_ptr.astype(np.uint32).tofile(f)
        for t in arrays:
            t.tofile(f)
    r = subprocess.run([exe, case, out], capture_output=True, text=True)
    if r.returncode:
        raise SystemExit(f"{mat.name} sigma {sigmas} family {family} mode {mode}: exit {r.returncode}\n{r.stderr[-4000:]}")
    if mode == 2:
        return np.fromfile(out, dtype=np.uint8).reshape(mat.nnz, ldb)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrices", default=DEFAULT)
    ap.add_argument("--dtypes", default="f64,f32")
    ap.add_argument("--heads", default=",".join(str(h) for h in HEADS))
    ap.add_argument("--cxx", default="/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else "clang++")
    args = ap.parse_args()
    dtypes = [{"f64": np.float64, "f32": np.float32}[t] for t in args.dtypes.split(",")]
    heads = [int(h) for h in args.heads.split(",")]
    orc = Oracle()
    mats = matrices()
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "dropout_host")
        build(args.cxx, "dropout_main.cpp", exe)
        for name in args.matrices.split(","):
            mat = mats(name)
            matT, amap = transpose_with_map(mat)
            ones = np.ones(mat.nnz)
            conv = {s: orc.convert(64, s, mat.m, mat.row_ptr, mat.col, ones) for s in (4, 7, 16)}
            convT = {s: orc.convert(64, s, matT.m, matT.row_ptr, matT.col, ones) for s in (4, 7, 16)}
            empty_r, empty_c = np.diff(mat.row_ptr) == 0, np.diff(matT.row_ptr) == 0
            for dtype in dtypes:
                u = float(np.finfo(dtype).eps) / 2
                ns, c, cd = float(dtype(SLOPE)), float(dtype(SCALE)), DR.cd_of(P, dtype)
                for H in heads:
                    B = distinct_bias(mat.nnz, H).astype(dtype)
                    a = distinct_a(H, K, dtype)
                    Q, K_, V, dO = operands(mat, H, K, D, dtype)
                    keep = DR.mask(mat.nnz, H, P, SEED, OFFSET, HEAD0)
                    assert 0 < keep.mean() < 1 or mat.nnz * H < 8
                    smag = float((abs(c) * (np.abs(Q).sum(2).max() + 1) * (np.abs(K_).sum(2).max() + 1) + 2)) if mat.nnz else 0.0
                    worst = 0.0
                    for family in (0, 1):
                        ref, mag = DR.numpy_reference(mat, c, B, Q, K_, V, dO, keep, cd, gat=(a, ns) if family else None)

                        def both(sigma, sigma_t, pad, groups, want=31 if family else 15):  # (the dot-product family has no dAr)
                            pair = ((conv[sigma], convT[sigma_t]), (mat, matT), (sigma, sigma_t), amap, family, a, B, Q, K_, V, dO)
                            return [run(exe, tmp, *pair, pad, groups, 0)] + run(exe, tmp, *pair, pad, groups, 1, want)
                        first = None
                        for sigma, sigma_t, pad, groups in CONFIGS:
                            got = both(sigma, sigma_t, pad, groups)
                            if first is None:
                                m_ = run(exe, tmp, (conv[sigma], convT[sigma_t]), (mat, matT), (sigma, sigma_t), amap, family, a, B, Q, K_,
                                         V, dO, True, groups, 2)
                                assert np.array_equal(m_[:, :H], keep) and (m_[:, H:] == 0xAB).all(), (name, H, "the mask kernel")
                            for i, (g, e, what) in enumerate(zip(got, (empty_r, empty_r, empty_c, empty_c, None, empty_r), NAMES)):
                                if g is None:
                                    continue
                                assert not np.isnan(g).any(), (name, H, family, sigma, what, "unwritten or poisoned")
                                ok = G.within(g, ref[i], mag[i], smag, u)
                                assert ok.all(), (name, np.dtype(dtype).name, H, family, sigma, what, float(np.abs(g - ref[i]).max()))
                                worst = max(worst, float(np.abs(g - ref[i]).max()) if g.size else 0.0)
                                if e is not None:
                                    assert not np.ascontiguousarray(g[e]).view(np.uint8).any(), f"{what}: a line without entries is not +0"
                            first = got if first is None else first
                            for g, g0, what in zip(got, first, NAMES):
                                assert g is None or same(g, g0), (name, H, family, sigma, what, "bits")
                        alone = both(7, 4, True, 1, want=9)
                        assert same(alone[1], first[1]) and same(alone[4], first[4]), "dQ and dB alone"
                    print(f"{name} {np.dtype(dtype).name} heads={H} k={K} d={D}: ok, worst |error| {worst:.2e}", flush=True)


if __name__ == "__main__":
    main()
