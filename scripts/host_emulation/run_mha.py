#!/usr/bin/env python3
"""The multi-head entries of csr5_attention.hip and csr5_attention_bwd.hip on the CPU, without a GPU: the kernel sources are
compiled for the host against the stand-in for the HIP runtime (fake/hip/hip_runtime.h) with -fsanitize=address,undefined, and run
as stand-alone programs (mha_main.cpp, mha_bwd_main.cpp) on matrices of tests/zoo.py converted by the oracle; for the backward
the transpose, converted at another sigma, plays the transposed companion.

    python scripts/host_emulation/run_mha.py [--matrices kat0,duplicates,aligned64,aligned1024,one-row] [--dtypes f64,f32]
                                             [--heads 1,3] [--kd 3x5,8x16,5x300] [--cxx clang++]

--matrices also takes class-edges and dealt of tests/attention_edges.py (a line on every class edge, hubs in every workgroup) and
NAME^T for the transpose of any matrix.

Per matrix, precision, heads in {1, 3} and (k, d) in {(3, 5), (8, 16), (5, 300)}, forward and backward:
  * head h of the packed call has the same bits as the SINGLE-HEAD launcher on that head's slices of the same arrays;
  * nothing is written beyond column heads * d (heads * k) of an output, and nothing at all into an output that is not wanted;
  * equal bits for sigma = 4 with the head groups of the rule, sigma = 7 with padded leading dimensions (element loads) and ONE
    group (all heads in one workgroup), and sigma = 16 with one group (16-byte loads where the slices allow them);
  * backward: dQ alone, without workspace and companion, has the bits it has with them.
Every array is an exact-size heap block (the workspace exactly 4 m heads values).  This exercises the indexing, the head loop in
the three row classes and the arithmetic of the source; it says nothing about the gfx950 build."""
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
from scripts.host_emulation.run_attention_backward import matrices, transpose  # noqa: E402

HEADS = (1, 3)
KD = ((3, 5), (8, 16), (5, 300))
CONFIGS = ((4, 16, False, 0), (7, 4, True, 1), (16, 7, False, 1))  # sigma, the companion's sigma, padded, head groups (0: the rule)


def build(cxx, main, out):
    cmd = [cxx, "-std=c++20", "-x", "c++", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-Wno-unknown-pragmas", f"-I{HERE}/fake", f"-I{ROOT}/benchmark_spmv_using_csr5_amd/csrc", f"-I{ROOT}/include",
           os.path.join(HERE, main), "-o", out]
    subprocess.check_call(cmd)


def wide(t, ld):
    """(rows, heads, width) packed into rows of ld values, the tail 7.5"""
    w = np.full((t.shape[0], ld), 7.5, dtype=t.dtype)
    w[:, :t.shape[1] * t.shape[2]] = t.reshape(t.shape[0], -1)
    return w


def execute(exe, tmp, header, patterns, operands, name):
    case, out = os.path.join(tmp, "case.bin"), os.path.join(tmp, "out.bin")
    with open(case, "wb") as f:
        np.array(header, dtype=np.int32).tofile(f)
        for mat, fmt in patterns:
            mat.row_ptr.astype(np.int32).tofile(f)
            fmt.col[:mat.nnz].astype(np.int32).tofile(f)
            fmt.tile_ptr.astype(np.uint32).tofile(f)
        for t in operands:
            t.tofile(f)
    r = subprocess.run([exe, case, out], capture_output=True, text=True)
    if r.returncode:
        raise SystemExit(f"{name}: exit {r.returncode}\n{r.stderr[-4000:]}")
    return out


def forward(exe, tmp, fmt, mat, sigma, Q, K, V, pad, groups, single=None):
    """O (m, heads, d) of the packed call, or with single = h of the single-head launcher on head h's slices (the rest NaN)"""
    dtype, (_, H, k), d = Q.dtype, Q.shape, V.shape[2]
    ldq, ldk, ldv, ldo = (H * k + 3, H * k + 1, H * d + 2, H * d + 3) if pad else (H * k, H * k, H * d, H * d)
    mode = (H, groups, 0, 0) if single is None else (0, 0, single * k, single * d)
    header = [mat.m, mat.n, mat.nnz, sigma, fmt.p, k, d, ldq, ldk, ldv, ldo, int(dtype == np.float64), *mode]
    out = execute(exe, tmp, header, ((mat, fmt),), (wide(Q, ldq), wide(K, ldk), wide(V, ldv)), f"{mat.name} sigma {sigma}")
    O = np.fromfile(out, dtype=dtype).reshape(mat.m, ldo)
    assert np.isnan(O[:, H * d:]).all(), "written beyond column heads * d"
    return np.ascontiguousarray(O[:, :H * d]).reshape(mat.m, H, d)


def backward(exe, tmp, fmts, mats, sigmas, Q, K, V, dO, pad, groups, want=7, single=None):
    """[dQ, dK, dV] packed (None where not wanted), or with single = h of the single-head launcher on head h's slices"""
    dtype, (_, H, k), d = Q.dtype, Q.shape, V.shape[2]
    wk, wd = H * k, H * d
    lds = (wk + 3, wk + 1, wd + 2, wd + 3, wk + 1, wk + 2, wd + 1) if pad else (wk, wk, wd, wd, wk, wk, wd)
    mat, matT = mats
    mode = (H, groups, 0, 0) if single is None else (0, 0, single * k, single * d)
    header = [mat.m, mat.n, mat.nnz, sigmas[0], fmts[0].p, sigmas[1], fmts[1].p, k, d, *lds, int(dtype == np.float64), want, *mode]
    out = execute(exe, tmp, header, zip(mats, fmts), [wide(t, ld) for t, ld in zip((Q, K, V, dO), lds[:4])], f"{mat.name} sigma {sigmas}")
    flat = np.fromfile(out, dtype=dtype)
    res, at = [], 0
    for bit, rows, ld, width in ((1, mat.m, lds[4], k), (2, mat.n, lds[5], k), (4, mat.n, lds[6], d)):
        g = flat[at:at + rows * ld].reshape(rows, ld)
        at += rows * ld
        assert np.isnan(g[:, H * width:]).all(), "written beyond the last column"
        if want & bit:
            res.append(np.ascontiguousarray(g[:, :H * width]).reshape(rows, H, width))
        else:
            assert np.isnan(g).all(), "an output that was not wanted is written"
            res.append(None)
    return res


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrices", default="kat0,duplicates,aligned64,aligned1024,one-row")
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
        fwd, bwd = os.path.join(tmp, "mha_host"), os.path.join(tmp, "mha_bwd_host")
        build(args.cxx, "mha_main.cpp", fwd)
        build(args.cxx, "mha_bwd_main.cpp", bwd)
        for name in args.matrices.split(","):
            mat = mats(name)
            matT = transpose(mat)
            conv = {s: orc.convert(64, s, mat.m, mat.row_ptr, mat.col, np.ones(mat.nnz)) for s in (4, 7, 16)}
            convT = {s: orc.convert(64, s, matT.m, matT.row_ptr, matT.col, np.ones(matT.nnz)) for s in (4, 7, 16)}
            for dtype in dtypes:
                for H in heads:
                    for k, d in kds:
                        rng = np.random.default_rng(5)
                        Q = (rng.uniform(-1, 1, (mat.m, H, k)) * 2).astype(dtype)
                        K = rng.uniform(-1, 1, (mat.n, H, k)).astype(dtype)
                        V = rng.uniform(-1, 1, (mat.n, H, d)).astype(dtype)
                        dO = rng.uniform(-1, 1, (mat.m, H, d)).astype(dtype)
                        O0 = G0 = None
                        for sigma, sigma_t, pad, groups in CONFIGS:
                            O = forward(fwd, tmp, conv[sigma], mat, sigma, Q, K, V, pad, groups)
                            G = backward(bwd, tmp, (conv[sigma], convT[sigma_t]), (mat, matT), (sigma, sigma_t), Q, K, V, dO, pad, groups)
                            assert not np.isnan(O).any() and not any(np.isnan(g).any() for g in G), (name, H, k, d, sigma, "unwritten")
                            O0, G0 = (O, G) if O0 is None else (O0, G0)
                            assert same(O, O0), (name, H, k, d, sigma, "O bits")
                            for g, g0, what in zip(G, G0, ("dQ", "dK", "dV")):
                                assert same(g, g0), (name, H, k, d, sigma, what, "bits")
                        for h in range(H):  # the single-head launcher on head h's slices of the same packed arrays
                            O1 = forward(fwd, tmp, conv[7], mat, 7, Q, K, V, True, 0, single=h)
                            assert same(O1[:, h], O0[:, h]), (name, H, k, d, h, "O against the single-head call")
                            G1 = backward(bwd, tmp, (conv[7], convT[4]), (mat, matT), (7, 4), Q, K, V, dO, True, 0, single=h)
                            for g1, g0, what in zip(G1, G0, ("dQ", "dK", "dV")):
                                assert same(g1[:, h], g0[:, h]), (name, H, k, d, h, what, "against the single-head call")
                        alone = backward(bwd, tmp, (conv[7], convT[4]), (mat, matT), (7, 4), Q, K, V, dO, True, 1, want=1)
                        assert same(alone[0], G0[0]), (name, H, k, d, "dQ alone")
                        print(f"{name} {np.dtype(dtype).name} heads={H} k={k} d={d}: ok", flush=True)


if __name__ == "__main__":
    main()
