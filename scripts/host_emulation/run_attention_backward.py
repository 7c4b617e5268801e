#!/usr/bin/env python3
"""csr5_attention_bwd.hip on the CPU, without a GPU: the kernel source is compiled for the host against the stand-in for the HIP
runtime (fake/hip/hip_runtime.h) with -fsanitize=address,undefined, and run as a stand-alone program on matrices of tests/zoo.py
and their transposes, both converted by the oracle (the transpose plays the transposed companion).

    python scripts/host_emulation/run_attention_backward.py [--matrices kat0,duplicates,...] [--kd 3x5,8x16] [--cxx clang++]

--matrices also takes class-edges and dealt of tests/attention_edges.py (a line on every class edge, hubs in every workgroup) and
NAME^T for the transpose of any matrix.

Per matrix, precision and (k, d): dQ, dK and dV against a float64 numpy reference (1e3 unit roundoffs of the gradient expression on
absolute values: a check of the indexing, not the accuracy test), rows and columns without entries exactly +0, nothing written
beyond column k or d, dQ alone without a workspace, and equal bits for sigma = 4, sigma = 7 with padded leading dimensions
(element loads) and sigma = 16 (16-byte loads); the companion is converted at another sigma than the parent.  This exercises the
indexing, the row classes and the arithmetic of the source; it says nothing about the gfx950 build."""
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
from tests import attention_edges as E  # noqa: E402
from tests import sddmm_reference as S  # noqa: E402
from tests import zoo  # noqa: E402

KD = ((1, 1), (3, 5), (8, 16), (70, 40), (0, 7), (7, 0), (5, 300), (300, 5))
DEFAULT = "kat0,duplicates,aligned64,aligned1024,one-row,aligned64^T,aligned1024^T,one-row^T"


def transpose(mat):
    """A^T in CSR with every column's entries in A's CSR order (a stable sort by column)"""
    rows = np.repeat(np.arange(mat.m, dtype=np.int64), np.diff(mat.row_ptr))
    cols = mat.col[:mat.nnz].astype(np.int64)
    order = np.argsort(cols, kind="stable")
    rp = np.zeros(mat.n + 1, dtype=np.int32)
    rp[1:] = np.cumsum(np.bincount(cols, minlength=mat.n))
    return M.CsrMatrix(mat.n, mat.m, rp, rows[order].astype(np.int32), np.ones(mat.nnz), mat.name + "^T")


def matrices():
    """name -> matrix: tests/zoo.py's, the duplicates matrix, class-edges and dealt; NAME^T is the transpose"""
    mats = {m.name: m for m in zoo.small_zoo()}
    mats["duplicates"] = S.duplicates_matrix()
    mats["class-edges"] = E.class_edges()
    mats["dealt"] = E.dealt()
    return lambda name: transpose(mats[name[:-2]]) if name.endswith("^T") else mats[name]


def build(cxx, out):
    cmd = [cxx, "-std=c++20", "-x", "c++", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-Wno-unknown-pragmas", f"-I{HERE}/fake", f"-I{ROOT}/benchmark_spmv_using_csr5_amd/csrc", f"-I{ROOT}/include",
           os.path.join(HERE, "attention_bwd_main.cpp"), "-o", out]
    subprocess.check_call(cmd)


def run(exe, tmp, orc, mat, matT, sigma, sigma_t, dtype, Q, K, V, dO, pad, want=7):
    k, d = Q.shape[1], V.shape[1]
    lds = (k + 3, k + 1, d + 2, d + 3, k + 1, k + 2, d + 1) if pad else (k, k, d, d, k, k, d)
    fmt = orc.convert(64, sigma, mat.m, mat.row_ptr, mat.col, np.ones(mat.nnz))
    fmt_t = orc.convert(64, sigma_t, matT.m, matT.row_ptr, matT.col, np.ones(matT.nnz))

    def wide(t, ld):
        w = np.full((t.shape[0], ld), 7.5, dtype=dtype)
        w[:, :t.shape[1]] = t
        return w
    case, out = os.path.join(tmp, "case.bin"), os.path.join(tmp, "out.bin")
    with open(case, "wb") as f:
        np.array([mat.m, mat.n, mat.nnz, sigma, fmt.p, sigma_t, fmt_t.p, k, d, *lds, int(dtype == np.float64), want],
                 dtype=np.int32).tofile(f)
        for m_, f_ in ((mat, fmt), (matT, fmt_t)):
            m_.row_ptr.astype(np.int32).tofile(f)
            f_.col[:m_.nnz].astype(np.int32).tofile(f)
            f_.tile_ptr.astype(np.uint32).tofile(f)
        for t, ld in zip((Q, K, V, dO), lds[:4]):
            wide(t, ld).tofile(f)
    r = subprocess.run([exe, case, out], capture_output=True, text=True)
    if r.returncode:
        raise SystemExit(f"{mat.name} sigma {sigma}: exit {r.returncode}\n{r.stderr[-4000:]}")
    flat = np.fromfile(out, dtype=dtype)
    res, at = [], 0
    for bit, rows, ld, width in ((1, mat.m, lds[4], k), (2, mat.n, lds[5], k), (4, mat.n, lds[6], d)):
        g = flat[at:at + rows * ld].reshape(rows, ld)
        at += rows * ld
        assert np.isnan(g[:, width:]).all(), "written beyond the last column"
        if want & bit:
            res.append(np.ascontiguousarray(g[:, :width]))
        else:
            assert np.isnan(g).all(), "an output that was not wanted is written"
            res.append(None)
    return res


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
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrices", default=DEFAULT)
    ap.add_argument("--kd", default=",".join(f"{k}x{d}" for k, d in KD))
    ap.add_argument("--cxx", default="/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else "clang++")
    args = ap.parse_args()
    kds = [tuple(int(v) for v in kd.split("x")) for kd in args.kd.split(",")]
    orc = Oracle()
    mats = matrices()
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "attention_bwd_host")
        build(args.cxx, exe)
        for name in args.matrices.split(","):
            mat = mats(name)
            matT = transpose(mat)
            empty = (np.diff(mat.row_ptr) == 0, np.diff(matT.row_ptr) == 0, np.diff(matT.row_ptr) == 0)
            for dtype in (np.float64, np.float32):
                u = float(np.finfo(dtype).eps) / 2
                for k, d in kds:
                    rng = np.random.default_rng(5)
                    Q = (rng.uniform(-1, 1, (mat.m, k)) * 2).astype(dtype)
                    K = rng.uniform(-1, 1, (mat.n, k)).astype(dtype)
                    V = rng.uniform(-1, 1, (mat.n, d)).astype(dtype)
                    dO = rng.uniform(-1, 1, (mat.m, d)).astype(dtype)
                    ref, mag = reference(mat, Q, K, V, dO)
                    first, worst = None, 0.0
                    for sigma, sigma_t, pad in ((4, 16, False), (7, 4, True), (16, 7, False)):
                        got = run(exe, tmp, orc, mat, matT, sigma, sigma_t, dtype, Q, K, V, dO, pad)
                        for g, r, a, e, what in zip(got, ref, mag, empty, ("dQ", "dK", "dV")):
                            err = np.abs(g - r)
                            assert (err <= 1e3 * u * np.maximum(a, 1e-30) + 1e-300).all(), (name, dtype, k, d, sigma, what, float(err.max()))
                            worst = max(worst, float(err.max()) if err.size else 0.0)
                            assert not np.ascontiguousarray(g[e]).view(np.uint8).any(), f"{what}: a row without entries is not +0"
                        first = got if first is None else first
                        for g, g0, what in zip(got, first, ("dQ", "dK", "dV")):
                            assert np.array_equal(g0.view(np.uint8), g.view(np.uint8)), (name, k, d, sigma, what, "bits")
                    alone = run(exe, tmp, orc, mat, matT, 7, 4, dtype, Q, K, V, dO, True, want=1)  # no workspace, no companion
                    assert np.array_equal(alone[0].view(np.uint8), first[0].view(np.uint8)), (name, k, d, "dQ alone")
                    print(f"{name} {np.dtype(dtype).name} k={k} d={d}: ok, worst |error| {worst:.2e}", flush=True)


if __name__ == "__main__":
    main()
