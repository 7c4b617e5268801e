#!/usr/bin/env python3
"""csr5_attention.hip on the CPU, without a GPU: the kernel source is compiled for the host against a stand-in for the HIP runtime
(fake/hip/hip_runtime.h: 256 threads per workgroup, cross-lane operations emulated) with -fsanitize=address,undefined, and run as
a stand-alone program on matrices of tests/zoo.py converted by the oracle.

    python scripts/host_emulation/run_attention.py [--matrices kat0,duplicates,aligned64,aligned1024,one-row] [--cxx clang++]

--matrices also takes class-edges and dealt of tests/attention_edges.py (a line on every class edge, hubs in every workgroup) and
NAME^T for the transpose of any of them.

Per matrix, precision and (k, d): O against a float64 numpy reference (1e3 unit roundoffs of the largest |V| sum: a check of the
indexing, not the accuracy test), rows without entries exactly +0, nothing written beyond column d, and equal bits for sigma = 4,
sigma = 7 with padded leading dimensions (element loads) and sigma = 16 (16-byte loads).  This exercises the indexing, the row
classes and the arithmetic of the source; it says nothing about the gfx950 build."""
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

KD = ((1, 1), (3, 5), (8, 16), (40, 70), (0, 7), (5, 300))


def build(cxx, out):
    cmd = [cxx, "-std=c++20", "-x", "c++", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-Wno-unknown-pragmas", f"-I{HERE}/fake", f"-I{ROOT}/benchmark_spmv_using_csr5_amd/csrc", f"-I{ROOT}/include",
           os.path.join(HERE, "attention_main.cpp"), "-o", out]
    subprocess.check_call(cmd)


def run(exe, tmp, orc, mat, sigma, dtype, Q, K, V, pad):
    k, d = Q.shape[1], V.shape[1]
    ldq, ldk, ldv, ldo = (k + 3, k + 1, d + 2, d + 3) if pad else (k, k, d, d)
    fmt = orc.convert(64, sigma, mat.m, mat.row_ptr, mat.col, np.ones(mat.nnz))

    def wide(t, ld):
        w = np.full((t.shape[0], ld), 7.5, dtype=dtype)
        w[:, :t.shape[1]] = t
        return w
    case, out = os.path.join(tmp, "case.bin"), os.path.join(tmp, "out.bin")
    with open(case, "wb") as f:
        np.array([mat.m, mat.n, mat.nnz, sigma, fmt.p, k, d, ldq, ldk, ldv, ldo, int(dtype == np.float64)], dtype=np.int32).tofile(f)
        mat.row_ptr.astype(np.int32).tofile(f)
        fmt.col[:mat.nnz].astype(np.int32).tofile(f)
        fmt.tile_ptr.astype(np.uint32).tofile(f)
        for t, ld in ((Q, ldq), (K, ldk), (V, ldv)):
            wide(t, ld).tofile(f)
    r = subprocess.run([exe, case, out], capture_output=True, text=True)
    if r.returncode:
        raise SystemExit(f"{mat.name} sigma {sigma}: exit {r.returncode}\n{r.stderr[-4000:]}")
    O = np.fromfile(out, dtype=dtype).reshape(mat.m, ldo)
    assert np.isnan(O[:, d:]).all(), "written beyond column d"
    return O[:, :d]


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
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrices", default="kat0,duplicates,aligned64,aligned1024,one-row")
    ap.add_argument("--cxx", default="/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else "clang++")
    args = ap.parse_args()
    orc = Oracle()
    mats = matrices()
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "attention_host")
        build(args.cxx, exe)
        for name in args.matrices.split(","):
            mat = mats(name)
            for dtype in (np.float64, np.float32):
                u = float(np.finfo(dtype).eps) / 2
                for k, d in KD:
                    rng = np.random.default_rng(5)
                    Q = (rng.uniform(-1, 1, (mat.m, k)) * 2).astype(dtype)
                    K = rng.uniform(-1, 1, (mat.n, k)).astype(dtype)
                    V = rng.uniform(-1, 1, (mat.n, d)).astype(dtype)
                    ref, scale = reference(mat, Q, K, V)
                    first = None
                    for sigma, pad in ((4, False), (7, True), (16, False)):
                        O = run(exe, tmp, orc, mat, sigma, dtype, Q, K, V, pad)
                        err = float(np.abs(O - ref).max())
                        assert err <= 1e3 * u * scale, (name, dtype, k, d, sigma, err)
                        empty = np.diff(mat.row_ptr) == 0
                        assert not np.ascontiguousarray(O[empty]).view(np.uint8).any(), "an empty row is not +0"
                        first = O.copy() if first is None else first
                        assert np.array_equal(first.view(np.uint8), np.ascontiguousarray(O).view(np.uint8)), (name, k, d, sigma, "bits")
                    print(f"{name} {np.dtype(dtype).name} k={k} d={d}: ok, worst |error| {err:.2e}", flush=True)


if __name__ == "__main__":
    main()
