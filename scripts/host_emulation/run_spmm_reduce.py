#!/usr/bin/env python3
"""csr5hip_spmm_reduce and its two gradients (csr5_reduce.hip) on the CPU, without a GPU: the kernel source is compiled for the host
against the stand-in for the HIP runtime (fake/hip/hip_runtime.h) with -fsanitize=address,undefined and run as a stand-alone
program (reduce_driver.cpp) on matrices converted by the oracle WITH THEIR VALUES at sigma = 4, 7 and 16; for dX the transpose,
converted with the values in its own order, plays the transposed companion, with its source map.  Nothing is loaded into Python.

    python scripts/host_emulation/run_spmm_reduce.py [--matrices kat0,one-row,duplicates,aligned64,class-edges,dealt]
            [--dtypes f64,f32] [--ks 3,17] [--ops max,min] [--weighted 1,0] [--modes forward,dval,dx] [--cxx clang++]

EVERY ENTRY'S VALUE IS DISTINCT, so a value taken from another entry's storage position shows.  Per matrix, precision, op, weighted
and k, against tests/spmm_reduce_reference.py:
  * forward: Y and arg bit for bit (X holds repeated values, so ties occur and arg must be the smallest tied rank), at every sigma, with
    padded leading dimensions (NaN in the padding, which must survive) at sigma = 7, and without arg (the bits of Y unchanged);
  * dval: bit for bit the reference's chain, at every sigma; an arg with ranks of other rows written into it matches nothing more;
  * dx: inside the derived bound of the float64 reference, equal bits at every pair of sigmas, rows without a winner exactly +0.
Every array is an exact-size heap block.  This exercises the indexing, the row classes and the comparisons of the source; it says
nothing about the gfx950 build."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle.csr5_oracle import Oracle  # noqa: E402
from scripts.host_emulation import emulation as EMU  # noqa: E402
from tests import spmm_reduce_reference as R  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT = "kat0,one-row,duplicates,aligned64,class-edges,dealt"
MAGIC = 0x35444552
FIELDS = ("mode", "kind", "op", "weighted", "has_arg", "m", "nnz", "sigma", "p", "k", "xrows", "grows", "ldx", "ldg", "ldarg", "ldo")
FORWARD, DVAL, DX = range(3)
OPS = {"max": 0, "min": 1}
CONFIGS = ((4, 16, 0), (7, 4, 3), (16, 7, 0))  # sigma, the companion's sigma, what a padded case adds to every leading dimension


def build(cxx, out):
    cmd = [cxx, "-std=c++20", "-x", "c++", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-Wno-unknown-pragmas", f"-I{HERE}/fake", f"-I{ROOT}/benchmark_spmv_using_csr5_amd/csrc", f"-I{ROOT}/include",
           os.path.join(HERE, "reduce_driver.cpp"), "-o", out]
    subprocess.check_call(cmd)


def run(exe, tmp, mode, dtype, mt, fmt, k, pad, op=0, weighted=True, has_arg=True, amap=None, X=None, dY=None, arg=None, grows=0):
    """one case: the outputs, cut to their k columns, the padding checked for survival"""
    ld = k + pad
    h = dict(mode=mode, kind=EMU.KIND[np.dtype(dtype).name], op=op, weighted=int(weighted), has_arg=int(has_arg), m=mt.m, nnz=mt.nnz,
             sigma=fmt.sigma, p=fmt.p, k=k, xrows=0 if X is None else X.shape[0], grows=grows, ldx=ld, ldg=ld, ldarg=ld, ldo=ld)
    case, out = os.path.join(tmp, "case.bin"), os.path.join(tmp, "out.bin")
    with open(case, "wb") as f:
        np.array([MAGIC, len(FIELDS)], dtype=np.uint32).tofile(f)
        np.array([h[name] for name in FIELDS], dtype=np.int32).tofile(f)
        mt.row_ptr.astype(np.int32).tofile(f)
        fmt.col[:mt.nnz].astype(np.int32).tofile(f)
        fmt.tile_ptr.astype(np.uint32).tofile(f)
        if weighted and mode != DVAL:
            fmt.val[:mt.nnz].astype(dtype).tofile(f)
        if mode == DX:
            amap.astype(np.uint32).tofile(f)
        else:
            EMU.wide(X, ld).tofile(f)
        if mode != FORWARD:
            EMU.wide(dY, ld).tofile(f)
            EMU.wide(arg, ld, fill=-7).tofile(f)
    r = subprocess.run([exe, case, out], capture_output=True, text=True)
    if r.returncode:
        raise SystemExit(f"{mt.name} sigma {fmt.sigma} mode {mode}: exit {r.returncode}\n{r.stderr[-4000:]}")
    raw = np.fromfile(out, dtype=np.uint8)
    if mode == DVAL:
        return raw.view(dtype)
    n = np.dtype(dtype).itemsize * mt.m * ld
    Y = raw[:n].view(dtype).reshape(mt.m, ld)
    assert np.isnan(Y[:, k:]).all(), "written beyond the last column"
    if mode == DX or not has_arg:
        assert raw.size == n
        return np.ascontiguousarray(Y[:, :k])
    A = raw[n:].view(np.int32).reshape(mt.m, ld)
    assert (A[:, k:] == 0x7B7B7B7B).all(), "arg written beyond the last column"
    return np.ascontiguousarray(Y[:, :k]), np.ascontiguousarray(A[:, :k])


def main():
    args = EMU.arguments(DEFAULT, extra=(("--ks", dict(default="3,17")), ("--ops", dict(default="max,min")),
                                         ("--weighted", dict(default="1,0")), ("--modes", dict(default="forward,dval,dx"))))
    ks = [int(v) for v in args.ks.split(",")]
    ops = args.ops.split(",")
    weights = [bool(int(v)) for v in args.weighted.split(",")]
    modes = args.modes.split(",")
    orc = Oracle()
    mats = EMU.matrices()
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "spmm_reduce_host")
        build(args.cxx, exe)
        for name in args.matrices:
            mat = mats(name)
            val64 = R.distinct_values(mat.nnz, np.float64)
            pat = EMU.Patterns(orc, mat, val64)
            for dtype in args.dtypes:
                val = val64.astype(dtype)
                for k in ks:
                    rng = np.random.default_rng([5, k])
                    X = rng.integers(-3, 4, size=(mat.n, k)).astype(dtype) / dtype(4)  # repeated values: ties
                    dY = rng.uniform(-1, 1, size=(mat.m, k)).astype(dtype)
                    for op in ops:
                        for weighted in weights:
                            where = (name, np.dtype(dtype).name, op, "weighted" if weighted else "unweighted", k)
                            Yr, argr = R.forward(mat, val, X, op, weighted)
                            if "forward" in modes:
                                for sigma, _, pad in CONFIGS:
                                    Y, arg = run(exe, tmp, FORWARD, dtype, mat, pat.conv[sigma], k, pad, OPS[op], weighted, X=X)
                                    assert R.same_bits(arg, argr), where + (sigma, "arg")
                                    assert R.same_bits(Y, Yr), where + (sigma, "Y")
                                Y = run(exe, tmp, FORWARD, dtype, mat, pat.conv[4], k, 0, OPS[op], weighted, has_arg=False, X=X)
                                assert R.same_bits(Y, Yr), where + ("Y without arg",)
                            if "dval" in modes and weighted and op == ops[0]:
                                ref = R.dval(mat, X, dY, argr)
                                for sigma, _, pad in CONFIGS:
                                    got = run(exe, tmp, DVAL, dtype, mat, pat.conv[sigma], k, pad, X=X, dY=dY, arg=argr, grows=mat.m)
                                    assert R.same_bits(got, ref), where + (sigma, "dval")
                                if mat.m > 1:  # a corrupt arg: the ranks of the next row match nothing in this one
                                    bad = np.roll(argr, 1, axis=0)
                                    got = run(exe, tmp, DVAL, dtype, mat, pat.conv[7], k, 0, X=X, dY=dY, arg=bad, grows=mat.m)
                                    assert R.same_bits(got, R.dval(mat, X, dY, bad)), where + ("dval, corrupt arg",)
                            if "dx" in modes and op == ops[0]:
                                ref, w, mag = R.dx(mat, val, dY, argr, weighted)
                                bound = R.dx_bound(w, mag, dtype)
                                first = None
                                for _, sigma_t, pad in CONFIGS:
                                    got = run(exe, tmp, DX, dtype, pat.matT, pat.convT[sigma_t], k, pad, weighted=weighted, amap=pat.amap,
                                              dY=dY, arg=argr, grows=mat.m)
                                    assert not np.isnan(got).any(), where + (sigma_t, "dX unwritten")
                                    assert (np.abs(got.astype(np.float64) - ref) <= bound).all(), where + (sigma_t, "dX")
                                    assert not got[w == 0].view(np.uint8).any(), where + (sigma_t, "dX: not +0 where nothing wins")
                                    first = got if first is None else first
                                    assert R.same_bits(got, first), where + (sigma_t, "dX bits")
                            print(" ".join(str(v) for v in where) + ": ok", flush=True)


if __name__ == "__main__":
    main()
