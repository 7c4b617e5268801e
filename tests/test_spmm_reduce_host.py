"""csr5hip_spmm_reduce / csr5hip_spmm_reduce_backward on the host side (no GPU): the C ABI symbols and their declarations, the C++
class members, the return codes and their order, the Python argument checks, that ``autograd.spmm_reduce`` is exported, the numpy
reference (tests/spmm_reduce_reference.py) against torch-CPU ``amax`` / ``amin`` and against the contract's special cases, and the host
emulation of the kernel source under the address and undefined-behaviour sanitizers (a stand-alone program)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from benchmark_spmv_using_csr5_amd import _capi
from benchmark_spmv_using_csr5_amd import handle as H
from benchmark_spmv_using_csr5_amd import matrices as M
from tests import sddmm_reference as S
from tests import spmm_reduce_reference as R
from tests import zoo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
DECLS = {
    "csr5hip_spmm_reduce": ("int csr5hip_spmm_reduce(csr5hip_handle h, int op, int weighted, const void *d_X, int ldx, int k, void *d_Y, "
                            "int ldy, int32_t *d_arg, int ldarg);"),
    "csr5hip_spmm_reduce_backward": ("int csr5hip_spmm_reduce_backward(csr5hip_handle h, int weighted, const void *d_X, int ldx, int k, "
                                     "const void *d_dY, int lddy, const int32_t *d_arg, int ldarg, void *d_dX, int lddx, "
                                     "void *d_dval_csr);"),
}


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_library_exports_both_symbols_with_the_declared_signatures():
    import torch  # noqa: F401  (one HIP runtime per process: see _capi.load)
    lib = C.CDLL(_capi.LIB_PATH)
    with open(os.path.join(INC, "csr5hip.h")) as f:
        assert '#include "csr5hip_reduce.h"' in f.read()
    with open(os.path.join(INC, "csr5hip_reduce.h")) as f:
        raw = f.read()
    text = re.sub(r"\s+", " ", raw)
    assert "#define CSR5HIP_REDUCE_MAX 0" in raw and "#define CSR5HIP_REDUCE_MIN 1" in raw
    for name, decl in DECLS.items():
        assert hasattr(lib, name)
        assert decl in text
    bound = {name: (res, args) for name, res, args in _capi.SYMBOLS_REDUCE}
    p, i = C.c_void_p, C.c_int
    assert bound == {"csr5hip_spmm_reduce": (i, [p, i, i, p, i, i, p, i, p, i]),
                     "csr5hip_spmm_reduce_backward": (i, [p, i, p, i, i, p, i, p, i, p, i, p])}
    loaded = _capi.load()
    assert loaded.csr5hip_spmm_reduce.argtypes == bound["csr5hip_spmm_reduce"][1]
    assert loaded.csr5hip_spmm_reduce_backward.argtypes == bound["csr5hip_spmm_reduce_backward"][1]
    assert not {n for n, _, _ in _capi.SYMBOLS} & set(bound)  # (SYMBOLS is as it was)
    assert (_capi.REDUCE_MAX, _capi.REDUCE_MIN) == (0, 1)


def test_cpp_class_has_the_reduce_members(tmp_path):
    src = tmp_path / "use_reduce.cpp"
    src.write_text(
        '#include "anonymouslib_hip.h"\n'
        "int use(anonymouslibHandle<int, unsigned, double> &A, const double *X, const double *dY, double *Y, int32_t *arg, double *dX,\n"
        "        double *dval)\n"
        "{ return A.spmmReduce(CSR5HIP_REDUCE_MAX, 1, X, 4, 4, Y, 5, arg, 4)\n"
        "       + A.spmmReduceBackward(1, X, 4, 4, dY, 5, arg, 4, dX, 4, dval); }\n"
        "int use32(anonymouslibHandle<int, unsigned, float> &A, const float *X, const float *dY, float *Y, int32_t *arg, float *dX)\n"
        "{ return A.spmmReduce(CSR5HIP_REDUCE_MIN, 0, X, 2, 2, Y, 2, nullptr, 0)\n"
        "       + A.spmmReduceBackward(0, nullptr, 2, 2, dY, 2, arg, 2, dX, 2, nullptr); }\n")
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", f"-I{INC}", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_return_codes_in_order_without_a_gpu():
    """Decided on the host, with fake non-null pointers, on a handle that never touches a device: the arguments first, then the
    format (CSR before "no matrix", as csr5hip_spmm), then the companion"""
    lib = _capi.load()
    INV, CSR, UNK = _capi.INVALID_ARGUMENT, _capi.UNSUPPORTED_CSR_SPMV, _capi.UNKOWN_FORMAT
    h = C.c_void_p()
    assert lib.csr5hip_create(C.byref(h), 10, 10, _capi.F64) == 0
    fake = C.c_void_p(64)
    fwd, bwd = lib.csr5hip_spmm_reduce, lib.csr5hip_spmm_reduce_backward
    for stage in ("before inputCSR", "CSR"):
        fmt = UNK if stage == "before inputCSR" else CSR
        assert fwd(h, 0, 1, fake, 2, 2, fake, 2, fake, 2) == fmt
        assert fwd(h, 1, 0, fake, 2, 2, fake, 2, None, 0) == fmt          # arg is optional, ldarg then not judged
        assert fwd(h, 0, 1, None, 0, 0, None, 0, None, 0) == fmt          # k = 0: no operand needed, the format still decides
        assert fwd(None, 0, 1, fake, 2, 2, fake, 2, fake, 2) == INV
        assert fwd(h, 2, 1, fake, 2, 2, fake, 2, fake, 2) == INV          # op
        assert fwd(h, -1, 1, fake, 2, 2, fake, 2, fake, 2) == INV
        assert fwd(h, 0, 2, fake, 2, 2, fake, 2, fake, 2) == INV          # weighted
        assert fwd(h, 0, 1, fake, 2, -1, fake, 2, fake, 2) == INV         # k < 0
        assert fwd(h, 0, 1, fake, 1, 2, fake, 2, fake, 2) == INV          # ldx < k
        assert fwd(h, 0, 1, fake, 2, 2, fake, 1, fake, 2) == INV          # ldy < k
        assert fwd(h, 0, 1, fake, 2, 2, fake, 2, fake, 1) == INV          # ldarg < k with arg
        assert fwd(h, 0, 1, None, 2, 2, fake, 2, fake, 2) == INV          # null X
        assert fwd(h, 0, 1, fake, 2, 2, None, 2, fake, 2) == INV          # null Y
        assert bwd(h, 1, fake, 2, 2, fake, 2, fake, 2, None, 2, fake) == fmt
        assert bwd(h, 0, None, 2, 2, fake, 2, fake, 2, fake, 2, None) == fmt      # dX alone: X not needed; the format before the companion
        assert bwd(h, 1, fake, 2, 2, fake, 2, fake, 2, None, 2, None) == fmt      # nothing wanted
        assert bwd(None, 1, fake, 2, 2, fake, 2, fake, 2, fake, 2, fake) == INV
        assert bwd(h, 2, fake, 2, 2, fake, 2, fake, 2, fake, 2, None) == INV      # weighted
        assert bwd(h, 1, fake, 2, -1, fake, 2, fake, 2, fake, 2, fake) == INV     # k < 0
        for bad in range(4):                                                       # each leading dimension below k
            lds = [2, 2, 2, 2]
            lds[bad] = 1
            assert bwd(h, 1, fake, lds[0], 2, fake, lds[1], fake, lds[2], fake, lds[3], fake) == INV
        assert bwd(h, 1, None, 2, 2, fake, 2, fake, 2, None, 2, fake) == INV      # null X while dval is wanted
        assert bwd(h, 1, fake, 2, 2, None, 2, fake, 2, fake, 2, fake) == INV      # null dY
        assert bwd(h, 1, fake, 2, 2, fake, 2, None, 2, fake, 2, fake) == INV      # null arg
        assert bwd(h, 0, fake, 2, 2, fake, 2, fake, 2, fake, 2, fake) == INV      # dval with weighted = 0
        if stage == "before inputCSR":
            assert lib.csr5hip_input_csr(h, 100, None, None, None) == 0
    assert lib.csr5hip_free(h) == 0


def test_the_companion_message_names_build_transpose():
    with open(os.path.join(ROOT, "benchmark_spmv_using_csr5_amd", "csrc", "csr5_capi.hip")) as f:
        text = f.read()
    assert "csr5hip_spmm_reduce_backward: dX needs the transposed companion, call csr5hip_build_transpose first" in text


# ---- the Python layers ---------------------------------------------------------------------------------------------------------------
def test_python_wrappers_reject_bad_tensors_before_the_library():
    torch = pytest.importorskip("torch")
    A = H.anonymouslibHandle(6, 4)
    A._nnz = 9
    calls = []
    A.spmm_reduce_ptr = lambda *a: calls.append(a) or 0  # nothing may reach the library
    A.spmm_reduce_backward_ptr = lambda *a: calls.append(a) or 0
    f64, i32 = torch.float64, torch.int32
    X, Y, arg = torch.zeros(4, 3, dtype=f64), torch.zeros(6, 3, dtype=f64), torch.zeros(6, 3, dtype=i32)
    dX, dVal = torch.zeros(4, 3, dtype=f64), torch.zeros(9, dtype=f64)
    with pytest.raises(ValueError, match="GPU"):
        A.spmmReduce(X, Y, "max", arg)                                               # host tensors
    with pytest.raises(ValueError, match="'max' or 'min'"):
        A.spmmReduce(X, Y, "mean", arg)
    with pytest.raises(ValueError, match="dtype"):
        A.spmmReduce(X.float(), Y, "max", arg)
    with pytest.raises(ValueError, match="dtype"):
        A.spmmReduce(X, Y, "max", arg.long())                                        # arg must be int32
    with pytest.raises(ValueError):
        A.spmmReduce(np.zeros((4, 3)), Y)                                            # not a tensor
    with pytest.raises(ValueError, match="shape"):
        A.spmmReduce(torch.zeros(5, 3, dtype=f64), Y)
    with pytest.raises(ValueError, match="shape"):
        A.spmmReduce(X, torch.zeros(6, 2, dtype=f64))                                # another k
    with pytest.raises(ValueError, match="shape"):
        A.spmmReduce(X, Y, "min", torch.zeros(6, 4, dtype=i32))
    with pytest.raises(ValueError, match="stride"):
        A.spmmReduce(torch.zeros(3, 4, dtype=f64).t(), Y)                            # column-major X
    with pytest.raises(ValueError, match="stride"):
        A.spmmReduce(X, Y, "max", torch.zeros(3, 6, dtype=i32).t())
    with pytest.raises(ValueError, match="GPU"):
        A.spmmReduceBackward(X, Y, arg, dX, dVal)
    with pytest.raises(ValueError, match="dtype"):
        A.spmmReduceBackward(X, Y, arg.long(), dX, dVal)
    with pytest.raises(ValueError, match="shape"):
        A.spmmReduceBackward(X, Y, arg, torch.zeros(4, 2, dtype=f64), None)
    with pytest.raises(ValueError, match="weighted"):
        A.spmmReduceBackward(X, Y, arg, None, dVal, weighted=False)
    with pytest.raises(ValueError, match="needs X"):
        A.spmmReduceBackward(None, Y, arg, None, dVal)
    with pytest.raises(ValueError, match="shape"):
        A.spmmReduceBackward(X, Y, arg, None, torch.zeros(8, dtype=f64))             # dVal holds nnz values
    assert calls == []
    A.close()


def test_overlap_is_rejected():
    torch = pytest.importorskip("torch")
    buf = torch.zeros(6, 8, dtype=torch.float64)
    with pytest.raises(ValueError, match="aliased"):
        H.anonymouslibHandle._reduce_apart("spmmReduce", [("Y", buf[:, :3]), ("arg", None)], [("X", buf[:4, 4:7])])
    with pytest.raises(ValueError, match="aliased"):
        H.anonymouslibHandle._reduce_apart("spmmReduceBackward", [("dX", buf[:4, :3]), ("dVal", buf.view(-1)[:9])], [("dY", torch.zeros(6, 3))])
    with pytest.raises(ValueError, match="GPU"):  # (apart, and then judged for their device)
        H.anonymouslibHandle._reduce_apart("spmmReduce", [("Y", torch.zeros(6, 3)), ("arg", None)], [("X", torch.zeros(4, 3))])


def test_autograd_exports_spmm_reduce():
    from benchmark_spmv_using_csr5_amd import autograd
    assert "spmm_reduce" in autograd.__all__ and callable(autograd.spmm_reduce)


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
def _small_matrices():
    keep = ("kat0", "tiny-p1", "dense16", "nonsquare", "hub", "aligned64", "single-nnz")
    return [m for m in zoo.small_zoo() if m.name in keep] + [S.duplicates_matrix()]


@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("fp64", "fp32"))
def test_reference_against_torch_cpu(dtype):
    """values bit for bit torch's scatter_reduce_("amax" / "amin") of the same products; Y is t[arg] bitwise; rows without entries"""
    torch = pytest.importorskip("torch")
    for mat in _small_matrices():
        rng = np.random.default_rng([3, mat.nnz])
        val = R.distinct_values(mat.nnz, dtype)
        X = rng.uniform(-1, 1, size=(mat.n, 5)).astype(dtype)
        rows = torch.from_numpy(R.rows_of(mat))
        for weighted in (True, False):
            t = R.terms(mat, val, X, weighted)
            for op, name in (("max", "amax"), ("min", "amin")):
                Y, arg = R.forward(mat, val, X, op, weighted)
                want = torch.zeros((mat.m, 5), dtype=torch.from_numpy(X).dtype)
                want.scatter_reduce_(0, rows[:, None].expand(-1, 5), torch.from_numpy(t), name, include_self=False)
                assert R.same_bits(Y, want.numpy()), (mat.name, op, weighted)
                has = np.diff(mat.row_ptr) > 0
                assert (arg[~has] == -1).all() and not Y[~has].view(np.uint8).any()
                lo, hi = mat.row_ptr[:-1][has, None], mat.row_ptr[1:][has, None]
                assert ((arg[has] >= lo) & (arg[has] < hi)).all()
                assert R.same_bits(Y[has], t[arg[has], np.arange(5)[None, :]])


def test_reference_ties_go_to_the_smallest_rank():
    mat = S.duplicates_matrix()
    X = np.random.default_rng(4).integers(-2, 3, size=(mat.n, 5)).astype(np.float32)
    t = R.terms(mat, None, X, False)
    tied = 0
    for op in ("max", "min"):
        Y, arg = R.forward(mat, None, X, op, False)
        for i in range(mat.m):
            a, b = int(mat.row_ptr[i]), int(mat.row_ptr[i + 1])
            for c in range(5):
                if b > a:
                    same = np.flatnonzero(t[a:b, c] == Y[i, c])
                    tied += same.size > 1
                    assert arg[i, c] == a + same[0]
    assert tied > 50


def test_reference_specials():
    """NaN first and the first NaN; +Inf of smaller rank does not hide a NaN; a row of -Inf; +0 against -0; 0 * Inf"""
    inf, nan = np.inf, np.nan
    mat = M.CsrMatrix(5, 4, np.array([0, 3, 6, 8, 10, 10], dtype=np.int32), np.array([0, 1, 2, 1, 2, 3, 0, 3, 2, 0], dtype=np.int32),
                      np.ones(10), "specials")
    X = np.array([[inf, -inf, 0.0], [1.0, -inf, -0.0], [nan, -inf, -0.0], [nan, -inf, 5.0]])
    Y, arg = R.forward(mat, None, X, "max", False)
    assert arg[0].tolist() == [2, 0, 0]           # NaN beats the +Inf before it; all -Inf: the first entry; +0 == -0: rank decides ...
    assert np.isnan(Y[0, 0]) and Y[0, 1] == -inf and not np.signbit(Y[0, 2])  # ... and Y is that entry's value: +0, not the later -0
    assert arg[1].tolist() == [4, 3, 5]           # the FIRST NaN of two
    assert arg[2].tolist() == [7, 6, 7]
    assert arg[4].tolist() == [-1, -1, -1] and not Y[4].view(np.uint8).any()
    Ymin, argmin = R.forward(mat, None, X, "min", False)
    assert argmin[0].tolist() == [2, 0, 0] and not np.signbit(Ymin[0, 2])     # min: +0 == -0 too, rank 0 holds +0
    val = np.array([0.0, 1, 1, 1, 1, 1, 1, 1, 1, 1])
    Yw, argw = R.forward(mat, val, X, "max", True)
    assert argw[0, 0] == 0 and np.isnan(Yw[0, 0])                              # 0 * Inf = NaN, the first NaN of the row now
    d = R.dval(mat, X, np.ones((5, 3)), np.full((5, 3), 99, dtype=np.int32))
    assert not d.view(np.uint8).any()                                          # a corrupt arg matches nothing


def test_reference_dval_is_the_fma_chain():
    assert R.fma(np.float32(1 + 2 ** -12), np.float32(1 + 2 ** -12), np.float32(-1), np.float32) == np.float32(2 ** -11 + 2 ** -24)
    assert R.fma(1 + 2.0 ** -30, 1 + 2.0 ** -30, -1.0, np.float64) == 2.0 ** -29 + 2.0 ** -60
    mat = S.duplicates_matrix()
    rng = np.random.default_rng(8)
    X, dY = rng.integers(-8, 9, size=(mat.n, 4)).astype(np.float64), rng.integers(-8, 9, size=(mat.m, 4)).astype(np.float64)
    val = R.distinct_values(mat.nnz, np.float64)
    _, arg = R.forward(mat, val, X, "max", True)
    got = R.dval(mat, X, dY, arg)
    cols, rows = mat.col[:mat.nnz].astype(np.int64), R.rows_of(mat)
    want = ((arg[rows] == np.arange(mat.nnz)[:, None]) * X[cols] * dY[rows]).sum(1)  # integers: exact in any order
    assert np.array_equal(got, want)
    ref, w, mag = R.dx(mat, val, dY, arg, True)
    assert w.sum() == (np.diff(mat.row_ptr) > 0).sum() * 4                            # one winner per (row with entries, column)
    assert np.allclose(ref.sum(0), (val[:, None] * (arg[rows] == np.arange(mat.nnz)[:, None]) * dY[rows]).sum(0))


# ---- the kernel source on the CPU --------------------------------------------------------------------------------------------------------
def _sanitizers_link(cxx, tmp_path):
    src = tmp_path / "probe.cpp"
    src.write_text("#include <barrier>\nint main() { return 0; }\n")
    r = subprocess.run([cxx, "-std=c++20", "-fsanitize=address,undefined", str(src), "-o", str(tmp_path / "probe")], capture_output=True,
                       text=True)
    return r.returncode == 0 and subprocess.run([str(tmp_path / "probe")]).returncode == 0


def test_host_emulation_under_the_sanitizers(tmp_path):
    """scripts/host_emulation/run_spmm_reduce.py: a stand-alone program built from csr5_reduce.hip with -fsanitize=address,undefined;
    kat0 and duplicates, both precisions, max and min, weighted and not, k = 3 and 17; forward, dval and dx at sigma = 4, 7 and 16"""
    cxx = "/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else "clang++"
    try:
        linked = _sanitizers_link(cxx, tmp_path)
    except OSError:
        linked = False
    if not linked:
        pytest.skip(f"no host C++20 compiler: {cxx} cannot build and run a program with -fsanitize=address,undefined")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "host_emulation", "run_spmm_reduce.py"), "--matrices", "kat0,duplicates",
                        "--ks", "3,17", "--cxx", cxx], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.count(": ok") == 32 and r.stdout.count("duplicates") == 16 and r.stdout.count("unweighted 17: ok") == 8, r.stdout
