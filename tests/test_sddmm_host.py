"""sddmm on the host side (no GPU): the reference of tests/sddmm_reference.py against a dense product, the C ABI symbol and its
declaration, the C++ class member, the return codes and their order, and the Python argument checks."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from benchmark_spmv_using_csr5_amd import _capi
from benchmark_spmv_using_csr5_amd import handle as H
from tests import sddmm_reference as S
from tests import zoo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
DECL = "int csr5hip_sddmm(csr5hip_handle h, const void *d_U, int ldu, const void *d_V, int ldv, int k, void *d_out_csr);"


@pytest.mark.parametrize("dtype", S.DTYPES, ids=("fp64", "fp32"))
def test_reference_equals_dense_product_sampled_at_the_pattern(dtype):
    for mat in list(zoo.small_zoo()) + [S.duplicates_matrix()]:
        for k in (0, 1, 5, 13):
            U, V = S.make("integer", mat, k, dtype, seed=3)
            ref = S.reference("integer", mat, U, V)
            dense = U.astype(np.float64) @ V.astype(np.float64).T  # (m, n), exact on integer data
            want = dense[S.rows_of(mat), mat.col[:mat.nnz]]
            assert (ref.bound < 0).all() and np.array_equal(ref.expected, want), (mat.name, k)
            S.check(want.astype(dtype), ref, f"{mat.name} k {k}")


def test_reference_rules_on_hard_data():
    mat = S.duplicates_matrix()
    rows, cols = S.rows_of(mat), mat.col[:mat.nnz]
    for dtype in S.DTYPES:
        U, V = S.make("nonfinite", mat, 8, dtype, seed=1)
        assert not np.isfinite(U[0]).all() and not np.isfinite(V[0]).all()
        ref = S.reference("nonfinite", mat, U, V)
        clean = np.isfinite(U[rows]).all(axis=1) & np.isfinite(V[cols]).all(axis=1)
        assert clean.any() and (~clean).any()
        assert np.isfinite(ref.expected[clean]).all() and not np.isfinite(ref.expected[~clean]).any()
        out = ref.expected.astype(dtype)
        S.check(out, ref)
        out[np.flatnonzero(clean)[0]] += 1
        assert S.bad_elements(out, ref).tolist() == [int(np.flatnonzero(clean)[0])]
        for dataset in ("row_scaled", "subnormal"):
            U, V = S.make(dataset, mat, 13, dtype, seed=2)
            ref = S.reference(dataset, mat, U, V)
            S.check(ref.expected.astype(dtype), ref, dataset)
            assert np.count_nonzero(ref.expected) > mat.nnz // 2
        tiny = float(np.finfo(dtype).tiny)
        assert 0 < np.abs(ref.expected[ref.expected != 0]).max() < tiny  # (subnormal sums)
        U, V = S.make("wide_range", mat, 40, dtype, seed=4)
        ref = S.reference("wide_range", mat, U, V)
        assert (ref.bound > 0).all()
        with np.errstate(over="ignore"):
            naive = (U[rows] * V[cols]).sum(axis=1, dtype=dtype)  # some summation order in the working precision
        S.check(naive.astype(dtype), ref, "wide_range, numpy's own order")
        assert S.bad_elements((naive * dtype(1.001)).astype(dtype), ref).size > 0


def test_library_exports_sddmm_with_the_declared_signature():
    import torch  # noqa: F401  (one HIP runtime per process: see _capi.load)
    lib = C.CDLL(_capi.LIB_PATH)
    assert hasattr(lib, "csr5hip_sddmm")
    with open(os.path.join(INC, "csr5hip.h")) as f:
        text = re.sub(r"\s+", " ", f.read())
    assert DECL in text
    bound = [(res, args) for name, res, args in _capi.SYMBOLS if name == "csr5hip_sddmm"]
    assert bound == [(C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p])]


def test_cpp_class_has_sddmm_member(tmp_path):
    src = tmp_path / "use_sddmm.cpp"
    src.write_text(
        '#include "anonymouslib_hip.h"\n'
        "int use(anonymouslibHandle<int, unsigned, double> &A, const double *U, const double *V, double *out)\n"
        "{ return A.sddmm(U, 4, V, 5, 4, out); }\n"
        "int use32(anonymouslibHandle<int, unsigned, float> &A, const float *U, const float *V, float *out)\n"
        "{ return A.sddmm(U, 2, V, 2, 2, out); }\n")
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", f"-I{INC}", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _info_bytes(lib, h):
    info = _capi.Csr5Info()
    assert lib.csr5hip_get_info(h, C.byref(info)) == 0
    return bytes(info)


def test_sddmm_return_codes_in_order_without_a_gpu():
    """Decided on the host: bad arguments first, then the CSR format, then the missing matrix; get_info unchanged throughout."""
    lib = _capi.load()
    h = C.c_void_p()
    assert lib.csr5hip_create(C.byref(h), 10, 10, _capi.F64) == 0
    fake = C.c_void_p(64)
    before = _info_bytes(lib, h)
    assert lib.csr5hip_sddmm(h, fake, 2, fake, 2, 2, fake) == _capi.UNKOWN_FORMAT      # before inputCSR
    assert lib.csr5hip_sddmm(h, fake, 2, fake, 2, -1, fake) == _capi.INVALID_ARGUMENT  # k < 0
    assert lib.csr5hip_sddmm(h, fake, 1, fake, 2, 2, fake) == _capi.INVALID_ARGUMENT   # ldu < k
    assert lib.csr5hip_sddmm(h, fake, 2, fake, 1, 2, fake) == _capi.INVALID_ARGUMENT   # ldv < k
    assert lib.csr5hip_sddmm(None, fake, 2, fake, 2, 2, fake) == _capi.INVALID_ARGUMENT
    assert _info_bytes(lib, h) == before
    assert lib.csr5hip_input_csr(h, 100, None, None, None) == 0
    before = _info_bytes(lib, h)
    assert lib.csr5hip_sddmm(h, fake, 2, fake, 2, 2, fake) == _capi.UNSUPPORTED_CSR_SPMV  # format is CSR
    assert lib.csr5hip_sddmm(h, fake, 0, fake, 0, 0, fake) == _capi.UNSUPPORTED_CSR_SPMV
    assert lib.csr5hip_sddmm(h, None, 0, None, 0, 0, fake) == _capi.UNSUPPORTED_CSR_SPMV  # k = 0 needs neither U nor V
    # arguments are judged before the format
    assert lib.csr5hip_sddmm(h, None, 2, fake, 2, 2, fake) == _capi.INVALID_ARGUMENT   # null U, k > 0, nnz > 0
    assert lib.csr5hip_sddmm(h, fake, 2, None, 2, 2, fake) == _capi.INVALID_ARGUMENT   # null V
    assert lib.csr5hip_sddmm(h, fake, 2, fake, 2, 2, None) == _capi.INVALID_ARGUMENT   # null out, nnz > 0
    assert lib.csr5hip_sddmm(h, None, 0, None, 0, 0, None) == _capi.INVALID_ARGUMENT   # null out even with k = 0
    assert lib.csr5hip_sddmm(h, fake, 1, fake, 2, 2, fake) == _capi.INVALID_ARGUMENT
    assert _info_bytes(lib, h) == before
    assert lib.csr5hip_input_csr(h, 0, None, None, None) == 0
    assert lib.csr5hip_sddmm(h, None, 2, None, 2, 2, None) == _capi.UNSUPPORTED_CSR_SPMV  # nnz = 0: no pointer is needed
    assert lib.csr5hip_free(h) == 0


def test_python_sddmm_rejects_bad_tensors_before_the_library():
    torch = pytest.importorskip("torch")
    A = H.anonymouslibHandle(6, 4)
    calls = []
    A.sddmm_ptr = lambda *a: calls.append(a) or 0  # nothing may reach the library
    f64 = torch.float64
    U, V, out = torch.zeros(6, 3, dtype=f64), torch.zeros(4, 3, dtype=f64), torch.zeros(7, dtype=f64)
    with pytest.raises(ValueError, match="inputCSR"):
        A.sddmm(U, V, out)
    assert A.inputCSR(7, None, None, None) == 0
    with pytest.raises(ValueError, match="GPU"):
        A.sddmm(U, V, out)                                                    # host tensors
    with pytest.raises(ValueError, match="dtype"):
        A.sddmm(U.float(), V, out)
    with pytest.raises(ValueError, match="dtype"):
        A.sddmm(U, V, out.float())
    with pytest.raises(ValueError):
        A.sddmm(np.zeros((6, 3)), V, out)                                     # not a tensor
    with pytest.raises(ValueError, match="shape"):
        A.sddmm(torch.zeros(5, 3, dtype=f64), V, out)                         # U has m rows
    with pytest.raises(ValueError, match="shape"):
        A.sddmm(U, torch.zeros(6, 3, dtype=f64), out)                         # V has n rows
    with pytest.raises(ValueError, match="columns"):
        A.sddmm(U, torch.zeros(4, 2, dtype=f64), out)
    with pytest.raises(ValueError, match="stride"):
        A.sddmm(torch.zeros(3, 6, dtype=f64).t(), V, out)                     # column-major U
    with pytest.raises(ValueError, match="shape"):
        A.sddmm(U, V, torch.zeros(8, dtype=f64))                              # out is not nnz long
    with pytest.raises(ValueError, match="shape"):
        A.sddmm(U, V, torch.zeros(7, 1, dtype=f64))
    with pytest.raises(ValueError, match="contiguous"):
        A.sddmm(U, V, torch.zeros(14, dtype=f64)[::2])
    big = torch.zeros(6 * 3 + 7, dtype=f64)
    with pytest.raises(ValueError, match="aliased"):
        A.sddmm(big[:18].view(6, 3), V, big[18:])                             # out in U's storage
    big = torch.zeros(4 * 3 + 7, dtype=f64)
    with pytest.raises(ValueError, match="aliased"):
        A.sddmm(U, big[7:].view(4, 3), big[:7])                               # out in V's storage
    assert calls == []
    A.close()


def test_autograd_module_imports_without_a_gpu():
    from benchmark_spmv_using_csr5_amd import autograd
    assert callable(autograd.spmm)
