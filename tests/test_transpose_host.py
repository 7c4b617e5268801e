"""The transposed product on the host side (no GPU): ``matrices.transpose_csr`` -- the independent statement of the canonical
A^T that csr5hip_build_transpose builds on the device --, the three C ABI symbols and their declarations, the C++ class members,
the return codes decided before any device work, the appended csr5hip_info fields and the Python argument checks."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from benchmark_spmv_using_csr5_amd import _capi
from benchmark_spmv_using_csr5_amd import handle as H
from benchmark_spmv_using_csr5_amd import matrices as M
from tests import zoo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")


def _dense(mat, val):
    """duplicates of one (row, column) pair add up"""
    D = np.zeros((mat.m, mat.n))
    rows = np.repeat(np.arange(mat.m), np.diff(mat.row_ptr))
    np.add.at(D, (rows, mat.col[:mat.nnz]), val)
    return D


def _duplicates_matrix():
    # row 0 holds (0, 2) three times and row 2 holds (2, 1) twice, unsorted columns
    row_ptr = np.array([0, 5, 5, 9], dtype=np.int32)
    col = np.array([2, 0, 2, 3, 2, 1, 3, 1, 0], dtype=np.int32)
    return M.CsrMatrix(3, 4, row_ptr, col, np.arange(1.0, 10.0), "duplicates")


def test_transpose_csr_is_the_canonical_transpose():
    rng = np.random.default_rng(3)
    for mat in list(zoo.small_zoo()) + [zoo.empty_matrix(), _duplicates_matrix()]:
        val = rng.integers(1, 1000, size=mat.nnz).astype(np.float64)  # integers: the dense sums are exact
        A = M.CsrMatrix(mat.m, mat.n, mat.row_ptr, mat.col, val, mat.name)
        T, src = M.transpose_csr(A, return_map=True)
        assert (T.m, T.n, T.nnz) == (mat.n, mat.m, mat.nnz)
        assert T.row_ptr.shape == (mat.n + 1,) and T.row_ptr[0] == 0 and (np.diff(T.row_ptr) >= 0).all()
        assert np.array_equal(np.sort(src), np.arange(mat.nnz)), mat.name          # a permutation
        assert np.array_equal(T.val, val[src]), mat.name
        plain = M.transpose_csr(A)
        assert np.array_equal(plain.row_ptr, T.row_ptr) and np.array_equal(plain.col, T.col) and np.array_equal(plain.val, T.val)
        if mat.m * mat.n <= 4_000_000:
            assert np.array_equal(_dense(T, T.val), _dense(A, val).T), mat.name
        # row j of A^T: A's entries of column j in ascending order of their position in A's arrays
        rows_T = np.repeat(np.arange(T.m), np.diff(T.row_ptr))
        assert np.array_equal(mat.col[:mat.nnz][src], rows_T), mat.name
        same_row = rows_T[1:] == rows_T[:-1]
        assert (np.diff(src)[same_row] > 0).all(), mat.name
        rows_A = np.repeat(np.arange(mat.m), np.diff(mat.row_ptr))
        assert np.array_equal(T.col, rows_A[src]), mat.name


def test_duplicates_keep_the_order_they_have_in_a():
    A = _duplicates_matrix()
    T, src = M.transpose_csr(A, return_map=True)
    assert T.row_ptr.tolist() == [0, 2, 4, 7, 9]
    assert T.col.tolist() == [0, 2, 2, 2, 0, 0, 0, 0, 2]
    assert src.tolist() == [1, 8, 5, 7, 0, 2, 4, 3, 6]
    assert T.val.tolist() == [2.0, 9.0, 6.0, 8.0, 1.0, 3.0, 5.0, 4.0, 7.0]


def test_transposing_twice_gives_back_a_column_sorted_matrix():
    for mat in list(zoo.small_zoo()) + [zoo.empty_matrix()]:
        # sort every row by column (stable: duplicates keep their order)
        rows = np.repeat(np.arange(mat.m), np.diff(mat.row_ptr))
        order = np.lexsort((np.arange(mat.nnz), mat.col[:mat.nnz], rows))
        val = np.arange(mat.nnz, dtype=np.float64)
        A = M.CsrMatrix(mat.m, mat.n, mat.row_ptr, mat.col[:mat.nnz][order], val, mat.name)
        B = M.transpose_csr(M.transpose_csr(A))
        assert (B.m, B.n) == (A.m, A.n)
        assert np.array_equal(B.row_ptr, A.row_ptr) and np.array_equal(B.col, A.col) and np.array_equal(B.val, A.val), mat.name


def test_library_exports_the_transpose_calls_with_the_declared_signatures():
    import torch  # noqa: F401  (one HIP runtime per process: see _capi.load)
    lib = C.CDLL(_capi.LIB_PATH)
    with open(os.path.join(INC, "csr5hip.h")) as f:
        text = re.sub(r"\s+", " ", f.read())
    p, i = C.c_void_p, C.c_int
    for name, decl, args in (
            ("csr5hip_build_transpose", "int csr5hip_build_transpose(csr5hip_handle h);", [p]),
            ("csr5hip_spmv_t", "int csr5hip_spmv_t(csr5hip_handle h, const void *d_x, void *d_y);", [p, p, p]),
            ("csr5hip_spmm_t", "int csr5hip_spmm_t(csr5hip_handle h, const void *d_X, int ldx, int k, void *d_Y, int ldy);",
             [p, p, i, i, p, i])):
        assert hasattr(lib, name)
        assert decl in text
        assert [(n, r, a) for n, r, a in _capi.SYMBOLS if n == name] == [(name, C.c_int, args)]


def test_cpp_class_has_the_transpose_members(tmp_path):
    src = tmp_path / "use_transpose.cpp"
    src.write_text(
        '#include "anonymouslib_hip.h"\n'
        "int use(anonymouslibHandle<int, unsigned, double> &A, const double *x, double *y)\n"
        "{ return A.buildTranspose() + A.spmvT(x, y) + A.spmmT(x, 3, 3, y, 4); }\n"
        "int use32(anonymouslibHandle<int, unsigned, float> &A, const float *x, float *y)\n"
        "{ return A.buildTranspose() + A.spmvT(x, y) + A.spmmT(x, 3, 3, y, 4); }\n")
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", f"-I{INC}", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# csr5hip_info as it was before the transposed product: the new fields are appended behind `stream_nt`, none moved
_OLD_FIELDS = ["format", "m", "n", "nnz", "value_type", "omega", "sigma", "bit_y_offset", "bit_scansum_offset", "num_packet", "p",
               "tail_partition_start", "num_offsets", "d_tile_ptr", "d_tile_desc", "d_offset_ptr", "d_offset", "x_window_tiles",
               "x_window_active", "x_window_cover_pct", "x_window_lines", "t_malloc_ms", "t_tile_ptr_ms", "t_tile_desc_ms",
               "t_transpose_ms", "column_slabs", "slab_shift", "slab_segments", "slab_sigma", "slab_tiles", "t_slab_ms", "slab_hot",
               "slab_hot_cover_pct", "slab_fallback", "device_bytes", "slab_x_permuted", "slab_cold_entries", "x_snapshot",
               "slab_values_narrowed", "carries_deferred", "narrow_columns", "flagged_columns", "lds_y", "stream_nt"]
_NEW_FIELDS = ["transpose_built", "t_transpose_build_ms", "t_sigma", "t_p", "t_tail_partition_start", "t_column_slabs", "t_slab_hot",
               "t_x_window_active"]


def test_info_fields_are_appended_in_header_and_binding():
    names = [f[0] for f in _capi.Csr5Info._fields_]
    assert names == _OLD_FIELDS + _NEW_FIELDS
    with open(os.path.join(INC, "csr5hip.h")) as f:
        text = f.read()
    body = text[text.index("typedef struct csr5hip_info {"):text.index("} csr5hip_info;")]
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    declared = []
    for stmt in body.split("{", 1)[1].split(";"):
        stmt = stmt.strip()
        if stmt:
            first, *rest = stmt.split(",")
            declared += [re.sub(r"[\s*]", "", first.split()[-1])] + [re.sub(r"[\s*]", "", r) for r in rest]
    assert declared == names
    assert _capi.Csr5Info.stream_nt.offset + 4 <= _capi.Csr5Info.transpose_built.offset


def test_transpose_return_codes_without_a_gpu():
    """Decided on the host: the handle and the pointers, then the format, then whether a companion exists."""
    lib = _capi.load()
    x, y = C.c_void_p(1 << 20), C.c_void_p(1 << 21)  # made-up device addresses: never dereferenced
    assert lib.csr5hip_build_transpose(None) == _capi.INVALID_ARGUMENT
    assert lib.csr5hip_spmv_t(None, x, y) == _capi.INVALID_ARGUMENT
    assert lib.csr5hip_spmm_t(None, x, 2, 2, y, 2) == _capi.INVALID_ARGUMENT
    h = C.c_void_p()
    assert lib.csr5hip_create(C.byref(h), 10, 7, _capi.F64) == 0
    info = _capi.Csr5Info()

    def check_info(fmt, nnz):
        assert lib.csr5hip_get_info(h, C.byref(info)) == 0
        assert (info.m, info.n, info.nnz, info.omega, info.format, info.value_type) == (10, 7, nnz, 64, fmt, _capi.F64)
        assert info.sigma == (lib.csr5hip_auto_sigma(10, nnz, _capi.F64) if fmt == _capi.FORMAT_CSR else 0)
        assert info.transpose_built == 0 and info.t_transpose_build_ms == 0.0
        assert (info.t_sigma, info.t_p, info.t_tail_partition_start) == (0, 0, 0)
        assert (info.t_column_slabs, info.t_slab_hot, info.t_x_window_active) == (0, 0, 0)
        assert info.device_bytes == 0 and info.column_slabs == 0 and info.p == 0

    # before inputCSR
    check_info(-1, 0)
    assert lib.csr5hip_build_transpose(h) == _capi.UNKOWN_FORMAT
    assert lib.csr5hip_spmv_t(h, x, y) == _capi.UNKOWN_FORMAT
    assert lib.csr5hip_spmm_t(h, x, 2, 2, y, 2) == _capi.UNKOWN_FORMAT
    assert lib.csr5hip_spmv_t(h, None, y) == _capi.INVALID_ARGUMENT
    assert lib.csr5hip_spmv_t(h, x, None) == _capi.INVALID_ARGUMENT
    # CSR format
    assert lib.csr5hip_input_csr(h, 100, None, None, None) == 0
    assert lib.csr5hip_set_sigma(h, _capi.AUTO_TUNED_SIGMA) == 0
    check_info(_capi.FORMAT_CSR, 100)
    assert lib.csr5hip_build_transpose(h) == _capi.UNSUPPORTED_CSR_SPMV
    assert lib.csr5hip_spmv_t(h, x, y) == _capi.UNSUPPORTED_CSR_SPMV
    assert lib.csr5hip_spmm_t(h, x, 2, 2, y, 2) == _capi.UNSUPPORTED_CSR_SPMV
    assert lib.csr5hip_spmm_t(h, x, 2, 0, y, 2) == _capi.UNSUPPORTED_CSR_SPMV
    # csr5hip_spmm's argument checks come first
    for ldx, k, ldy in ((1, 2, 2), (2, 2, 1), (2, -1, 2)):
        assert lib.csr5hip_spmm_t(h, x, ldx, k, y, ldy) == _capi.INVALID_ARGUMENT
    assert lib.csr5hip_spmm_t(h, None, 2, 2, y, 2) == _capi.INVALID_ARGUMENT
    assert lib.csr5hip_spmm_t(h, x, 2, 2, None, 2) == _capi.INVALID_ARGUMENT
    check_info(_capi.FORMAT_CSR, 100)
    assert lib.csr5hip_free(h) == 0


def test_python_transpose_calls_reject_bad_tensors_before_the_library():
    torch = pytest.importorskip("torch")
    A = H.anonymouslibHandle(6, 4)
    calls = []
    A.spmvT_ptr = lambda *a: calls.append(a) or 0  # nothing may reach the library
    A.spmmT_ptr = lambda *a: calls.append(a) or 0
    f64 = torch.float64
    with pytest.raises(ValueError, match="GPU"):
        A.spmvT(torch.zeros(6, dtype=f64), torch.zeros(4, dtype=f64))       # host tensors, otherwise right
    with pytest.raises(ValueError, match="shape"):
        A.spmvT(torch.zeros(4, dtype=f64), torch.zeros(6, dtype=f64))       # x has m values, y has n
    with pytest.raises(ValueError, match="shape"):
        A.spmvT(torch.zeros(6, 1, dtype=f64), torch.zeros(4, dtype=f64))
    with pytest.raises(ValueError, match="dtype"):
        A.spmvT(torch.zeros(6, dtype=torch.float32), torch.zeros(4, dtype=f64))
    with pytest.raises(ValueError, match="tensor"):
        A.spmvT(np.zeros(6), torch.zeros(4, dtype=f64))
    with pytest.raises(ValueError, match="contiguous"):
        A.spmvT(torch.zeros(12, dtype=f64)[::2], torch.zeros(4, dtype=f64))
    with pytest.raises(ValueError, match="GPU"):
        A.spmmT(torch.zeros(6, 3, dtype=f64), torch.zeros(4, 3, dtype=f64))
    with pytest.raises(ValueError, match="shape"):
        A.spmmT(torch.zeros(4, 3, dtype=f64), torch.zeros(6, 3, dtype=f64))  # X has m rows, Y has n
    with pytest.raises(ValueError, match="dtype"):
        A.spmmT(torch.zeros(6, 3, dtype=torch.float32), torch.zeros(4, 3, dtype=f64))
    with pytest.raises(ValueError, match="row-major"):
        A.spmmT(torch.zeros(3, 6, dtype=f64).t(), torch.zeros(4, 3, dtype=f64))
    assert calls == []
    A.close()
