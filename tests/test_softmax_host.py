"""row_softmax / row_softmax_grad on the host side (no GPU): the reference of tests/softmax_reference.py against a dense float64
softmax, what its bounds let through and what they catch, the C ABI symbols and their declarations, the C++ class members, the
return codes and their order, the Python argument checks and the autograd exports."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from benchmark_spmv_using_csr5_amd import _capi
from benchmark_spmv_using_csr5_amd import handle as H
from tests import sddmm_reference as S
from tests import softmax_reference as R
from tests import zoo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
DECLS = ("int csr5hip_row_softmax(csr5hip_handle h, const void *d_scores_csr, void *d_out_csr);",
         "int csr5hip_row_softmax_grad(csr5hip_handle h, const void *d_p_csr, const void *d_g_csr, void *d_out_csr);")


def _dense(mat, values):
    """(m, n) float64 with -Inf where nothing is stored; needs a pattern without repeated pairs"""
    D = np.full((mat.m, mat.n), -np.inf)
    D[S.rows_of(mat), mat.col[:mat.nnz]] = values
    return D


def _small():
    return [m for m in zoo.small_zoo() if m.nnz <= 20000 and m.m * m.n <= 4_000_000]


def test_reference_equals_a_dense_softmax_and_its_jacobian():
    mats = _small()
    assert len(mats) >= 3
    for mat in mats:
        rows, cols = S.rows_of(mat), mat.col[:mat.nnz]
        if np.unique(rows * mat.n + cols).size != mat.nnz:
            continue
        s = R.make_scores("gaussian", mat.row_ptr, np.float64, seed=1)
        D = _dense(mat, s)
        has = np.diff(mat.row_ptr) > 0
        with np.errstate(invalid="ignore"):
            E = np.exp(D - np.where(has, D.max(axis=1), 0.0)[:, None])
            P = E / np.where(has, E.sum(axis=1), 1.0)[:, None]
        ref = R.softmax_reference(mat.row_ptr, s)
        want = P[rows, cols]
        assert np.allclose(ref.expected.astype(np.float64), want, rtol=1e-13, atol=0), mat.name
        R.check(want, ref, mat.name)
        p, g = R.make_grad("softmax", mat.row_ptr, np.float64, seed=1)
        G = np.zeros((mat.m, mat.n))
        G[rows, cols] = g
        Pd = np.zeros((mat.m, mat.n))
        Pd[rows, cols] = p
        dS = Pd * (G - (Pd * G).sum(axis=1)[:, None])
        gref = R.grad_reference(mat.row_ptr, p, g)
        assert np.allclose(gref.expected.astype(np.float64), dS[rows, cols], rtol=1e-11, atol=1e-15), mat.name
        R.check(dS[rows, cols], gref, mat.name)


def _long_rows(seed, count=60):
    rng = np.random.default_rng(seed)
    lens = np.concatenate([[1, 2, 3, 0, 100000], np.exp(rng.uniform(0, np.log(30000), size=count)).astype(np.int64)])
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=("fp64", "fp32"))
def test_bounds_pass_a_working_precision_softmax_and_catch_a_perturbation(dtype):
    """A plain numpy softmax in the working precision, exp(s - max) / sum with numpy's own summation order, stays inside the
    forward bound on rows of 1 to 100 000 entries and spans up to the dataset's; the same for the gradient; a relative
    perturbation of 1e-3 of one element is caught at exactly that element (in rows of at most 1 000 entries: gamma(L - 1) of the
    100 000-entry row is 6e-3 in fp32, the bound of ANY summation order there)."""
    rp = _long_rows(3)
    lens, starts, nlens, rows = R._rows(rp)
    for dataset in ("gaussian", "wide", "shifted"):
        s = R.make_scores(dataset, rp, dtype, seed=2)
        M = np.repeat(np.maximum.reduceat(s, starts), nlens)
        with np.errstate(under="ignore"):
            e = np.exp(s - M)
            Z = np.array([e[a:a + n].sum(dtype=dtype) for a, n in zip(starts, nlens)], dtype=dtype)
            out = (e / np.repeat(Z, nlens)).astype(dtype)
        ref = R.softmax_reference(rp, s, dataset)
        R.check(out, ref, dataset)
        worst = R.ratios(out, ref).max()
        assert 0 < worst <= 1, (dataset, worst)
        sel = np.flatnonzero((ref.kind == R.BOUND) & (ref.expected > 1e-6) & (np.repeat(nlens, nlens) <= 1000))
        assert sel.size
        for i in sel[[0, sel.size // 2, -1]].tolist():
            hurt = out.copy()
            hurt[i] *= dtype(1.001)
            assert R.bad_elements(hurt, ref).tolist() == [i], (dataset, i)
    p, g = R.make_grad("softmax", rp, dtype, seed=2)
    pg = p * g
    D = np.array([pg[a:a + n].sum(dtype=dtype) for a, n in zip(starts, nlens)], dtype=dtype)
    out = (p * (g - np.repeat(D, nlens))).astype(dtype)
    ref = R.grad_reference(rp, p, g)
    R.check(out, ref, "gradient")
    big = np.flatnonzero((np.abs(ref.expected) > 1e-3 * np.abs(ref.expected).max()) & (np.repeat(nlens, nlens) <= 1000))
    i = int(big[big.size // 2])
    hurt = out.copy()
    hurt[i] *= dtype(1.001)
    assert R.bad_elements(hurt, ref).tolist() == [i]


@pytest.mark.parametrize("dtype", R.DTYPES, ids=("fp64", "fp32"))
def test_reference_rules_on_special_data(dtype):
    mat = S.duplicates_matrix()
    rp = mat.row_ptr
    lens, starts, nlens, rows = R._rows(rp)
    L = np.repeat(nlens, nlens)
    # uniform: exactly 1 / L, and a softmax without the subtraction of the maximum is caught
    s = R.make_scores("uniform", rp, dtype, seed=4)
    ref = R.softmax_reference(rp, s, "uniform")
    assert (ref.kind == R.EXACT).all()
    R.check((dtype(1) / L.astype(dtype)).astype(dtype), ref, "uniform")
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(s)
        naive = (e / np.repeat(np.add.reduceat(e, starts), nlens)).astype(dtype)
    assert R.bad_elements(naive, ref).size > 0
    # shifted: the pair has the same reference
    a, b = R.shifted_pair(rp, dtype, seed=4)
    ra, rb = R.softmax_reference(rp, a, "shifted"), R.softmax_reference(rp, b, "shifted")
    assert np.array_equal(ra.expected, rb.expected) and not np.array_equal(a, b)
    # masked: +0 for -Inf, NaN for the row of -Inf only, 1 for the single survivor
    s = R.make_scores("masked", rp, dtype, seed=4)
    ref = R.softmax_reference(rp, s, "masked")
    assert (ref.kind[np.isneginf(s) & (ref.kind != R.ALLNAN)] == R.EXACT).all()
    nan_rows = np.unique(rows[ref.kind == R.ALLNAN])
    assert nan_rows.size >= 1 and all(np.isneginf(s[rp[r]:rp[r + 1]]).all() for r in nan_rows)
    ones = np.flatnonzero((ref.kind == R.EXACT) & (ref.expected == 1))
    assert any(lens[rows[i]] >= 2 for i in ones)
    good = ref.expected.astype(dtype)
    good[ref.kind == R.ALLNAN] = np.nan
    R.check(good, ref, "masked")
    neg = good.copy()
    z = np.flatnonzero(np.isneginf(s) & (ref.kind == R.EXACT))[0]
    neg[z] = -0.0
    assert R.bad_elements(neg, ref).tolist() == [int(z)]           # -0 is not +0
    # nonfinite: the first non-empty row is poisoned, whole rows and nothing else
    s = R.make_scores("nonfinite", rp, dtype, seed=4)
    ref = R.softmax_reference(rp, s, "nonfinite")
    bad_rows = np.unique(rows[~np.isfinite(s)])
    assert bad_rows[0] == np.flatnonzero(lens > 0)[0]
    assert np.array_equal(ref.kind == R.ALLNAN, np.isin(rows, bad_rows))
    good = ref.expected.astype(dtype)
    R.check(good, ref, "nonfinite")
    leak = good.copy()
    first_clean = np.flatnonzero(ref.kind != R.ALLNAN)[0]
    leak[first_clean] = np.nan
    assert R.bad_elements(leak, ref).tolist() == [int(first_clean)]
    # gradient: exact data are exact; NaN in g poisons whole rows only
    p, g = R.make_grad("exact", rp, dtype, seed=4)
    ref = R.grad_reference(rp, p, g, "exact")
    assert (ref.kind == R.EXACT).all()
    R.check(ref.expected.astype(dtype), ref, "exact")
    p, g = R.make_grad("nonfinite", rp, dtype, seed=4)
    ref = R.grad_reference(rp, p, g, "nonfinite")
    assert np.array_equal(ref.kind == R.ALLNAN, np.isin(rows, np.unique(rows[np.isnan(g)])))
    assert 0 < (ref.kind == R.ALLNAN).sum() < ref.kind.size
    assert 1 <= R.C_EXP[dtype] <= 8


def test_hub_matrix_has_the_rows_the_kernel_classes_need():
    mat = R.hub_matrix()
    lens = np.diff(mat.row_ptr)
    assert lens.max() >= 200000 and set((0, 1, 2, 3, 63, 64, 65)) <= set(lens.tolist())
    p, g = R.make_grad("exact", mat.row_ptr, np.float32, seed=1)   # (asserts that the exact dataset stays exact on the hub row)
    R.grad_reference(mat.row_ptr, p, g, "exact")


def test_library_exports_both_symbols_with_the_declared_signatures():
    import torch  # noqa: F401  (one HIP runtime per process: see _capi.load)
    lib = C.CDLL(_capi.LIB_PATH)
    assert hasattr(lib, "csr5hip_row_softmax") and hasattr(lib, "csr5hip_row_softmax_grad")
    with open(os.path.join(INC, "csr5hip.h")) as f:
        text = re.sub(r"\s+", " ", f.read())
    for decl in DECLS:
        assert decl in text
    bound = {name: (res, args) for name, res, args in _capi.SYMBOLS if name.startswith("csr5hip_row_softmax")}
    assert bound == {"csr5hip_row_softmax": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
                     "csr5hip_row_softmax_grad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])}


def test_cpp_class_has_the_row_softmax_members(tmp_path):
    src = tmp_path / "use_row_softmax.cpp"
    src.write_text(
        '#include "anonymouslib_hip.h"\n'
        "int use(anonymouslibHandle<int, unsigned, double> &A, const double *s, const double *g, double *out)\n"
        "{ return A.rowSoftmax(s, out) + A.rowSoftmaxGrad(s, g, out); }\n"
        "int use32(anonymouslibHandle<int, unsigned, float> &A, const float *s, const float *g, float *out)\n"
        "{ return A.rowSoftmax(s, out) + A.rowSoftmaxGrad(s, g, out); }\n")
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", f"-I{INC}", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _info_bytes(lib, h):
    info = _capi.Csr5Info()
    assert lib.csr5hip_get_info(h, C.byref(info)) == 0
    return bytes(info)


def test_return_codes_in_order_without_a_gpu():
    """Decided on the host: the null handle and null pointers first, then the missing matrix; nnz = 0 succeeds with null pointers
    and touches no device; get_info unchanged throughout."""
    lib = _capi.load()
    h = C.c_void_p()
    assert lib.csr5hip_create(C.byref(h), 10, 10, _capi.F64) == 0
    fake = C.c_void_p(64)
    before = _info_bytes(lib, h)
    assert lib.csr5hip_row_softmax(None, fake, fake) == _capi.INVALID_ARGUMENT
    assert lib.csr5hip_row_softmax_grad(None, fake, fake, fake) == _capi.INVALID_ARGUMENT
    assert lib.csr5hip_row_softmax(h, fake, fake) == _capi.UNKOWN_FORMAT               # before inputCSR
    assert lib.csr5hip_row_softmax_grad(h, fake, fake, fake) == _capi.UNKOWN_FORMAT
    assert lib.csr5hip_row_softmax(h, None, None) == _capi.UNKOWN_FORMAT               # (no nnz yet: no pointer is judged)
    assert lib.csr5hip_row_softmax_grad(h, None, None, None) == _capi.UNKOWN_FORMAT
    assert _info_bytes(lib, h) == before
    assert lib.csr5hip_input_csr(h, 100, None, None, None) == 0
    before = _info_bytes(lib, h)
    assert lib.csr5hip_row_softmax(h, None, fake) == _capi.INVALID_ARGUMENT            # null pointers, nnz > 0
    assert lib.csr5hip_row_softmax(h, fake, None) == _capi.INVALID_ARGUMENT
    assert lib.csr5hip_row_softmax_grad(h, None, fake, fake) == _capi.INVALID_ARGUMENT
    assert lib.csr5hip_row_softmax_grad(h, fake, None, fake) == _capi.INVALID_ARGUMENT
    assert lib.csr5hip_row_softmax_grad(h, fake, fake, None) == _capi.INVALID_ARGUMENT
    assert lib.csr5hip_row_softmax(None, None, None) == _capi.INVALID_ARGUMENT
    assert _info_bytes(lib, h) == before
    assert lib.csr5hip_input_csr(h, 0, None, None, None) == 0
    before = _info_bytes(lib, h)
    assert lib.csr5hip_row_softmax(h, None, None) == _capi.SUCCESS                     # nnz = 0: legal in CSR format, no device
    assert lib.csr5hip_row_softmax_grad(h, None, None, None) == _capi.SUCCESS
    assert _info_bytes(lib, h) == before
    assert lib.csr5hip_free(h) == 0


def test_python_methods_reject_bad_tensors_before_the_library():
    torch = pytest.importorskip("torch")
    A = H.anonymouslibHandle(6, 4)
    calls = []
    A.rowSoftmax_ptr = lambda *a: calls.append(a) or 0  # nothing may reach the library
    A.rowSoftmaxGrad_ptr = lambda *a: calls.append(a) or 0
    f64 = torch.float64
    s, g, out = torch.zeros(7, dtype=f64), torch.zeros(7, dtype=f64), torch.zeros(7, dtype=f64)
    with pytest.raises(ValueError, match="inputCSR"):
        A.rowSoftmax(s, out)
    with pytest.raises(ValueError, match="inputCSR"):
        A.rowSoftmaxGrad(s, g, out)
    assert A.inputCSR(7, None, None, None) == 0
    with pytest.raises(ValueError, match="GPU"):
        A.rowSoftmax(s, out)                                                  # host tensors
    with pytest.raises(ValueError, match="GPU"):
        A.rowSoftmaxGrad(s, g, out)
    for bad, word in ((s.float(), "dtype"), (torch.zeros(8, dtype=f64), "shape"), (torch.zeros(7, 1, dtype=f64), "shape"),
                      (torch.zeros(14, dtype=f64)[::2], "contiguous"), (np.zeros(7), "tensor")):
        with pytest.raises(ValueError, match=f"scores.*{word}"):
            A.rowSoftmax(bad, out)
        with pytest.raises(ValueError, match=f"out.*{word}"):
            A.rowSoftmax(s, bad)
        with pytest.raises(ValueError, match=f"p .*{word}"):
            A.rowSoftmaxGrad(bad, g, out)
        with pytest.raises(ValueError, match=f"g .*{word}"):
            A.rowSoftmaxGrad(s, bad, out)
        with pytest.raises(ValueError, match=f"out.*{word}"):
            A.rowSoftmaxGrad(s, g, bad)
    big = torch.zeros(14, dtype=f64)
    with pytest.raises(ValueError, match="scores.*aliased"):
        A.rowSoftmax(big[:7], big[7:])
    with pytest.raises(ValueError, match="scores.*aliased"):
        A.rowSoftmax(s, s)
    with pytest.raises(ValueError, match="with p .*aliased"):
        A.rowSoftmaxGrad(big[:7], g, big[7:])
    with pytest.raises(ValueError, match="with g .*aliased"):
        A.rowSoftmaxGrad(s, big[:7], big[7:])
    with pytest.raises(ValueError, match="GPU"):
        A.rowSoftmaxGrad(s, s, out)                                           # p and g may be one tensor: only the device is wrong
    assert calls == []
    A.close()


def test_autograd_exports_the_new_names_without_a_gpu():
    from benchmark_spmv_using_csr5_amd import autograd
    assert {"spmm", "sddmm", "row_softmax", "attention"} <= set(autograd.__all__)
    assert callable(autograd.sddmm) and callable(autograd.row_softmax) and callable(autograd.attention)
