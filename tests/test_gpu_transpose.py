"""y = A^T x on a converted handle (csr5hip_build_transpose / csr5hip_spmv_t / csr5hip_spmm_t).

Parents: every matrix of test_gpu_exact_reference._matrices() and ``transpose_csr`` of each of them, so that the companion is in
turn a hub-column matrix, a hub-row matrix, a matrix with rows over 64 tiles, one with p = 1, one with 78 % empty rows.  The
companion's structure is pinned by bit-identity with a handle built by hand from ``matrices.transpose_csr`` on every path, its
values by the exact reference of tests/exact_reference.py on data where one misplaced value changes a row by many orders of
magnitude.  fp64 and fp32.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from benchmark_spmv_using_csr5_amd import _capi  # noqa: E402
from benchmark_spmv_using_csr5_amd import handle as H  # noqa: E402
from benchmark_spmv_using_csr5_amd import matrices as M  # noqa: E402
from tests import exact_reference as R  # noqa: E402
from tests import zoo  # noqa: E402
from tests.test_gpu_exact_reference import (AUTO, DEV, PATHS, Y0, Path, _bits, _close, _dt, _handle, _matrices, _spmv,  # noqa: E402
                                            _tdt)

BY_NAME = {p.name: p for p in PATHS}
EXACT_PATHS = ("two-pass-s7", "fused-default", "xwin-narrow", "deferred-s7", "slabs8", "slabs8-hot", "zero-empty")
UPDATE_PATHS = ("fused-default", "slabs8-hot", "two-pass-s16")
T_FIELDS = (("t_sigma", "sigma"), ("t_p", "p"), ("t_tail_partition_start", "tail_partition_start"),
            ("t_column_slabs", "column_slabs"), ("t_slab_hot", "slab_hot"), ("t_x_window_active", "x_window_active"))
NEW_FIELDS = ("transpose_built", "t_transpose_build_ms") + tuple(t for t, _ in T_FIELDS)


@functools.lru_cache(maxsize=1)
def _parents():
    """(A, A^T, source map) for every parent: the matrices and their transposes"""
    out = []
    for mat in _matrices():
        out.append(mat)
        out.append(M.transpose_csr(mat))
    return tuple((mat,) + M.transpose_csr(mat, return_map=True) for mat in out)


@functools.lru_cache(maxsize=None)
def _tcase(pi, dataset, dtype, k=1, finite_matrix=False):
    """values drawn ON THE TRANSPOSED STRUCTURE (that is where the generators' invariants must hold) and carried back to A's
    order through the map: (A, A^T, val_A, val_T, X, [reference of A^T X[:, c]])"""
    mat, matT, src = _parents()[pi]
    valT, X = R.make(dataset, matT, dtype, seed=31 + pi, k=k, finite_matrix=finite_matrix)
    val = np.empty_like(valT)
    val[src] = valT
    return mat, matT, val, valT, X, [R.reference(dataset, matT, valT, X[:, c]) for c in range(k)]


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _fresh_path(path):
    """the same sigma request, mode and options for a handle built by hand from the transposed CSR: which variant the transposed
    shape selects is the library's business, and the x snapshot is not forwarded to a companion"""
    return Path(path.name, path.sigma, path.mode, tuple(o for o in path.opts if o[0] != "setXSnapshot"), {}, path.zero_empty)


def _build(A):
    assert A.buildTranspose() == 0, _capi.last_error()
    info = A.info()
    assert info.transpose_built == 1
    return info


def _spmvT(A, mat, x, dtype):
    xd = _dev(x, dtype)
    yd = torch.full((mat.n,), Y0, dtype=_tdt(dtype), device=DEV)
    assert A.spmvT(xd, yd) == 0, _capi.last_error()
    torch.cuda.synchronize()
    return yd.cpu().numpy()


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_dt)
@pytest.mark.parametrize("path", PATHS, ids=lambda p: p.name)
def test_spmvT_bit_identical_to_a_handle_built_by_hand(path, dtype):
    """every path, every parent: y (preset to Y0, so untouched empty rows count) and the companion's geometry / variant"""
    for pi in range(len(_parents())):
        mat, matT, val, valT, X, _ = _tcase(pi, "wide_range", dtype)
        A, _ = _handle(mat, val, path, dtype)
        info = _build(A)
        y = _spmvT(A, mat, X[:, 0], dtype)
        B, binfo = _handle(matT, valT, _fresh_path(path), dtype)
        yb = _spmv(B, matT, X[:, 0], dtype)
        assert _same(y, yb), (path.name, mat.name, _dt(dtype))
        got = {t: getattr(info, t) for t, _ in T_FIELDS}
        want = {t: getattr(binfo, f) for t, f in T_FIELDS}
        assert got == want, (path.name, mat.name, _dt(dtype))
        _close(B)
        _close(A)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_dt)
@pytest.mark.parametrize("name", EXACT_PATHS)
def test_spmvT_exact(name, dtype):
    path = BY_NAME[name]
    for pi in range(len(_parents())):
        for dataset in R.DATASETS:
            mat, matT, val, valT, X, refs = _tcase(pi, dataset, dtype)
            A, _ = _handle(mat, val, path, dtype)
            info = _build(A)
            y = _spmvT(A, mat, X[:, 0], dtype)
            R.check(y, refs[0], R.empty_zero_rows(mat.n, info.t_tail_partition_start, path.zero_empty), Y0,
                    f"spmvT {name} {mat.name} {dataset} {_dt(dtype)} t_sigma {info.t_sigma}")
            _close(A)


def _spmmT_run(A, mat, X, k, dtype, ldx, ldy):
    tdt = _tdt(dtype)
    Xb = torch.full((mat.m, ldx), float("nan"), dtype=tdt, device=DEV)
    Xb[:, :k] = _dev(X[:, :k], dtype)
    Yb = torch.full((mat.n, ldy), Y0, dtype=tdt, device=DEV)
    assert A.spmmT_ptr(Xb, ldx, k, Yb, ldy) == 0, _capi.last_error()
    torch.cuda.synchronize()
    return Yb.cpu().numpy()


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_dt)
def test_spmmT_matches_two_pass_spmv_of_the_transposed_handle(dtype):
    ks = (1, 3, 8, 13)
    two_pass = Path("two-pass", AUTO, H.SPMV_TWO_PASS)
    poison = _bits(np.full(1, Y0, dtype=dtype))[0]
    for pi in range(len(_parents())):
        mat, matT, val, valT, X, _ = _tcase(pi, "wide_range", dtype, k=max(ks))
        A, _ = _handle(mat, val, BY_NAME["fused-default"], dtype)
        _build(A)
        B, _ = _handle(matT, valT, two_pass, dtype)
        cols = [_spmv(B, matT, X[:, c], dtype) for c in range(max(ks))]
        for k in ks:
            for ldx, ldy in ((k, k), (k + 1, k + 2)):
                Y = _spmmT_run(A, mat, X, k, dtype, ldx, ldy)
                for c in range(k):
                    assert _same(Y[:, c], cols[c]), (mat.name, k, ldx, c)
                assert (_bits(Y[:, k:]) == poison).all(), (mat.name, k, ldy)
        # the tensor front end: leading dimensions from the strides
        Xd = _dev(X[:, :3], dtype)
        Yd = torch.full((mat.n, 3), Y0, dtype=_tdt(dtype), device=DEV)
        assert A.spmmT(Xd, Yd) == 0, _capi.last_error()
        torch.cuda.synchronize()
        for c in range(3):
            assert _same(Yd.cpu().numpy()[:, c], cols[c]), (mat.name, c)
        _close(B)
        _close(A)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_dt)
@pytest.mark.parametrize("name", ("fused-default", "slabs8-hot"))
def test_parent_is_untouched(name, dtype):
    path = BY_NAME[name]
    for pi in range(len(_parents())):
        mat, matT, val, valT, X, _ = _tcase(pi, "wide_range", dtype)
        _, XA = R.make("wide_range", mat, dtype, seed=5, k=3)
        A, before = _handle(mat, val, path, dtype)

        def products():
            y = _spmv(A, mat, XA[:, 0], dtype)
            Yd = torch.full((mat.m, 3), Y0, dtype=_tdt(dtype), device=DEV)
            assert A.spmm(_dev(XA, dtype), Yd) == 0
            torch.cuda.synchronize()
            return y, Yd.cpu().numpy()

        y0, Y0s = products()
        before = A.info()
        assert before.transpose_built == 0
        after = _build(A)
        y1, Y1s = products()
        assert _same(y0, y1) and _same(Y0s, Y1s), (name, mat.name)
        for f, _ in _capi.Csr5Info._fields_:
            if f not in NEW_FIELDS and f != "device_bytes":
                assert getattr(before, f) == getattr(after, f), (f, name, mat.name)
        if mat.nnz:
            # the CSR of A^T, the source map and the staging buffer at the very least
            assert after.device_bytes - before.device_bytes >= mat.nnz * (8 + 2 * np.dtype(dtype).itemsize) + 4 * (mat.n + 1)
            assert after.t_transpose_build_ms > 0
        else:
            assert after.device_bytes == before.device_bytes
        _spmvT(A, mat, X[:, 0], dtype)
        assert A.destroy() == 0
        torch.cuda.synchronize()
        rp, ci, va = A._arrays
        assert np.array_equal(rp.cpu().numpy(), mat.row_ptr.astype(np.int32))
        assert np.array_equal(ci.cpu().numpy(), mat.col.astype(np.int32)), (name, mat.name)
        assert _same(va.cpu().numpy(), val.astype(dtype)), (name, mat.name)
        gone = A.info()
        assert gone.transpose_built == 0 and gone.device_bytes == before.device_bytes, (name, mat.name)
        A.close()


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_dt)
@pytest.mark.parametrize("name", UPDATE_PATHS)
def test_update_values_keeps_both_sides_in_step(name, dtype):
    """V0 = wide_range, then V1 = row_scaled and nonfinite through updateValues: spmv equals a fresh handle of (A, V1), spmvT a
    fresh handle of (A^T, V1 through the map), bit for bit.  Then updateValues + spmvT + spmv captured in ONE graph on the handle's
    stream (after a warm-up round outside the capture) and replayed twice."""
    path = BY_NAME[name]
    side = torch.cuda.Stream()
    for pi in range(len(_parents())):
        mat, matT, v0, _, X0, _ = _tcase(pi, "wide_range", dtype)
        _, XA = R.make("wide_range", mat, dtype, seed=7)
        A, _ = _handle(mat, v0, path, dtype)
        _build(A)
        _spmv(A, mat, XA[:, 0], dtype)
        _spmvT(A, mat, X0[:, 0], dtype)
        fresh = {}
        for dataset in ("row_scaled", "nonfinite"):
            _, _, v1, v1T, X1, refs = _tcase(pi, dataset, dtype)
            _, X1A = R.make(dataset, mat, dtype, seed=9)
            buf = _dev(v1, dtype)
            keep = buf.clone()
            assert A.updateValues(buf) == 0, _capi.last_error()
            y = _spmv(A, mat, X1A[:, 0], dtype)
            yT = _spmvT(A, mat, X1[:, 0], dtype)
            assert torch.equal(buf.view(torch.uint8), keep.view(torch.uint8))  # the caller's tensor is only read
            B, _ = _handle(mat, v1, path, dtype)
            BT, binfo = _handle(matT, v1T, _fresh_path(path), dtype)
            fresh[dataset] = (_spmv(B, mat, X1A[:, 0], dtype), _spmv(BT, matT, X1[:, 0], dtype), v1, X1A[:, 0], X1[:, 0])
            assert _same(y, fresh[dataset][0]), (name, mat.name, dataset)
            assert _same(yT, fresh[dataset][1]), (name, mat.name, dataset)
            R.check(yT, refs[0], R.empty_zero_rows(mat.n, binfo.tail_partition_start), Y0, f"update {name} {mat.name} {dataset}")
            _close(B)
            _close(BT)
        if mat.nnz == 0:
            _close(A)
            continue
        # one captured graph: update + A^T x + A x
        torch.cuda.synchronize()
        buf = _dev(v0, dtype)
        xd, xTd = _dev(XA[:, 0], dtype), _dev(X0[:, 0], dtype)
        yd = torch.full((mat.m,), Y0, dtype=_tdt(dtype), device=DEV)
        yTd = torch.full((mat.n,), Y0, dtype=_tdt(dtype), device=DEV)
        assert A.setStream(side) == 0 and A.setX(xd) == 0
        assert A.updateValues(buf) == 0 and A.spmvT(xTd, yTd) == 0 and A.spmv(1.0, yd) == 0  # warm-up round
        side.synchronize()
        held = A.info().device_bytes
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            assert A.updateValues(buf) == 0, _capi.last_error()
            assert A.spmvT(xTd, yTd) == 0, _capi.last_error()
            assert A.spmv(1.0, yd) == 0, _capi.last_error()
        assert A.info().device_bytes == held
        for dataset in ("row_scaled", "nonfinite"):
            want_y, want_yT, v1, xa, xt = fresh[dataset]
            buf.copy_(_dev(v1, dtype))
            xd.copy_(_dev(xa, dtype))
            xTd.copy_(_dev(xt, dtype))
            for _ in range(2):
                yd.fill_(Y0)
                yTd.fill_(Y0)
                torch.cuda.synchronize()
                graph.replay()
                torch.cuda.synchronize()
                assert _same(yd.cpu().numpy(), want_y), (name, mat.name, dataset)
                assert _same(yTd.cpu().numpy(), want_yT), (name, mat.name, dataset)
        del graph
        assert A.setStream(None) == 0
        _close(A)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_dt)
def test_life_cycle_and_errors(dtype):
    picks = [i for i, (m, _, _) in enumerate(_parents()) if m.name in ("hub", "nonsquare", "half-empty^T", "tiny-p1")]
    assert len(picks) == 4
    for pi in picks:
        mat, matT, val, valT, X, _ = _tcase(pi, "nonfinite", dtype)
        A, _ = _handle(mat, val, BY_NAME["fused-default"], dtype)
        xd = _dev(X[:, 0], dtype)
        yd = torch.full((mat.n,), Y0, dtype=_tdt(dtype), device=DEV)
        assert A.spmvT(xd, yd) == _capi.INVALID_ARGUMENT                      # never built lazily
        assert "csr5hip_build_transpose" in _capi.last_error()
        assert A.spmmT_ptr(xd, 1, 1, yd, 1) == _capi.INVALID_ARGUMENT
        torch.cuda.synchronize()
        assert (_bits(yd.cpu().numpy()) == _bits(np.full(1, Y0, dtype=dtype))[0]).all()
        _build(A)
        assert A.spmvT_ptr(None, yd) == _capi.INVALID_ARGUMENT and A.spmvT_ptr(xd, None) == _capi.INVALID_ARGUMENT
        first = _spmvT(A, mat, X[:, 0], dtype)
        held = A.info().device_bytes
        assert A.buildTranspose() == 0 and A.info().device_bytes == held       # a no-op
        for _ in range(10):                                                    # run-to-run bit reproducibility
            assert _same(_spmvT(A, mat, X[:, 0], dtype), first), mat.name
        # an option set on the parent after the build reaches the companion
        has = np.diff(matT.row_ptr) > 0
        assert A.setZeroEmptyRows(1) == 0
        y = _spmvT(A, mat, X[:, 0], dtype)
        assert (y[~has] == 0).all() and _same(y[has], first[has]), mat.name
        assert A.setZeroEmptyRows(0) == 0
        assert _same(_spmvT(A, mat, X[:, 0], dtype), first), mat.name
        assert A.asCSR() == 0
        assert A.info().transpose_built == 0
        assert A.spmvT(xd, yd) == _capi.UNSUPPORTED_CSR_SPMV
        assert A.spmmT_ptr(xd, 1, 1, yd, 1) == _capi.UNSUPPORTED_CSR_SPMV
        assert A.buildTranspose() == _capi.UNSUPPORTED_CSR_SPMV
        assert A.asCSR5() == 0
        assert A.spmvT(xd, yd) == _capi.INVALID_ARGUMENT                      # the companion went with the conversion
        _build(A)
        assert _same(_spmvT(A, mat, X[:, 0], dtype), first), mat.name
        _close(A)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_dt)
@pytest.mark.parametrize("zero_empty", (False, True))
def test_empty_matrix(zero_empty, dtype):
    mat = zoo.empty_matrix()
    path = BY_NAME["zero-empty" if zero_empty else "fused-default"]
    A, _ = _handle(mat, np.zeros(0, dtype=dtype), path, dtype)
    before = A.info().device_bytes
    info = _build(A)
    assert info.device_bytes == before and info.t_p == 0 and info.t_tail_partition_start == mat.n
    y = _spmvT(A, mat, np.ones(mat.m, dtype=dtype), dtype)
    assert (y == (0.0 if zero_empty else Y0)).all()
    Xd = torch.ones((mat.m, 2), dtype=_tdt(dtype), device=DEV)
    Yd = torch.full((mat.n, 2), Y0, dtype=_tdt(dtype), device=DEV)
    assert A.spmmT(Xd, Yd) == 0
    torch.cuda.synchronize()
    assert (Yd.cpu().numpy() == (0.0 if zero_empty else Y0)).all()
    assert A.updateValues_ptr(None) == 0
    _close(A)
