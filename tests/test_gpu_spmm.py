"""SpMM on the GPU: Y = A * X for k dense vectors (csr5hip_spmm / anonymouslibHandle.spmm).

Contract pinned here (include/csr5hip.h): column c of Y is bit-identical to a two-pass spmv() (no column slabs) of X[:, c]
on a handle made from the same CSR with the same sigma -- whatever options the SpMM handle carries; rows and padding
columns that spmv() would not write keep their contents."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from benchmark_spmv_using_csr5_amd import matrices as M  # noqa: E402
from benchmark_spmv_using_csr5_amd import handle as H  # noqa: E402
from benchmark_spmv_using_csr5_amd import _capi  # noqa: E402
from tests import zoo  # noqa: E402

DEV = "cuda:0"
SIGMAS = [1, 3, 4, 7, 12, 16, 24, 32]
KS = [1, 2, 3, 5, 8, 13]
POISON = 777.0


def _tdt(dtype):
    return torch.float64 if dtype == np.float64 else torch.float32


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def _handle(mat, val, sigma, dtype, mode=H.SPMV_TWO_PASS, slabs=0, **opts):
    """a converted handle on device copies of the CSR arrays (kept alive on the handle object)"""
    rp = torch.from_numpy(mat.row_ptr.astype(np.int32)).to(DEV)
    ci = torch.from_numpy(mat.col.astype(np.int32)).to(DEV)
    va = torch.from_numpy(val.astype(dtype)).to(DEV)
    A = H.anonymouslibHandle(mat.m, mat.n, dtype=np.dtype(dtype).name)
    A._arrays = (rp, ci, va)
    assert A.inputCSR(mat.nnz, rp, ci, va) == 0
    assert A.setSigma(sigma) == 0
    assert A.setSpmvMode(mode) == 0
    for name, value in opts.items():
        assert getattr(A, name)(value) == 0, name
    assert A.asCSR5() == 0
    if slabs is not None:
        assert A.setColumnSlabs(slabs) == 0
    return A


def _columns(n, k, dtype, seed, mode):
    cols = [M.fill_values(1, n, dtype, seed=seed + c, mode=mode)[1] for c in range(k)]
    return np.stack(cols, axis=1).astype(dtype) if k else np.zeros((n, 0), dtype=dtype)


def _spmm(A, X, m, k, dtype, ldy=None, y0=POISON):
    """Y (m x ldy, poisoned) = A * X through the Python binding; returns the whole Y buffer on the host"""
    ldy = k if ldy is None else ldy
    Xd = torch.from_numpy(np.ascontiguousarray(X)).to(DEV)
    Yb = torch.full((m, ldy), y0, dtype=_tdt(dtype), device=DEV)
    assert A.spmm(Xd, Yb[:, :k]) == 0
    torch.cuda.synchronize()
    return Yb.cpu().numpy()


def _two_pass_columns(mat, val, sigma, dtype, X, y0=POISON):
    """the reference of the contract: two-pass spmv() of every column, column slabs off"""
    R = _handle(mat, val, sigma, dtype)
    out = np.empty((mat.m, X.shape[1]), dtype=dtype)
    for c in range(X.shape[1]):
        xd = torch.from_numpy(np.ascontiguousarray(X[:, c])).to(DEV)
        yd = torch.full((mat.m,), y0, dtype=_tdt(dtype), device=DEV)
        assert R.setX(xd) == 0 and R.spmv(1.0, yd) == 0
        torch.cuda.synchronize()
        out[:, c] = yd.cpu().numpy()
    R.destroy()
    R.close()
    return out


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_spmm_integer_data_exact_against_oracle(oracle, dtype):
    """integer data: every column equals the oracle's CSR5 SpMV with a poisoned y0; padding columns keep their poison"""
    kmax = max(KS)
    for mat in zoo.small_zoo():
        val, _ = M.fill_values(mat.nnz, mat.n, dtype, seed=1, mode="int")
        X13 = _columns(mat.n, kmax, dtype, 100, "int")
        for sigma in SIGMAS:
            fmt = oracle.convert(64, sigma, mat.m, mat.row_ptr, mat.col, val.astype(dtype))
            exp = np.stack([oracle.spmv(fmt, mat.row_ptr, X13[:, c], y0=np.full(mat.m, POISON, dtype=dtype))
                            for c in range(kmax)], axis=1)
            A = _handle(mat, val, sigma, dtype, slabs=None)
            for k in KS:
                Y = _spmm(A, X13[:, :k], mat.m, k, dtype, ldy=k + 3)
                assert np.array_equal(Y[:, :k], exp[:, :k]), (mat.name, sigma, k)
                assert (Y[:, k:] == POISON).all(), (mat.name, sigma, k)
            A.destroy()
            A.close()


def _long_row_matrix():
    rng = np.random.default_rng(77)
    lens = list(rng.integers(0, 9, size=300)) + [21000] + list(rng.integers(0, 9, size=300)) + [17000, 3]
    return M.csr_from_row_lengths(np.asarray(lens), 30000, rng, name="row-over-64-tiles")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_spmm_bit_identical_to_two_pass_spmv_on_real_data(dtype):
    cases = [(mat, s, 5) for mat in zoo.small_zoo() for s in (4, 7, 16)]
    cases += [(_long_row_matrix(), 4, 3), (_long_row_matrix(), 4, 8)]
    nd = M.nd24k_like(scale=0.25, dtype=dtype)
    cases += [(nd, 16, 8), (nd, 16, 16)]
    for mat, sigma, k in cases:
        val, _ = M.fill_values(mat.nnz, mat.n, dtype, seed=3, mode="real")
        X = _columns(mat.n, k, dtype, 200, "real")
        ref = _two_pass_columns(mat, val, sigma, dtype, X)
        A = _handle(mat, val, sigma, dtype, slabs=None)
        Y = _spmm(A, X, mat.m, k, dtype)
        assert np.array_equal(_bits(Y), _bits(ref)), (mat.name, sigma, k)
        # and close to the float64 product
        dense = np.zeros(mat.m, dtype=np.float64)
        rows = np.repeat(np.arange(mat.m), np.diff(mat.row_ptr))
        has = np.diff(mat.row_ptr) > 0
        for c in range(k):
            prod = val.astype(np.float64) * X[mat.col, c].astype(np.float64)
            dense[:] = 0
            np.add.at(dense, rows, prod)
            tol = 1e-9 if dtype == np.float64 else 2e-3
            scale = np.abs(val.astype(np.float64)).max() * np.abs(X[:, c]).max() * (np.diff(mat.row_ptr).max() + 1)
            assert np.abs(Y[has, c] - dense[has]).max() <= tol * scale, (mat.name, c)
        A.destroy()
        A.close()


def test_spmm_ignores_the_handles_spmv_options():
    """forced column slabs + forced hot table, and fused mode + forced deferred carries: the same Y as the two-pass
    reference; spmv() on the same handle gives the same y before and after an spmm() call"""
    dtype = np.float64
    for mat in (M.rmat(14, 16, seed=2), M.scircuit_like(scale=0.1), zoo.small_zoo()[6]):
        val, x = M.fill_values(mat.nnz, mat.n, dtype, seed=4, mode="real")
        X = _columns(mat.n, 4, dtype, 300, "real")
        ref = _two_pass_columns(mat, val, 16, dtype, X)
        variants = [dict(mode=H.SPMV_FUSED, slabs=8, setSlabHot=2),
                    dict(mode=H.SPMV_FUSED, slabs=0, setDeferCarries=2)]
        for opts in variants:
            opts = dict(opts)
            mode, slabs = opts.pop("mode"), opts.pop("slabs")
            hot = opts.pop("setSlabHot", None)
            A = _handle(mat, val, 16, dtype, mode=mode, slabs=None, **opts)
            if slabs:
                assert A.setColumnSlabs(slabs) == 0 and A.setSlabHot(hot) == 0
            xd = torch.from_numpy(x).to(DEV)
            assert A.setX(xd) == 0
            y1 = torch.full((mat.m,), POISON, dtype=torch.float64, device=DEV)
            assert A.spmv(1.0, y1) == 0
            Y = _spmm(A, X, mat.m, 4, dtype)
            y2 = torch.full((mat.m,), POISON, dtype=torch.float64, device=DEV)
            assert A.spmv(1.0, y2) == 0
            torch.cuda.synchronize()
            assert np.array_equal(_bits(Y), _bits(ref)), (mat.name, opts, slabs)
            assert np.array_equal(_bits(y1.cpu().numpy()), _bits(y2.cpu().numpy())), (mat.name, opts, slabs)
            if slabs:
                assert A.info().column_slabs > 0 and A.info().slab_hot == 1
            A.destroy()
            A.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_spmm_x_layouts(dtype):
    """ldx = k, ldx = k + 1 and X one element into its allocation (element loads instead of 16-byte ones)"""
    mat = M.webbase_like(scale=0.02)
    val, _ = M.fill_values(mat.nnz, mat.n, dtype, seed=6, mode="real")
    sigma = 8
    for k in (2, 4, 8):
        X = _columns(mat.n, k, dtype, 400, "real")
        ref = _two_pass_columns(mat, val, sigma, dtype, X)
        A = _handle(mat, val, sigma, dtype, slabs=None)
        tdt = _tdt(dtype)
        for layout in ("dense", "ld+1", "offset"):
            if layout == "dense":
                Xd, ldx, base = torch.from_numpy(X).to(DEV), k, None
                ptr = Xd.data_ptr()
            elif layout == "ld+1":
                buf = torch.zeros((mat.n, k + 1), dtype=tdt, device=DEV)
                buf[:, :k] = torch.from_numpy(X).to(DEV)
                Xd, ldx, ptr = buf, k + 1, buf.data_ptr()
            else:
                buf = torch.zeros(mat.n * k + 1, dtype=tdt, device=DEV)
                buf[1:] = torch.from_numpy(X.reshape(-1)).to(DEV)
                Xd, ldx, ptr = buf, k, buf.data_ptr() + buf.element_size()
                assert ptr % 16 != 0
            Yd = torch.full((mat.m, k), POISON, dtype=tdt, device=DEV)
            assert A.spmm_ptr(ptr, ldx, k, Yd, k) == 0
            torch.cuda.synchronize()
            assert np.array_equal(_bits(Yd.cpu().numpy()), _bits(ref)), (k, layout)
            if layout == "ld+1":  # the tensor binding takes the leading dimension from stride(0)
                Y2 = torch.full((mat.m, k), POISON, dtype=tdt, device=DEV)
                assert A.spmm(buf[:, :k], Y2) == 0
                torch.cuda.synchronize()
                assert np.array_equal(_bits(Y2.cpu().numpy()), _bits(ref)), (k, "tensor ld+1")
        A.destroy()
        A.close()


def test_spmm_is_repeatable():
    mat = M.scircuit_like(scale=0.1)
    val, _ = M.fill_values(mat.nnz, mat.n, np.float64, seed=7, mode="real")
    X = _columns(mat.n, 8, np.float64, 500, "real")
    A = _handle(mat, val, 6, np.float64, mode=H.SPMV_FUSED, slabs=None)
    first = _spmm(A, X, mat.m, 8, np.float64)
    for _ in range(9):
        assert np.array_equal(_bits(_spmm(A, X, mat.m, 8, np.float64)), _bits(first))
    A.destroy()
    A.close()


def test_spmm_edge_cases(tmp_path):
    lib = _capi.load()
    mat = zoo.small_zoo()[5]  # half-empty
    val, _ = M.fill_values(mat.nnz, mat.n, np.float64, seed=8, mode="int")
    X = _columns(mat.n, 3, np.float64, 600, "int")
    Xd = torch.from_numpy(X).to(DEV)
    # argument errors
    A = H.anonymouslibHandle(mat.m, mat.n)
    Yd = torch.full((mat.m, 3), POISON, dtype=torch.float64, device=DEV)
    assert A.spmm_ptr(Xd, 3, 3, Yd, 3) == _capi.UNKOWN_FORMAT
    rp = torch.from_numpy(mat.row_ptr).to(DEV)
    ci = torch.from_numpy(mat.col).to(DEV)
    va = torch.from_numpy(val).to(DEV)
    assert A.inputCSR(mat.nnz, rp, ci, va) == 0
    assert A.spmm(Xd, Yd) == _capi.UNSUPPORTED_CSR_SPMV
    assert A.setSigma(7) == 0 and A.asCSR5() == 0
    assert A.spmm_ptr(Xd, 3, -1, Yd, 3) == _capi.INVALID_ARGUMENT
    assert A.spmm_ptr(Xd, 2, 3, Yd, 3) == _capi.INVALID_ARGUMENT
    assert A.spmm_ptr(Xd, 3, 3, Yd, 2) == _capi.INVALID_ARGUMENT
    assert A.spmm_ptr(0, 3, 3, Yd, 3) == _capi.INVALID_ARGUMENT
    assert A.spmm_ptr(Xd, 3, 3, 0, 3) == _capi.INVALID_ARGUMENT
    # k = 0 writes nothing
    assert A.spmm_ptr(Xd, 3, 0, Yd, 3) == 0
    assert A.spmm_ptr(0, 0, 0, 0, 0) == 0
    torch.cuda.synchronize()
    assert (Yd.cpu().numpy() == POISON).all()
    # ZERO_EMPTY_ROWS: every row defined; padding column untouched
    ref = _two_pass_columns(mat, val, 7, np.float64, X, y0=0.0)
    assert A.setZeroEmptyRows(1) == 0
    Y = _spmm(A, X, mat.m, 3, np.float64, ldy=4)
    assert np.array_equal(_bits(Y[:, :3]), _bits(ref)) and (Y[:, 3] == POISON).all()
    assert A.setZeroEmptyRows(0) == 0
    Y = _spmm(A, X, mat.m, 3, np.float64)
    has = np.diff(mat.row_ptr) > 0
    assert (Y[~has & (np.arange(mat.m) < A.info().tail_partition_start)] == POISON).all()
    # a handle loaded from a checkpoint
    path = os.path.join(str(tmp_path), "m.csr5")
    assert A.save(path) == 0
    exp = _spmm(A, X, mat.m, 3, np.float64)
    B = H.anonymouslibHandle.load(path)
    assert np.array_equal(_bits(_spmm(B, X, mat.m, 3, np.float64)), _bits(exp))
    B.close()
    A.destroy()
    A.close()
    # the empty matrix
    e = zoo.empty_matrix()
    E = _handle(e, np.zeros(0), 4, np.float64, slabs=None)
    Y = _spmm(E, np.ones((e.n, 2)), e.m, 2, np.float64)
    assert (Y == POISON).all()
    assert E.setZeroEmptyRows(1) == 0
    assert (_spmm(E, np.ones((e.n, 2)), e.m, 2, np.float64) == 0).all()
    E.destroy()
    E.close()
    del lib


def test_spmm_is_capturable_in_a_callers_graph():
    """after one warm-up call spmm only enqueues kernels: a torch CUDA graph on a side stream replays it"""
    mat = M.scircuit_like(scale=0.1)
    val, _ = M.fill_values(mat.nnz, mat.n, np.float64, seed=9, mode="real")
    X = _columns(mat.n, 5, np.float64, 700, "real")
    side = torch.cuda.Stream(device=DEV)
    rp = torch.from_numpy(mat.row_ptr).to(DEV)
    ci = torch.from_numpy(mat.col).to(DEV)
    va = torch.from_numpy(val).to(DEV)
    A = H.anonymouslibHandle(mat.m, mat.n, stream=side.cuda_stream)
    assert A.inputCSR(mat.nnz, rp, ci, va) == 0 and A.setSigma(8) == 0 and A.asCSR5() == 0
    Xd = torch.from_numpy(X).to(DEV)
    Yd = torch.zeros((mat.m, 5), dtype=torch.float64, device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert A.spmm(Xd, Yd) == 0  # warm-up: allocates the workspace
    side.synchronize()
    direct = Yd.cpu().numpy().copy()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        assert A.spmm(Xd, Yd) == 0
    for _ in range(2):
        Yd.fill_(-5.0)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        has = np.diff(mat.row_ptr) > 0
        assert np.array_equal(_bits(Yd.cpu().numpy()[has]), _bits(direct[has]))
    del graph
    A.destroy()
    A.close()
