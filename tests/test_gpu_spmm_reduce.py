"""csr5hip_spmm_reduce and csr5hip_spmm_reduce_backward on the GPU against tests/spmm_reduce_reference.py (include/csr5hip_reduce.h).

The forward has no tolerance: the order is total, so Y and arg are compared bit for bit on every path, class edge and width.  dval
is one fma chain and is compared bit for bit; dX is compared bit for bit on integer operands (every sum exact in any order) and, on
random operands, under the bound (w + 1) u sum|a_e dY| per (j, c) -- w winning terms: one rounding per product, w - 1 additions
and the +0 a chain starts from.  The reference alone sits inside that bound (its own products are exact in fp32 and rounded once in
fp64)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from benchmark_spmv_using_csr5_amd import _capi  # noqa: E402
from benchmark_spmv_using_csr5_amd import autograd as AG  # noqa: E402
from benchmark_spmv_using_csr5_amd import handle as H  # noqa: E402
from benchmark_spmv_using_csr5_amd import matrices as M  # noqa: E402
from tests import attention_edges as E  # noqa: E402
from tests import sddmm_reference as S  # noqa: E402
from tests import spmm_reduce_reference as R  # noqa: E402
from tests import zoo  # noqa: E402
from tests.test_gpu_exact_reference import PATHS, _handle  # noqa: E402

DEV = "cuda:0"
PATH = {p.name: p for p in PATHS}
PATH_NAMES = ("two-pass-s4", "two-pass-s7", "two-pass-s32", "fused-default", "xwin-narrow", "slabs8-hot")
KS = (1, 3, 16, 17, 64, 65)   # a width below 16, a power-of-two pad, one full block, a second column block of width 1
DTYPES = (np.float64, np.float32)
Y_POISON, ARG_POISON = 777.25, 0x7B7B7B7B


def _dt(dtype):
    return "fp64" if dtype == np.float64 else "fp32"


def _tdt(dtype):
    return torch.float64 if np.dtype(dtype) == np.float64 else torch.float32


@functools.lru_cache(maxsize=1)
def _matrices():
    return (E.class_edges(),) + tuple(zoo.small_zoo()) + (S.duplicates_matrix(),)


@functools.lru_cache(maxsize=None)
def _values(mi, dtype):
    return R.distinct_values(_matrices()[mi].nnz, dtype, seed=11 + mi)


@functools.lru_cache(maxsize=None)
def _x(mi, dtype, k):
    return np.random.default_rng([7, mi, k]).uniform(-1, 1, size=(_matrices()[mi].n, k)).astype(dtype)


@functools.lru_cache(maxsize=None)
def _forward_ref(mi, dtype, k, op, weighted):
    """computed once, shared by every path"""
    return R.forward(_matrices()[mi], _values(mi, dtype), _x(mi, dtype, k), op, weighted)


def _padded(t, pad, off, fill):
    """a device copy of the (rows, k) array t inside a 1-D buffer: `off` elements in front, rows of k + pad elements, one guard element
    behind; padding, front and guard hold `fill`.  Returns (the (rows, k) view with stride k + pad, the buffer)"""
    rows, k = t.shape
    ld = k + pad
    buf = torch.full((off + rows * ld + 1,), fill, dtype=torch.from_numpy(t[:0]).dtype, device=DEV)
    view = buf[off:off + rows * ld].view(rows, ld)[:, :k]
    view.copy_(torch.from_numpy(t).to(DEV))
    return view, buf


def _untouched(buf, view_rows, k, pad, off, fill):
    """front, padding and guard of a _padded buffer still hold `fill`"""
    ld = k + pad
    b = buf.cpu().numpy()
    body = b[off:off + view_rows * ld].reshape(view_rows, ld)
    f = np.array(fill, dtype=b.dtype)
    same = (lambda a: np.isnan(a).all()) if (b.dtype.kind == "f" and np.isnan(f)) else (lambda a: (a == f).all())
    return same(b[:off]) and same(body[:, k:]) and same(b[-1:])


def _run_forward(A, X, m, k, dtype, op, weighted, pad=0, off=0, want_arg=True):
    Xv, _ = _padded(X, pad, off, np.nan)
    Yv, Yb = _padded(np.full((m, k), Y_POISON, dtype=dtype), pad, off, Y_POISON)
    Av, Ab = _padded(np.full((m, k), ARG_POISON, dtype=np.int32), pad, off, ARG_POISON)
    assert A.spmmReduce(Xv, Yv, op, Av if want_arg else None, weighted) == 0, _capi.last_error()
    torch.cuda.synchronize()
    assert _untouched(Yb, m, k, pad, off, Y_POISON), "Y: written outside its k columns"
    assert _untouched(Ab, m, k, pad, off, ARG_POISON), "arg: written outside its k columns"
    return Yv.cpu().numpy(), Av.cpu().numpy()


def _close(A):
    A.destroy()
    A.close()


# ---- 1. forward, bit for bit -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("path", PATH_NAMES)
def test_forward_bit_for_bit(path, dtype):
    """every matrix, k, op and weighting on one conversion path: Y and arg equal the reference bit for bit; leading dimensions padded
    with NaN and pointers 1 and 3 elements into their buffers on alternating cases; poison everywhere before the call, every row
    overwritten (rows without entries +0 / -1), nothing outside the k columns, the guard element intact"""
    for mi, mat in enumerate(_matrices()):
        A, _ = _handle(mat, _values(mi, dtype), PATH[path], dtype)
        case = 0
        for k in KS:
            for op in ("max", "min"):
                for weighted in (True, False):
                    pad, off = ((0, 0), (3, 1), (1, 3))[case % 3]
                    case += 1
                    Y, arg = _run_forward(A, _x(mi, dtype, k), mat.m, k, dtype, op, weighted, pad, off)
                    Yr, argr = _forward_ref(mi, dtype, k, op, weighted)
                    where = (mat.name, path, k, op, weighted)
                    assert np.array_equal(arg, argr), where
                    assert R.same_bits(Y, Yr), where
        _close(A)


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_forward_without_arg(dtype):
    mat = _matrices()[0]
    A, _ = _handle(mat, _values(0, dtype), PATH["fused-default"], dtype)
    for k in (3, 65):
        Y, arg = _run_forward(A, _x(0, dtype, k), mat.m, k, dtype, "max", True, 2, 1, want_arg=False)
        assert R.same_bits(Y, _forward_ref(0, dtype, k, "max", True)[0])
        assert (arg == ARG_POISON).all()
    X = torch.zeros((mat.n, 0), dtype=_tdt(dtype), device=DEV)
    assert A.spmmReduce(X, torch.zeros((mat.m, 0), dtype=_tdt(dtype), device=DEV)) == 0  # k = 0: a successful no-op
    _close(A)


# ---- 2. ties and specials ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("path", ("two-pass-s7", "fused-default"))
def test_ties_and_specials(path, dtype):
    rng = np.random.default_rng(41)
    for mat in (_matrices()[0], _matrices()[-1]):  # class-edges, duplicates
        val = R.distinct_values(mat.nnz, dtype)
        zeros = rng.random(mat.nnz) < 0.3
        val0 = np.where(zeros, 0, val).astype(dtype)  # a_e = 0 against Inf: NaN
        A, _ = _handle(mat, val, PATH[path], dtype)
        A0, _ = _handle(mat, val0, PATH[path], dtype)
        k = 5
        Xi = rng.integers(-2, 3, size=(mat.n, k)).astype(dtype)
        Xneg = np.full((mat.n, k), -np.inf, dtype=dtype)
        Xnan = rng.uniform(-1, 1, size=(mat.n, k)).astype(dtype)
        jn = int(mat.col[mat.row_ptr[np.flatnonzero(np.diff(mat.row_ptr) > 16)[0]]])
        Xnan[jn, :] = np.nan
        Xz = np.where(rng.random((mat.n, k)) < 0.5, 0.0, -0.0).astype(dtype)
        Xinf = rng.uniform(-1, 1, size=(mat.n, k)).astype(dtype)
        Xinf[rng.random(mat.n) < 0.2] = np.inf
        for what, h, v, X, weighted in (("integer X", A, val, Xi, False), ("all -Inf", A, val, Xneg, False), ("NaN row", A, val, Xnan, False),
                                        ("NaN row, weighted", A, val, Xnan, True), ("+0 against -0", A, val, Xz, False),
                                        ("+0 against -0, weighted", A, val, Xz, True), ("0 * Inf", A0, val0, Xinf, True)):
            for op in ("max", "min"):
                Y, arg = _run_forward(h, X, mat.m, k, dtype, op, weighted, 1, 1)
                Yr, argr = R.forward(mat, v, X, op, weighted)
                assert np.array_equal(arg, argr), (mat.name, what, op)
                assert R.same_bits(Y, Yr), (mat.name, what, op)
                has = np.diff(mat.row_ptr) > 0
                if what == "integer X":  # most pairs tie, and arg is the smallest tied rank
                    t = R.terms(mat, v, X, False)
                    rows = R.rows_of(mat)
                    tied = (t == Y[rows]).astype(np.int64)
                    count = np.zeros((mat.m, k), dtype=np.int64)
                    np.add.at(count, rows, tied)
                    assert (count[has] > 1).mean() > (0.5 if mat.m > 200 else 0.25), (mat.name, "too few ties to mean anything")
                    firsts = np.full((mat.m, k), mat.nnz, dtype=np.int64)
                    np.minimum.at(firsts, rows, np.where(tied > 0, np.arange(mat.nnz)[:, None], mat.nnz))
                    assert np.array_equal(arg[has], firsts[has])
                if what == "all -Inf":
                    assert np.isneginf(Y[has]).all()
                    assert np.array_equal(arg[has], np.broadcast_to(mat.row_ptr[:-1][has, None], arg[has].shape))
                if what == "NaN row":  # the NaN reaches exactly the rows that hold column jn; arg is the first such entry
                    cols, rows = mat.col[:mat.nnz], R.rows_of(mat)
                    holds = np.zeros(mat.m, dtype=bool)
                    holds[rows[cols == jn]] = True
                    assert np.array_equal(np.isnan(Y).all(axis=1), holds) and not np.isnan(Y[~holds]).any()
                    first = np.full(mat.m, mat.nnz, dtype=np.int64)
                    np.minimum.at(first, rows[cols == jn], np.flatnonzero(cols == jn))
                    assert np.array_equal(arg[holds], np.broadcast_to(first[holds, None], arg[holds].shape))
                if what == "0 * Inf":
                    assert np.isnan(Yr).any() and np.isinf(Yr).any()
        _close(A)
        _close(A0)


# ---- 3. backward -------------------------------------------------------------------------------------------------------------------------
def _backward(A, X, dY, arg, n, nnz, k, dtype, weighted, want_dx=True, want_dval=True, pad=0, off=0):
    Xv, _ = _padded(X, pad, off, np.nan)
    Gv, _ = _padded(dY, pad, off, np.nan)
    Av, _ = _padded(arg, pad, off, -5)
    dXv, dXb = _padded(np.full((n, k), Y_POISON, dtype=dtype), pad, off, Y_POISON)
    dval = torch.full((nnz + 1,), Y_POISON, dtype=_tdt(dtype), device=DEV)
    rc = A.spmmReduceBackward(Xv, Gv, Av, dXv if want_dx else None, dval[:nnz] if want_dval else None, weighted)
    torch.cuda.synchronize()
    assert _untouched(dXb, n, k, pad, off, Y_POISON), "dX: written outside its k columns"
    assert float(dval[nnz]) == Y_POISON
    return rc, dXv.cpu().numpy(), dval[:nnz].cpu().numpy()


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("which", ("class-edges", "dealt"))
def test_backward(which, dtype):
    """class_edges() takes the row kernel (dval) through every class, dealt() the column kernel (dX): its column lengths are
    class_edges()' row lengths, hub columns in later workgroups included"""
    mat = E.class_edges() if which == "class-edges" else E.dealt()
    rng = np.random.default_rng([51, mat.nnz])
    val = R.distinct_values(mat.nnz, dtype)
    ival = (rng.integers(1, 9, size=mat.nnz) * rng.choice([-1, 1], size=mat.nnz)).astype(dtype)
    A, _ = _handle(mat, val, PATH["two-pass-s7"], dtype)
    Ai, _ = _handle(mat, ival, PATH["fused-default"], dtype)

    # dX without a companion: the error, and nothing is written
    X, dY = rng.uniform(-1, 1, size=(mat.n, 3)).astype(dtype), rng.uniform(-1, 1, size=(mat.m, 3)).astype(dtype)
    _, arg = R.forward(mat, val, X, "max", True)
    rc, dX, dval = _backward(A, X, dY, arg, mat.n, mat.nnz, 3, dtype, True)
    assert rc == _capi.INVALID_ARGUMENT and "csr5hip_build_transpose first" in _capi.last_error()
    assert (dX == Y_POISON).all() and (dval == Y_POISON).all()
    assert A.buildTranspose() == 0 and Ai.buildTranspose() == 0, _capi.last_error()

    for k in (3, 17, 65):
        X, dY = rng.uniform(-1, 1, size=(mat.n, k)).astype(dtype), rng.uniform(-1, 1, size=(mat.m, k)).astype(dtype)
        for weighted in (True, False):
            op = "max" if weighted else "min"
            Y, arg = _run_forward(A, X, mat.m, k, dtype, op, weighted)
            assert np.array_equal(arg, R.forward(mat, val, X, op, weighted)[1])
            rc, dX, dval = _backward(A, X, dY, arg, mat.n, mat.nnz, k, dtype, weighted, want_dval=weighted, pad=2, off=1)
            assert rc == 0, _capi.last_error()
            ref, w, mag = R.dx(mat, val, dY, arg, weighted)
            err = np.abs(dX.astype(np.float64) - ref)
            assert (err <= R.dx_bound(w, mag, dtype)).all(), (which, k, weighted, float(err.max()))
            assert not dX[w == 0].view(np.uint8).any(), "dX is not +0 where nothing wins"
            if weighted and (which == "class-edges" or k == 17):
                assert R.same_bits(dval, R.dval(mat, X, dY, arg)), (which, k, "dval")
            if weighted and k == 17:  # either output left out leaves the other unchanged, bit for bit
                rc, dX1, dval1 = _backward(A, X, dY, arg, mat.n, mat.nnz, k, dtype, True, want_dval=False)
                assert rc == 0 and R.same_bits(dX1, dX) and (dval1 == Y_POISON).all()
                rc, dX2, dval2 = _backward(A, X, dY, arg, mat.n, mat.nnz, k, dtype, True, want_dx=False)
                assert rc == 0 and R.same_bits(dval2, dval) and (dX2 == Y_POISON).all()
                bad = np.roll(arg, 1, axis=0)  # a corrupt arg: other rows' ranks match nothing, nothing is indexed by it
                rc, _, dval3 = _backward(A, X, dY, bad, mat.n, mat.nnz, k, dtype, True, want_dx=False)
                assert rc == 0 and R.same_bits(dval3, R.dval(mat, X, dY, bad))
        # integer operands of magnitude <= 8: every sum is exact in any order
        Xi, dYi = rng.integers(-8, 9, size=(mat.n, k)).astype(dtype), rng.integers(-8, 9, size=(mat.m, k)).astype(dtype)
        Y, arg = _run_forward(Ai, Xi, mat.m, k, dtype, "max", True)
        assert np.array_equal(arg, R.forward(mat, ival, Xi, "max", True)[1])
        rc, dX, dval = _backward(Ai, Xi, dYi, arg, mat.n, mat.nnz, k, dtype, True)
        assert rc == 0, _capi.last_error()
        ref, w, mag = R.dx(mat, ival, dYi, arg, True)
        assert mag.max() < 2 ** 24
        assert R.same_bits(dX, ref.astype(dtype)), (which, k, "dX on integers")
        cols, rows = mat.col[:mat.nnz].astype(np.int64), R.rows_of(mat)
        want = ((arg[rows] == np.arange(mat.nnz)[:, None]) * Xi[cols].astype(np.float64) * dYi[rows]).sum(1)
        assert R.same_bits(dval, want.astype(dtype)), (which, k, "dval on integers")
    _close(A)
    _close(Ai)


# ---- 4. handle state --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_handle_state(dtype, tmp_path):
    mat = _matrices()[0]
    k = 17
    val = _values(0, dtype)
    X = _x(0, dtype, k)
    dY = np.random.default_rng(61).uniform(-1, 1, size=(mat.m, k)).astype(dtype)
    A, _ = _handle(mat, val, PATH["slabs8-hot"], dtype)
    assert A.buildTranspose() == 0
    x = torch.from_numpy(np.random.default_rng(62).uniform(-1, 1, mat.n).astype(dtype)).to(DEV)
    y0, y1 = (torch.zeros(mat.m, dtype=_tdt(dtype), device=DEV) for _ in range(2))
    assert A.setX(x) == 0 and A.spmv(1.0, y0) == 0
    torch.cuda.synchronize()
    before = bytes(A.info())
    Y, arg = _run_forward(A, X, mat.m, k, dtype, "max", True)
    rc, dX, dval = _backward(A, X, dY, arg, mat.n, mat.nnz, k, dtype, True)
    assert rc == 0, _capi.last_error()
    assert bytes(A.info()) == before  # csr5hip_info, device_bytes included
    assert A.spmv(1.0, y1) == 0
    torch.cuda.synchronize()
    assert torch.equal(y0.view(torch.uint8), y1.view(torch.uint8))

    # a handle restored from a checkpoint gives the fresh handle's bits
    path = str(tmp_path / "reduce.csr5")
    assert A.save(path) == 0, _capi.last_error()
    B = H.anonymouslibHandle.load(path)
    Yb, argb = _run_forward(B, X, mat.m, k, dtype, "max", True)
    assert R.same_bits(Yb, Y) and np.array_equal(argb, arg)
    assert B.buildTranspose() == 0
    rc, dXb, dvalb = _backward(B, X, dY, arg, mat.n, mat.nnz, k, dtype, True)
    assert rc == 0 and R.same_bits(dXb, dX) and R.same_bits(dvalb, dval)
    B.close()

    # new values: the row kernel and the column kernel both use them
    new = R.distinct_values(mat.nnz, dtype, seed=99)
    assert A.updateValues(torch.from_numpy(new).to(DEV)) == 0, _capi.last_error()
    Y2, arg2 = _run_forward(A, X, mat.m, k, dtype, "min", True)
    Yr, argr = R.forward(mat, new, X, "min", True)
    assert R.same_bits(Y2, Yr) and np.array_equal(arg2, argr)
    rc, dX2, _ = _backward(A, X, dY, arg2, mat.n, mat.nnz, k, dtype, True)
    ref, w, mag = R.dx(mat, new, dY, arg2, True)
    assert rc == 0 and (np.abs(dX2.astype(np.float64) - ref) <= R.dx_bound(w, mag, dtype)).all()
    assert not (np.abs(dX2.astype(np.float64) - R.dx(mat, val, dY, arg2, True)[0]) <= R.dx_bound(w, mag, dtype)).all()  # (not the old ones)

    # the values come back unchanged
    assert A.asCSR() == 0
    torch.cuda.synchronize()
    assert np.array_equal(A._arrays[2].cpu().numpy(), new)
    assert np.array_equal(A._arrays[1].cpu().numpy(), mat.col[:mat.nnz])
    A.close()


# ---- 5. graph capture ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_graph_capture(dtype):
    """forward, dval and dX in one single-stream graph on the handle's stream, captured at the handle's FIRST calls; two replays
    with changed X both equal eager"""
    mat = _matrices()[0]
    k = 17
    A, _ = _handle(mat, _values(0, dtype), PATH["fused-default"], dtype)
    assert A.buildTranspose() == 0
    rng = np.random.default_rng(71)
    td = _tdt(dtype)
    X = torch.from_numpy(rng.uniform(-1, 1, size=(mat.n, k)).astype(dtype)).to(DEV)
    dY = torch.from_numpy(rng.uniform(-1, 1, size=(mat.m, k)).astype(dtype)).to(DEV)
    Y = torch.full((mat.m, k), Y_POISON, dtype=td, device=DEV)
    arg = torch.full((mat.m, k), ARG_POISON, dtype=torch.int32, device=DEV)
    dX = torch.full((mat.n, k), Y_POISON, dtype=td, device=DEV)
    dval = torch.full((mat.nnz,), Y_POISON, dtype=td, device=DEV)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert A.setStream(side) == 0
    held = A.info().device_bytes
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        assert A.spmmReduce(X, Y, "max", arg, True) == 0, _capi.last_error()
        assert A.spmmReduceBackward(X, dY, arg, dX, dval, True) == 0, _capi.last_error()
    assert A.info().device_bytes == held
    torch.cuda.synchronize()
    for seed in (72, 73):
        X.copy_(torch.from_numpy(np.random.default_rng(seed).uniform(-1, 1, size=(mat.n, k)).astype(dtype)).to(DEV))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in (Y, arg, dX, dval)]
        assert A.setStream(None) == 0
        eY, earg, edX, edval = (torch.empty_like(t) for t in (Y, arg, dX, dval))
        assert A.spmmReduce(X, eY, "max", earg, True) == 0 and A.spmmReduceBackward(X, dY, earg, edX, edval, True) == 0
        torch.cuda.synchronize()
        for g, e in zip(got, (eY, earg, edX, edval)):
            assert torch.equal(g.view(torch.uint8), e.view(torch.uint8))
        Yr, argr = R.forward(mat, _values(0, dtype), X.cpu().numpy(), "max", True)
        assert R.same_bits(got[0].cpu().numpy(), Yr) and np.array_equal(got[1].cpu().numpy(), argr)
        assert A.setStream(side) == 0
    del graph
    assert A.setStream(None) == 0
    _close(A)


# ---- 6. autograd ---------------------------------------------------------------------------------------------------------------------------
def _torch_route(mat, val, X, reduce):
    rows = torch.from_numpy(R.rows_of(mat)).to(DEV)
    cols = torch.from_numpy(mat.col[:mat.nnz].astype(np.int64)).to(DEV)
    t = X[cols] * val[:, None] if val is not None else X[cols]
    out = torch.zeros((mat.m, X.shape[1]), dtype=X.dtype, device=DEV)
    return out.scatter_reduce(0, rows[:, None].expand(-1, X.shape[1]), t, "amax" if reduce == "max" else "amin", include_self=False)


@pytest.mark.parametrize("reduce", ("max", "min"))
def test_autograd_against_torch(reduce):
    mat = _matrices()[0]
    k = 6
    rng = np.random.default_rng(81)
    A, _ = _handle(mat, np.ones(mat.nnz), PATH["fused-default"], np.float64)
    val = torch.from_numpy(R.distinct_values(mat.nnz, np.float64, seed=82)).to(DEV).requires_grad_(True)
    X = torch.from_numpy(rng.uniform(-1, 1, size=(mat.n, k))).to(DEV).requires_grad_(True)
    G = torch.from_numpy(rng.uniform(-1, 1, size=(mat.m, k))).to(DEV)
    Y = AG.spmm_reduce(A, val, X, reduce)
    want = _torch_route(mat, val, X, reduce)
    assert torch.equal(Y, want)
    t = R.terms(mat, val.detach().cpu().numpy(), X.detach().cpu().numpy(), True)
    tied = np.zeros((mat.m, k), dtype=np.int64)
    np.add.at(tied, R.rows_of(mat), (t == Y.detach().cpu().numpy()[R.rows_of(mat)]).astype(np.int64))
    assert tied.max() == 1, "the gradients are compared where the forward has no ties: everywhere, on this data"
    gv, gx = torch.autograd.grad(Y, (val, X), G)
    wv, wx = torch.autograd.grad(want, (val, X), G)
    assert torch.allclose(gv, wv, rtol=1e-13, atol=1e-15)  # (equal to rounding: the two sides sum in their own orders)
    assert torch.allclose(gx, wx, rtol=1e-13, atol=1e-15)

    # unweighted: the handle's values and the record of them are left alone
    key = A._autograd_key
    assert key is not None
    Xu = X.detach().clone().requires_grad_(True)
    Yu, arg = AG.spmm_reduce(A, None, Xu, reduce, return_arg=True)
    assert torch.equal(Yu, _torch_route(mat, None, Xu, reduce)) and arg.dtype == torch.int32
    (gu,) = torch.autograd.grad(Yu, (Xu,), G)
    (wu,) = torch.autograd.grad(_torch_route(mat, None, Xu, reduce), (Xu,), G)
    assert torch.allclose(gu, wu, rtol=1e-13, atol=1e-15)
    assert A._autograd_key == key
    Y2 = torch.empty_like(Y)
    assert A.spmmReduce(X.detach(), Y2, reduce, None, True) == 0  # (the handle still holds val)
    torch.cuda.synchronize()
    assert torch.equal(Y2, Y.detach())
    _close(A)


def test_autograd_gradcheck():
    rng = np.random.default_rng(91)
    lengths = np.array([3, 0, 5, 1, 9, 2, 0, 4, 7, 1, 6, 2])
    mat = M.csr_from_row_lengths(lengths, 9, rng, name="gradcheck-12x9")
    A, _ = _handle(mat, np.ones(mat.nnz), PATH["two-pass-s4"], np.float64)
    # distinct products, far apart compared with gradcheck's step: a permutation of a grid in val and in X
    val = torch.from_numpy((rng.permutation(mat.nnz) + 1.0) / mat.nnz + 0.5).to(DEV).requires_grad_(True)
    X = torch.from_numpy((rng.permutation(9 * 3).reshape(9, 3) + 1.0) * 0.37).to(DEV).requires_grad_(True)
    t = R.terms(mat, val.detach().cpu().numpy(), X.detach().cpu().numpy(), True)
    for i in range(mat.m):
        seg = np.sort(t[mat.row_ptr[i]:mat.row_ptr[i + 1]], axis=0)
        assert seg.shape[0] < 2 or np.diff(seg, axis=0).min() > 1e-3, "products too close for a finite difference"
    for reduce in ("max", "min"):
        # (gradcheck perturbs through ``.data``, which does not move ``_version``: the clone hands every evaluation its own tensor)
        assert torch.autograd.gradcheck(lambda v, x: AG.spmm_reduce(A, v.clone(), x.clone(), reduce), (val, X))
        assert torch.autograd.gradcheck(lambda x: AG.spmm_reduce(A, None, x.clone(), reduce), (X,))
    _close(A)
