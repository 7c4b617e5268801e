"""row_softmax and row_softmax_grad on the GPU against the reference of tests/softmax_reference.py: every stored element of every
matrix on every dataset in both precisions; bit-identical in CSR format, on every converted path, one element off the
allocation and wherever the row stands in the matrix; nothing written besides the nnz outputs and nothing changed in the handle;
the result fed back through updateValues; graph capture."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from benchmark_spmv_using_csr5_amd import _capi  # noqa: E402
from benchmark_spmv_using_csr5_amd import handle as H  # noqa: E402
from benchmark_spmv_using_csr5_amd import matrices as M  # noqa: E402
from tests import sddmm_reference as S  # noqa: E402
from tests import softmax_reference as R  # noqa: E402
from tests.exact_reference import unit_roundoff  # noqa: E402
from tests.test_gpu_exact_reference import DEV, PATHS, _close, _handle, _matrices  # noqa: E402

POISON = 777.0
GUARD = -12345.0
BY_NAME = {p.name: p for p in PATHS}
GROUPS = 3


def _dt(dtype):
    return "fp64" if dtype == np.float64 else "fp32"


def _tdt(dtype):
    return torch.float64 if dtype == np.float64 else torch.float32


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


@functools.lru_cache(maxsize=1)
def _all_matrices():
    """every matrix of the exact-reference suite, its transpose, a matrix with repeated pairs and empty rows, and one with a row of
    200 003 entries next to rows of 0, 1, 2, 3, 63, 64, 65 entries and of every class boundary of the kernel"""
    base = list(_matrices())
    return tuple(base + [M.transpose_csr(m) for m in base] + [S.duplicates_matrix(), R.hub_matrix()])


def _csr_handle(row_ptr, n, dtype):
    """a handle in CSR format (never converted) on a device copy of row_ptr; the columns and values are never read"""
    rp = torch.from_numpy(np.asarray(row_ptr, dtype=np.int32)).to(DEV)
    nnz = int(row_ptr[-1])
    ci = torch.zeros(max(nnz, 1), dtype=torch.int32, device=DEV)
    va = torch.zeros(max(nnz, 1), dtype=_tdt(dtype), device=DEV)
    A = H.anonymouslibHandle(len(row_ptr) - 1, n, dtype=np.dtype(dtype).name)
    A._arrays = (rp, ci, va)
    assert A.inputCSR(nnz, rp, ci, va) == 0
    return A


def _buffer(values, offset, dtype):
    """the values `offset` elements into an allocation of their own"""
    b = torch.full((offset + values.size,), float("nan"), dtype=_tdt(dtype), device=DEV)
    b[offset:] = torch.from_numpy(np.ascontiguousarray(values)).to(DEV)
    return b[offset:]


def _run(A, dtype, scores=None, p=None, g=None, offset=0):
    """the forward on `scores`, or the gradient on (p, g): nnz outputs; out is preset to POISON, lies `offset` elements into its
    allocation and is followed by one guard element, which must survive"""
    nnz = (scores if scores is not None else p).size
    ob = torch.full((offset + nnz + 1,), POISON, dtype=_tdt(dtype), device=DEV)
    ob[-1] = GUARD
    out = ob[offset:offset + nnz]
    if scores is not None:
        rc = A.rowSoftmax(_buffer(scores, offset, dtype), out)
    else:
        rc = A.rowSoftmaxGrad(_buffer(p, offset, dtype), _buffer(g, offset, dtype), out)
    assert rc == 0, _capi.last_error()
    torch.cuda.synchronize()
    got = ob.cpu().numpy()
    assert got[-1] == dtype(GUARD), "the element behind out was written"
    assert (got[:offset] == dtype(POISON)).all(), "an element in front of out was written"
    return got[offset:-1].copy()


def _fields(A):
    i = A.info()
    return {f[0]: getattr(i, f[0]) for f in i._fields_}


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_dt)
@pytest.mark.parametrize("group", range(GROUPS))
def test_row_softmax_forward_every_element(group, dtype):
    for mi, mat in enumerate(_all_matrices()):
        if mi % GROUPS != group:
            continue
        A, _ = _handle(mat, np.ones(mat.nnz, dtype=dtype), BY_NAME["fused-default"], dtype)
        before = _fields(A)
        for dataset in R.FORWARD_DATASETS:
            s = R.make_scores(dataset, mat.row_ptr, dtype, seed=3 + mi)
            got = _run(A, dtype, scores=s)
            ref = R.softmax_reference(mat.row_ptr, s, dataset)
            what = f"{mat.name} {dataset} {_dt(dtype)}"
            r = R.ratios(got, ref)
            print(f"{what}: worst |error| / bound {r.max() if r.size else 0.0:.3f}")
            R.check(got, ref, what)
            if dataset == "shifted":
                a, b = R.shifted_pair(mat.row_ptr, dtype, seed=3 + mi)
                assert np.array_equal(a, s)
                got_b = _run(A, dtype, scores=b)
                assert np.array_equal(_bits(got_b), _bits(got)), what
                R.check(got_b, R.softmax_reference(mat.row_ptr, b, dataset), what + " + row shift")
        after = _fields(A)
        assert after == before and after["device_bytes"] == before["device_bytes"], mat.name
        _close(A)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_dt)
@pytest.mark.parametrize("group", range(GROUPS))
def test_row_softmax_grad_every_element(group, dtype):
    for mi, mat in enumerate(_all_matrices()):
        if mi % GROUPS != group:
            continue
        A, _ = _handle(mat, np.ones(mat.nnz, dtype=dtype), BY_NAME["two-pass-s7"], dtype)
        before = _fields(A)
        for dataset in R.GRAD_DATASETS:
            p, g = R.make_grad(dataset, mat.row_ptr, dtype, seed=3 + mi)
            got = _run(A, dtype, p=p, g=g)
            ref = R.grad_reference(mat.row_ptr, p, g, dataset)
            what = f"{mat.name} grad {dataset} {_dt(dtype)}"
            r = R.ratios(got, ref)
            print(f"{what}: worst |error| / bound {r.max() if r.size else 0.0:.3f}")
            R.check(got, ref, what)
        # p and g may be one array
        p, _g = R.make_grad("softmax", mat.row_ptr, dtype, seed=3 + mi)
        nnz = p.size
        pd = _buffer(p, 0, dtype)
        out = torch.full((nnz,), POISON, dtype=_tdt(dtype), device=DEV)
        assert A.rowSoftmaxGrad(pd, pd, out) == 0
        torch.cuda.synchronize()
        R.check(out.cpu().numpy(), R.grad_reference(mat.row_ptr, p, p), f"{mat.name} p = g")
        after = _fields(A)
        assert after == before and after["device_bytes"] == before["device_bytes"], mat.name
        _close(A)


def _hard(mat, dtype, seed):
    """scores and gradient data whose sums round: gaussian scores; the reference softmax of them and N(0, 1)"""
    s = R.make_scores("gaussian", mat.row_ptr, dtype, seed=seed)
    p, g = R.make_grad("softmax", mat.row_ptr, dtype, seed=seed)
    return s, p, g


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_dt)
def test_bits_do_not_depend_on_format_path_or_alignment(dtype):
    """the handle in CSR format gives the bits that every entry of PATHS gives after conversion, and the bits do not move with
    the pointers one or two elements off their allocation"""
    names = ("hub", "half-empty", "scircuit-like(synthetic)", "duplicates", "hub-row")
    picks = [m for m in _all_matrices() if m.name in names]
    assert sorted(m.name for m in picks) == sorted(names)
    for mat in picks:
        s, p, g = _hard(mat, dtype, seed=21)
        A = _csr_handle(mat.row_ptr, mat.n, dtype)
        assert A.info().format == _capi.FORMAT_CSR
        base_f, base_g = _run(A, dtype, scores=s), _run(A, dtype, p=p, g=g)
        R.check(base_f, R.softmax_reference(mat.row_ptr, s), f"{mat.name} CSR format")
        R.check(base_g, R.grad_reference(mat.row_ptr, p, g), f"{mat.name} CSR format, gradient")
        for off in (1, 2, 3):
            assert np.array_equal(_bits(_run(A, dtype, scores=s, offset=off)), _bits(base_f)), (mat.name, off)
            assert np.array_equal(_bits(_run(A, dtype, p=p, g=g, offset=off)), _bits(base_g)), (mat.name, off)
        A.close()
        for path in (PATHS if mat.name != "hub-row" else [BY_NAME["two-pass-s4"], BY_NAME["fused-default"]]):
            B, _ = _handle(mat, np.ones(mat.nnz, dtype=dtype), path, dtype)
            assert B.info().format == _capi.FORMAT_CSR5
            assert np.array_equal(_bits(_run(B, dtype, scores=s)), _bits(base_f)), (mat.name, path.name)
            assert np.array_equal(_bits(_run(B, dtype, p=p, g=g)), _bits(base_g)), (mat.name, path.name)
            assert B.asCSR() == 0  # back in CSR format: the same again
            assert np.array_equal(_bits(_run(B, dtype, scores=s)), _bits(base_f)), (mat.name, path.name)
            B.close()


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_dt)
def test_bits_do_not_depend_on_the_position_of_the_row(dtype):
    """a second matrix holds the rows in reversed order (other m-relative positions, other neighbours, other lanes, other
    workgroups), the scores permuted to match: the same bits row for row"""
    for mat in [m for m in _all_matrices() if m.name in ("hub", "half-empty", "duplicates", "hub-row")]:
        rp = np.asarray(mat.row_ptr, dtype=np.int64)
        lens = np.diff(rp)
        rev_rp = np.concatenate([[0], np.cumsum(lens[::-1])])
        # element e of the reversed matrix = element perm[e] of the first
        perm = np.concatenate([np.arange(rp[r], rp[r + 1]) for r in range(lens.size - 1, -1, -1)] + [np.zeros(0, dtype=np.int64)])
        s, p, g = _hard(mat, dtype, seed=22)
        A, B = _csr_handle(rp, mat.n, dtype), _csr_handle(rev_rp, mat.n, dtype)
        f1, f2 = _run(A, dtype, scores=s), _run(B, dtype, scores=s[perm])
        g1, g2 = _run(A, dtype, p=p, g=g), _run(B, dtype, p=p[perm], g=g[perm])
        assert np.array_equal(_bits(f1[perm]), _bits(f2)), mat.name
        assert np.array_equal(_bits(g1[perm]), _bits(g2)), mat.name
        # and with other neighbours altogether: every row alone in a matrix of one row (three rows of each matrix)
        for r in np.flatnonzero(lens > 0)[[0, -1]].tolist() + [int(np.argmax(lens))]:
            C_ = _csr_handle(np.array([0, lens[r]]), mat.n, dtype)
            alone = _run(C_, dtype, scores=s[rp[r]:rp[r + 1]])
            assert np.array_equal(_bits(alone), _bits(f1[rp[r]:rp[r + 1]])), (mat.name, r)
            C_.close()
        A.close()
        B.close()


def test_empty_matrices_and_empty_rows_write_nothing():
    dtype = np.float64
    for m in (5, 0):
        A = _csr_handle(np.zeros(m + 1, dtype=np.int64), 5, dtype)
        guard = torch.full((1,), GUARD, dtype=torch.float64, device=DEV)
        assert A.rowSoftmax(guard[:0], guard[:0].clone()) == 0
        assert A.rowSoftmax_ptr(0, 0) == 0 and A.rowSoftmaxGrad_ptr(0, 0, 0) == 0
        torch.cuda.synchronize()
        assert guard.item() == GUARD
        A.close()
    # rows of one entry between empty rows: exactly 1 each, whatever the score
    lens = np.array([0, 1, 0, 0, 1, 1, 0])
    A = _csr_handle(np.concatenate([[0], np.cumsum(lens)]), 5, dtype)
    got = _run(A, dtype, scores=np.array([-1e300, 0.0, 1.7976931348623157e308]))
    assert np.array_equal(got, np.ones(3))
    A.close()


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_dt)
def test_result_feeds_update_values(dtype):
    """updateValues of the softmax, then spmv with x = ones: every non-empty row sums to 1 within the forward bound summed over
    the row plus the product's own summation error gamma(L) * sum |p| (any order; Higham section 4.2)"""
    u = unit_roundoff(dtype)
    for mat in [m for m in _all_matrices() if m.name in ("hub", "half-empty", "duplicates", "hub-row")]:
        A, _ = _handle(mat, np.ones(mat.nnz, dtype=dtype), BY_NAME["fused-default"], dtype)
        s = R.make_scores("gaussian", mat.row_ptr, dtype, seed=8)
        sd = _buffer(s, 0, dtype)
        out = torch.full((mat.nnz,), POISON, dtype=_tdt(dtype), device=DEV)
        x = torch.ones(mat.n, dtype=_tdt(dtype), device=DEV)
        y = torch.full((mat.m,), POISON, dtype=_tdt(dtype), device=DEV)
        assert A.rowSoftmax(sd, out) == 0 and A.updateValues(out) == 0
        assert A.setX(x) == 0 and A.spmv(1.0, y) == 0
        torch.cuda.synchronize()
        ref = R.softmax_reference(mat.row_ptr, s)
        R.check(out.cpu().numpy(), ref, mat.name)
        lens, starts, nlens, _rows = R._rows(mat.row_ptr)
        allowed = np.add.reduceat(ref.bound, starts).astype(np.float64) + (nlens * u / (1 - nlens * u)) * (1 + 1e-3)
        got = y.cpu().numpy()[lens > 0].astype(np.float64)
        worst = np.abs(got - 1.0) / allowed
        print(f"{mat.name} {_dt(dtype)}: row sums, worst |sum - 1| / allowed {worst.max():.3f}")
        assert (worst <= 1).all(), (mat.name, np.flatnonzero(worst > 1)[:5], got[worst > 1][:5])
        _close(A)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_dt)
def test_both_calls_are_captured_in_a_graph(dtype):
    """one linear chain on the handle's stream; the handle's very first calls are the captured ones (enqueue-only from the first
    call on: a host synchronisation or an allocation inside the call would break the capture)"""
    mat = [m for m in _all_matrices() if m.name == "half-empty"][0]
    s, p, g = _hard(mat, dtype, seed=23)
    A, _ = _handle(mat, np.ones(mat.nnz, dtype=dtype), BY_NAME["fused-default"], dtype)
    sd, gd = _buffer(s, 0, dtype), _buffer(g, 0, dtype)
    pd = torch.full((mat.nnz,), POISON, dtype=_tdt(dtype), device=DEV)
    dd = torch.full((mat.nnz,), POISON, dtype=_tdt(dtype), device=DEV)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert A.setStream(side) == 0
    held = A.info().device_bytes
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        assert A.rowSoftmax(sd, pd) == 0, _capi.last_error()
        assert A.rowSoftmaxGrad(pd, gd, dd) == 0, _capi.last_error()
    assert A.info().device_bytes == held
    torch.cuda.synchronize()
    for _ in range(2):
        pd.fill_(POISON)
        dd.fill_(POISON)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        rp_, rd_ = pd.cpu().numpy(), dd.cpu().numpy()
        R.check(rp_, R.softmax_reference(mat.row_ptr, s), "replay")
    del graph
    assert A.setStream(None) == 0
    eager_p = _run(A, dtype, scores=s)
    eager_d = _run(A, dtype, p=eager_p, g=g)
    assert np.array_equal(_bits(eager_p), _bits(rp_)) and np.array_equal(_bits(eager_d), _bits(rd_))
    _close(A)
