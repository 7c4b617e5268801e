"""sddmm on the GPU against the reference of tests/sddmm_reference.py: every stored element of every matrix, on every dataset, on
handles converted for a representative set of SpMV paths; bit-identical across ALL paths, paddings and alignments; the layout
corners (tail only, fast-track only, exactly full last tile, nothing at all); the handle untouched; graph capture."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from benchmark_spmv_using_csr5_amd import _capi  # noqa: E402
from benchmark_spmv_using_csr5_amd import handle as H  # noqa: E402
from benchmark_spmv_using_csr5_amd import matrices as M  # noqa: E402
from tests import sddmm_reference as S  # noqa: E402
from tests import zoo  # noqa: E402
from tests.test_gpu_exact_reference import DEV, PATHS, Path, _close, _handle, _matrices  # noqa: E402

KS = (1, 3, 8, 13, 40)
POISON = 777.0
GUARD = -12345.0
EXACT_PATHS = ("two-pass-s4", "two-pass-s7", "two-pass-s32", "fused-default", "xwin-narrow", "slabs8-hot", "zero-empty")
BY_NAME = {p.name: p for p in PATHS}
GROUPS = 4


def _dt(dtype):
    return "fp64" if dtype == np.float64 else "fp32"


def _tdt(dtype):
    return torch.float64 if dtype == np.float64 else torch.float32


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=1)
def _all_matrices():
    """every matrix of the exact-reference suite (hub rows, rows over 64 tiles, p = 1, 78 % empty rows ...), its transpose (hub
    columns become hub rows and the other way round) and a matrix with repeated (row, column) pairs"""
    base = list(_matrices())
    return tuple(base + [M.transpose_csr(m) for m in base] + [S.duplicates_matrix()])


def _ones(mat, dtype):
    return np.ones(mat.nnz, dtype=dtype)


def _sddmm(A, mat, U, V, dtype, ldu=None, ldv=None, offset=0):
    """out (nnz,) of A.sddmm with U / V at leading dimensions ldu / ldv (padding columns NaN), `offset` elements into their
    allocations; out preset to POISON and followed by one guard element, which must survive"""
    k = U.shape[1]
    ldu, ldv = ldu or k, ldv or k
    tdt = _tdt(dtype)
    Ub = torch.full((offset + mat.m * ldu,), float("nan"), dtype=tdt, device=DEV)
    Vb = torch.full((offset + mat.n * ldv,), float("nan"), dtype=tdt, device=DEV)
    Uv, Vv = Ub[offset:].view(mat.m, ldu), Vb[offset:].view(mat.n, ldv)
    if k:
        Uv[:, :k] = _dev(U)
        Vv[:, :k] = _dev(V)
    ob = torch.full((offset + mat.nnz + 1,), POISON, dtype=tdt, device=DEV)
    ob[-1] = GUARD
    assert A.sddmm_ptr(Uv, ldu, Vv, ldv, k, ob[offset:]) == 0, _capi.last_error()
    torch.cuda.synchronize()
    got = ob.cpu().numpy()
    assert got[-1] == dtype(GUARD), "the element behind out was written"
    assert (got[:offset] == dtype(POISON)).all()
    return got[offset:-1].copy()


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
@pytest.mark.parametrize("group", range(GROUPS))
def test_sddmm_exact(group, dtype):
    """all nnz outputs of every matrix x dataset x k on seven differently converted handles"""
    for mi, mat in enumerate(_all_matrices()):
        if mi % GROUPS != group:
            continue
        handles = [_handle(mat, _ones(mat, dtype), BY_NAME[name], dtype)[0] for name in EXACT_PATHS]
        for dataset in S.DATASETS:
            for k in KS:
                U, V = S.make(dataset, mat, k, dtype, seed=5 + mi)
                ref = S.reference(dataset, mat, U, V)
                Ud, Vd = _dev(U), _dev(V)
                for name, A in zip(EXACT_PATHS, handles):
                    ob = torch.full((mat.nnz + 1,), POISON, dtype=_tdt(dtype), device=DEV)
                    ob[-1] = GUARD
                    assert A.sddmm(Ud, Vd, ob[:mat.nnz]) == 0, _capi.last_error()
                    torch.cuda.synchronize()
                    got = ob.cpu().numpy()
                    assert got[-1] == dtype(GUARD), (name, mat.name)
                    S.check(got[:-1], ref, f"{name} {mat.name} {dataset} {_dt(dtype)} k {k}")
        for A in handles:
            _close(A)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_sddmm_is_bit_identical_on_every_path(dtype):
    """wide_range data (the sum rounds): every entry of PATHS gives the bits of two-pass-s4.  Two elements whose U rows and V rows
    are equal give equal bits: the first element and up to three others that share neither row nor column with it (the first,
    the middle and the last such element, so one of them lies in or next to the tail) get copies of its two rows."""
    k = 13  # fp64: three whole blocks + a remainder of one column; fp32: one whole block + a remainder of five
    for mi, mat in enumerate(_matrices()):
        U, V = S.make("wide_range", mat, k, dtype, seed=40 + mi)
        rows, cols = S.rows_of(mat), mat.col[:mat.nnz]
        e0 = 0
        picked = [e0]
        free = np.flatnonzero((rows != rows[e0]) & (cols != cols[e0]))  # elements that share neither row nor column with e0
        for e in (free[[0, free.size // 2, -1]].tolist() if free.size else []):
            # (a row or column already rewritten stays as it is)
            if rows[e] not in rows[picked] and cols[e] not in cols[picked]:
                U[rows[e]] = U[rows[e0]]
                V[cols[e]] = V[cols[e0]]
                picked.append(e)
        assert len(picked) >= 2 or mat.name in ("one-row", "single-nnz"), (mat.name, picked)
        ref = S.reference("wide_range", mat, U, V)
        base = None
        for path in PATHS:
            A, _ = _handle(mat, _ones(mat, dtype), path, dtype)
            got = _sddmm(A, mat, U, V, dtype)
            _close(A)
            if base is None:
                assert path.name == "two-pass-s4"
                S.check(got, ref, f"{mat.name} wide_range")
                base = got
                assert (_bits(got[picked]) == _bits(got[picked[:1]])[0]).all(), (mat.name, picked)
            assert np.array_equal(_bits(got), _bits(base)), (path.name, mat.name)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_sddmm_does_not_depend_on_padding_or_alignment(dtype):
    """(ldu, ldv) = (k, k) against (k + 1, k + 3) with NaN in the padding, and against pointers one element off"""
    names = ("hub", "hub^T", "half-empty", "aligned1024^T", "scircuit-like(synthetic)", "duplicates")
    picks = [m for m in _all_matrices() if m.name in names]
    assert sorted(m.name for m in picks) == sorted(names)
    for mat in picks:
        A, _ = _handle(mat, _ones(mat, dtype), BY_NAME["two-pass-s7"], dtype)
        for k in KS:
            U, V = S.make("wide_range", mat, k, dtype, seed=3)
            base = _sddmm(A, mat, U, V, dtype)
            S.check(base, S.reference("wide_range", mat, U, V), f"{mat.name} k {k}")
            for ldu, ldv, off in ((k + 1, k + 3, 0), (k, k, 1), (k + 4, k + 8, 2)):
                got = _sddmm(A, mat, U, V, dtype, ldu, ldv, off)
                assert np.array_equal(_bits(got), _bits(base)), (mat.name, k, ldu, ldv, off)
        _close(A)


def _lens(name, lengths, n, seed):
    return M.csr_from_row_lengths(np.asarray(lengths), n, np.random.default_rng(seed), name=name)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_sddmm_layout_corners(dtype):
    corners = [
        (_lens("tail-only", [2, 0, 3, 1, 5, 0, 4, 4], 8, 1), 4),          # 19 elements: p = 1
        (_lens("one-row", [3000], 3000, 12), 4),                            # every tile 0 .. p-2 is fast-track
        (_lens("one-row-s16", [5000], 700, 13), 16),
        (_lens("full-last-tile", [64] * 300, 512, 8), 4),                   # 19 200 = 75 x 256
        (_lens("full-only-tile", [16] * 16, 16, 2), 4),                     # 256 elements: p = 1 and full
        (_lens("long-then-short", [700, 0, 0, 1, 300, 2, 0], 900, 3), 4),   # fast-track tiles between ordinary ones
    ]
    for mat, sigma in corners:
        A, info = _handle(mat, _ones(mat, dtype), Path("corner", sigma, H.SPMV_TWO_PASS), dtype)
        assert info.p == -(-mat.nnz // (64 * sigma))
        for dataset in ("integer", "nonfinite"):
            for k in (5, 8):
                U, V = S.make(dataset, mat, k, dtype, seed=9)
                S.check(_sddmm(A, mat, U, V, dtype), S.reference(dataset, mat, U, V), f"{mat.name} {dataset} k {k}")
        # k = 0: +0 everywhere, U and V not needed
        got = _sddmm(A, mat, np.zeros((mat.m, 0), dtype=dtype), np.zeros((mat.n, 0), dtype=dtype), dtype)
        assert not _bits(got).any(), mat.name
        ob = torch.full((mat.nnz,), POISON, dtype=_tdt(dtype), device=DEV)
        assert A.sddmm_ptr(0, 0, 0, 0, 0, ob) == 0
        torch.cuda.synchronize()
        assert not _bits(ob.cpu().numpy()).any()
        _close(A)
    # nothing stored: a successful no-op, with and without rows
    for m, n in ((5, 5), (0, 5), (5, 0)):
        mat = M.CsrMatrix(m, n, np.zeros(m + 1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=dtype), "empty")
        A, _ = _handle(mat, _ones(mat, dtype), Path("empty", 4, H.SPMV_TWO_PASS), dtype)
        U, V = S.make("integer", mat, 3, dtype)
        guard = torch.full((1,), GUARD, dtype=_tdt(dtype), device=DEV)
        assert A.sddmm(_dev(U), _dev(V), guard[:0]) == 0
        assert A.sddmm_ptr(0, 3, 0, 3, 3, 0) == 0
        torch.cuda.synchronize()
        assert guard.item() == GUARD
        _close(A)


@pytest.mark.parametrize("name", ("two-pass-s7", "fused-default", "slabs8-hot"))
def test_sddmm_leaves_the_handle_untouched(name):
    dtype = np.float64
    mat = [m for m in _matrices() if m.name == "half-empty"][0]
    rng = np.random.default_rng(2)
    val = rng.integers(1, 10, size=mat.nnz).astype(dtype)
    x = rng.integers(0, 10, size=mat.n).astype(dtype)
    A, _ = _handle(mat, val, BY_NAME[name], dtype)
    xd = _dev(x)
    assert A.setX(xd) == 0

    def spmv():
        yd = torch.full((mat.m,), POISON, dtype=torch.float64, device=DEV)
        assert A.spmv(1.0, yd) == 0
        torch.cuda.synchronize()
        return yd.cpu().numpy()

    def fields():
        i = A.info()
        return {f[0]: getattr(i, f[0]) for f in i._fields_}
    y0, before = spmv(), fields()
    for k in (3, 8):
        U, V = S.make("wide_range", mat, k, dtype, seed=1)
        _sddmm(A, mat, U, V, dtype)
    after = fields()
    assert after == before and after["device_bytes"] == before["device_bytes"]
    assert np.array_equal(_bits(spmv()), _bits(y0))
    assert A.asCSR() == 0
    torch.cuda.synchronize()
    rp, ci, va = A._arrays
    assert np.array_equal(va.cpu().numpy(), val) and np.array_equal(ci.cpu().numpy(), mat.col[:mat.nnz])
    A.close()


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_sddmm_output_feeds_update_values(dtype):
    """sddmm into a tensor, updateValues of it, spmv == a handle built by hand from those values, bit for bit"""
    for mat in [m for m in _matrices() if m.name in ("half-empty", "hub", "nonsquare")] + [S.duplicates_matrix()]:
        for name in ("fused-default", "slabs8-hot"):
            U, V = S.make("integer", mat, 8, dtype, seed=6)
            x = np.random.default_rng(8).integers(0, 10, size=mat.n).astype(dtype)
            A, _ = _handle(mat, _ones(mat, dtype), BY_NAME[name], dtype)
            out = torch.full((mat.nnz,), POISON, dtype=_tdt(dtype), device=DEV)
            xd = _dev(x)
            y1 = torch.full((mat.m,), POISON, dtype=_tdt(dtype), device=DEV)
            assert A.sddmm(_dev(U), _dev(V), out) == 0 and A.updateValues(out) == 0
            assert A.setX(xd) == 0 and A.spmv(1.0, y1) == 0
            torch.cuda.synchronize()
            vals = out.cpu().numpy()
            S.check(vals, S.reference("integer", mat, U, V), mat.name)
            B, _ = _handle(mat, vals, BY_NAME[name], dtype)
            y2 = torch.full((mat.m,), POISON, dtype=_tdt(dtype), device=DEV)
            assert B.setX(xd) == 0 and B.spmv(1.0, y2) == 0
            torch.cuda.synchronize()
            assert np.array_equal(_bits(y1.cpu().numpy()), _bits(y2.cpu().numpy())), (mat.name, name)
            _close(A)
            _close(B)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_sddmm_is_captured_in_a_graph(dtype):
    """one linear chain on the handle's stream; the very first sddmm of the handle is the captured one (enqueue-only from the
    first call: a host synchronisation or an allocation inside the call would break the capture)"""
    mat = [m for m in _matrices() if m.name == "half-empty"][0]
    U, V = S.make("wide_range", mat, 13, dtype, seed=2)
    A, _ = _handle(mat, _ones(mat, dtype), BY_NAME["fused-default"], dtype)
    Ud, Vd = _dev(U), _dev(V)
    out = torch.full((mat.nnz,), POISON, dtype=_tdt(dtype), device=DEV)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert A.setStream(side) == 0
    held = A.info().device_bytes
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        assert A.sddmm(Ud, Vd, out) == 0, _capi.last_error()
    assert A.info().device_bytes == held
    torch.cuda.synchronize()
    for _ in range(2):
        out.fill_(POISON)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        replayed = out.cpu().numpy()
        S.check(replayed, S.reference("wide_range", mat, U, V), "replay")
    del graph
    assert A.setStream(None) == 0
    eager = _sddmm(A, mat, U, V, dtype)
    assert np.array_equal(_bits(eager), _bits(replayed))
    _close(A)
