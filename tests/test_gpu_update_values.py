"""updateValues: new values under an unchanged pattern must leave a handle exactly where a fresh conversion of the new values
would -- bit for bit, on every SpMV path of tests/test_gpu_exact_reference.py, for SpMM, spmv_repeat, save / load and asCSR,
through a captured graph and through the multi-GPU handle.

Values: V0 = wide_range, V1 = row_scaled (plus nonfinite and subnormal on the two-pass, fused-default, slabs8 and
slabs8-hot entries), each with the x its generator draws.  Every result is compared with a fresh handle of the same path
built from the new values and checked against the exact reference."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from benchmark_spmv_using_csr5_amd import _capi  # noqa: E402
from benchmark_spmv_using_csr5_amd import handle as H  # noqa: E402
from tests import exact_reference as R  # noqa: E402
from tests.test_gpu_exact_reference import (DEV, PATHS, Y0, Path, _bits, _case, _close, _dt, _handle, _matrices,  # noqa: E402
                                            _spmm_run, _spmv, _tdt)
from tests.test_gpu_multi import _devices  # noqa: E402

HARD = tuple(p.name for p in PATHS if p.name.startswith("two-pass-s")) + ("fused-default", "slabs8", "slabs8-hot")
BY_NAME = {p.name: p for p in PATHS}


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dtype))).to(DEV)


def _update(A, val, dtype):
    """updateValues from a fresh device copy of `val`; returns that copy (the library only reads it, asynchronously)"""
    vd = _dev(val, dtype)
    assert A.updateValues(vd) == 0, _capi.last_error()
    return vd


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


# rows that span more than 64 tiles (fast-track tiles: whole tiles inside one row), p = 1, short rows, hub columns
SOME = ("row-over-64-tiles", "tiny-p1", "scircuit-like(synthetic)", "hubcols1")


def _some():
    out = [i for n in SOME for i, m in enumerate(_matrices()) if m.name == n]
    assert len(out) == len(SOME), [m.name for m in _matrices()]
    return out


def _updated_against_fresh(path, dtype, datasets):
    """One handle per matrix, converted with V0 and multiplied once; per dataset: updateValues(V1), spmv with V1's x, and the
    same on a fresh handle built from V1.  Returns what differs between the two, as text (nothing = all equal)."""
    differs = []
    for mi, mat in enumerate(_matrices()):
        _, v0, X0, _ = _case(mi, "wide_range", dtype)
        A, info0 = _handle(mat, v0, path, dtype)
        _spmv(A, mat, X0[:, 0], dtype)
        for dataset in datasets:
            what = f"{path.name} {mat.name} {dataset} {_dt(dtype)}"
            _, v1, X1, refs = _case(mi, dataset, dtype)
            vd = _update(A, v1, dtype)
            y = _spmv(A, mat, X1[:, 0], dtype)
            info = A.info()
            if info.p >= 2:
                got = {f: getattr(info, f) for f in path.expect}
                assert got == path.expect, (what, got)
            assert (info.sigma, info.p, info.column_slabs, info.slab_hot) == (info0.sigma, info0.p, info0.column_slabs, info0.slab_hot)
            B, _ = _handle(mat, v1, path, dtype)
            yB = _spmv(B, mat, X1[:, 0], dtype)
            # the handle's own value array (the caller's tensor, in tile order while converted) is the fresh handle's
            assert _same(A._arrays[2].cpu().numpy(), B._arrays[2].cpu().numpy()), what
            R.check(y, refs[0], R.empty_zero_rows(mat.m, info.tail_partition_start, path.zero_empty), Y0, what)
            assert _same(vd.cpu().numpy(), v1.astype(dtype)), what  # the caller's array is only read
            if not _same(y, yB):
                rows = np.flatnonzero(_bits(y) != _bits(yB))
                again = int((_bits(_spmv(B, mat, X1[:, 0], dtype)) != _bits(yB)).sum())
                differs.append(f"{what}: {rows.size} of {mat.m} rows, e.g. row {rows[0]}: {_bits(y)[rows[0]]:#x} / "
                               f"{_bits(yB)[rows[0]]:#x}; the fresh handle against its own second run: {again} rows")
            _close(B)
        _close(A)
    return differs


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_dt)
@pytest.mark.parametrize("path", PATHS, ids=lambda p: p.name)
def test_update_values_equals_fresh_handle_on_every_path(path, dtype):
    differs = _updated_against_fresh(path, dtype, ("row_scaled",))
    assert not differs, "\n".join(differs)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_dt)
@pytest.mark.parametrize("path", [p for p in PATHS if p.name in HARD], ids=lambda p: p.name)
def test_update_values_equals_fresh_handle_on_nonfinite_and_subnormal_data(path, dtype):
    """The same with V1 = nonfinite and V1 = subnormal, y compared bit for bit, NaN payloads and signs included.  (This needs
    the fused kernel to add the two partials of a row cut in two in tile order: csr5_carry.h carry_arrive, expected == 2.)"""
    differs = _updated_against_fresh(path, dtype, ("nonfinite", "subnormal"))
    assert not differs, "\n".join(differs)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_dt)
@pytest.mark.parametrize("name", ["fused-default", "ldsy", "zero-empty", "deferred-s7"])
def test_fused_spmv_repeats_its_nan_bits(name, dtype):
    """One handle, nonfinite data, ten SpMVs: y is the same bits every time.  Where two tiles each hold a NaN partial of one
    row, the sign of the sum used to follow the order in which the tiles arrived (nd24k-like fp32: up to 3 of 360 rows
    differed between two runs of one handle)."""
    path = BY_NAME[name]
    for mi, mat in enumerate(_matrices()):
        _, val, X, _ = _case(mi, "nonfinite", dtype)
        A, _ = _handle(mat, val, path, dtype)
        first = _spmv(A, mat, X[:, 0], dtype)
        for run in range(9):
            assert _same(_spmv(A, mat, X[:, 0], dtype), first), (name, mat.name, run)
        _close(A)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_dt)
@pytest.mark.parametrize("name", ["fused-default", "two-pass-s4", "slabs8", "slabs8-hot"])
def test_back_to_csr_and_twice_and_back(name, dtype):
    """asCSR after an update hands back the new values in CSR order and the original columns; V0 -> V1 -> V0 gives the first y
    again; after the first update no call changes the device memory the handle holds."""
    path = BY_NAME[name]
    for mi in _some():
        mat = _matrices()[mi]
        _, v0, X0, _ = _case(mi, "wide_range", dtype)
        _, v1, X1, _ = _case(mi, "row_scaled", dtype)
        A, _ = _handle(mat, v0, path, dtype)
        _, ci, va = A._arrays
        y0 = _spmv(A, mat, X0[:, 0], dtype)
        _update(A, v1, dtype)
        y1 = _spmv(A, mat, X1[:, 0], dtype)
        held = A.info().device_bytes
        _update(A, v0, dtype)
        assert _same(_spmv(A, mat, X0[:, 0], dtype), y0), (name, mat.name)
        vd = _update(A, v1, dtype)
        assert _same(_spmv(A, mat, X1[:, 0], dtype), y1), (name, mat.name)
        assert A.info().device_bytes == held, (name, mat.name)
        assert A.asCSR() == 0
        torch.cuda.synchronize()
        assert _same(va.cpu().numpy(), v1.astype(dtype)), (name, mat.name)
        assert np.array_equal(ci.cpu().numpy(), mat.col.astype(np.int32)), (name, mat.name)
        assert _same(vd.cpu().numpy(), v1.astype(dtype))
        # ... and a conversion of what came back is the fresh handle
        assert A.asCSR5() == 0
        assert _same(_spmv(A, mat, X1[:, 0], dtype), y1), (name, mat.name)
        _close(A)


def test_narrowed_values_are_redecided_by_every_update():
    """fp64, slabs + hot table, CSR5HIP_OPT_NARROW_VALUES: integers -> narrowed; one value that is no fp32 number -> not
    narrowed; integers again -> narrowed; y equals a fresh handle's each time."""
    mi = len(_matrices()) - 1
    mat = _matrices()[mi]
    hot = BY_NAME["slabs8-hot"]
    narrow = Path("narrow", 16, H.SPMV_FUSED, hot.opts + (("setNarrowValues", 1),), hot.expect)
    rng = np.random.default_rng(9)
    x = rng.integers(0, 10, size=mat.n).astype(np.float64)
    v0 = rng.integers(0, 10, size=mat.nnz).astype(np.float64)
    v1 = rng.integers(0, 10, size=mat.nnz).astype(np.float64)
    v1[rng.integers(0, mat.nnz)] = 2.0 ** 128
    v2 = rng.integers(0, 10, size=mat.nnz).astype(np.float64)
    A, info = _handle(mat, v0, narrow, np.float64)
    assert info.slab_values_narrowed == 1
    _spmv(A, mat, x, np.float64)
    yd = torch.empty(mat.m, dtype=torch.float64, device=DEV)
    for val, want in ((v1, 0), (v2, 1), (v1, 0), (v0, 1)):
        _update(A, val, np.float64)
        assert A.info().slab_values_narrowed == want
        y = _spmv(A, mat, x, np.float64)
        yd.fill_(Y0)
        assert A.spmv_repeat(1.0, yd, 2) == 0  # (a library-owned graph recorded under the other outcome must not be replayed)
        torch.cuda.synchronize()
        B, infoB = _handle(mat, val, narrow, np.float64)
        assert infoB.slab_values_narrowed == want
        yB = _spmv(B, mat, x, np.float64)
        assert _same(y, yB) and _same(yd.cpu().numpy(), yB), want
        R.check(y, R.reference("wide_range", mat, val, x), R.empty_zero_rows(mat.m, infoB.tail_partition_start), Y0,
                f"narrowed {want}")
        _close(B)
    _close(A)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_dt)
@pytest.mark.parametrize("name", ["fused-default", "slabs8-hot"])
def test_spmm_repeat_and_checkpoint_after_an_update(name, dtype, tmp_path):
    path = BY_NAME[name]
    for mi in _some():
        mat = _matrices()[mi]
        _, v0, _, _ = _case(mi, "wide_range", dtype)
        _, v1, X, _ = _case(mi, "row_scaled", dtype, k=8)
        A, _ = _handle(mat, v0, path, dtype)
        _update(A, v1, dtype)
        B, _ = _handle(mat, v1, path, dtype)
        what = f"{name} {mat.name} {_dt(dtype)}"
        for k in (1, 3, 8):
            assert _same(_spmm_run(A, mat, X, k, dtype, k, k), _spmm_run(B, mat, X, k, dtype, k, k)), (what, k)
        xd = _dev(X[:, 0], dtype)
        ys = []
        for Hn in (A, B):
            yd = torch.full((mat.m,), Y0, dtype=_tdt(dtype), device=DEV)
            assert Hn.setX(xd) == 0 and Hn.spmv_repeat(1.0, yd, 3) == 0
            torch.cuda.synchronize()
            ys.append(yd.cpu().numpy())
        assert _same(ys[0], ys[1]), what
        # the checkpoint holds the tile-ordered values: the two files are the same bytes, and loaded handles multiply alike
        fa, fb = str(tmp_path / "a.csr5"), str(tmp_path / "b.csr5")
        assert A.save(fa) == 0 and B.save(fb) == 0
        with open(fa, "rb") as f, open(fb, "rb") as g:
            assert f.read() == g.read(), what
        LA, LB = H.anonymouslibHandle.load(fa), H.anonymouslibHandle.load(fb)
        ya = _spmv(LA, mat, X[:, 0], dtype)
        assert _same(ya, _spmv(LB, mat, X[:, 0], dtype)), what
        R.check(ya, R.reference("row_scaled", mat, v1, X[:, 0]), R.empty_zero_rows(mat.m, LA.info().tail_partition_start), Y0,
                what + " loaded")
        LA.close(), LB.close()
        os.remove(fa), os.remove(fb)
        _close(B)
        _close(A)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_dt)
def test_update_does_not_disturb_the_x_snapshot(dtype):
    """CSR5HIP_OPT_X_SNAPSHOT = 1: the copy of x taken at setX serves the SpMV after an update (no setX in between)"""
    path = BY_NAME["slabs8-hot-snapshot"]
    for mi in _some():
        mat = _matrices()[mi]
        _, v0, _, _ = _case(mi, "wide_range", dtype)
        _, v1, X1, refs = _case(mi, "row_scaled", dtype)
        A, info = _handle(mat, v0, path, dtype)
        _spmv(A, mat, X1[:, 0], dtype)  # setX: the snapshot is taken here
        _update(A, v1, dtype)
        yd = torch.full((mat.m,), Y0, dtype=_tdt(dtype), device=DEV)
        assert A.spmv(1.0, yd) == 0
        torch.cuda.synchronize()
        B, _ = _handle(mat, v1, path, dtype)
        assert _same(yd.cpu().numpy(), _spmv(B, mat, X1[:, 0], dtype)), mat.name
        R.check(yd.cpu().numpy(), refs[0], R.empty_zero_rows(mat.m, info.tail_partition_start), Y0, f"snapshot {mat.name}")
        _close(B)
        _close(A)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_dt)
@pytest.mark.parametrize("name", ["fused-default", "slabs8-hot"])
def test_update_and_spmv_replay_from_one_captured_graph(name, dtype):
    """On a side stream: one warm-up call (it may build the pattern-only helper), then updateValues(buf) + spmv captured once;
    buf, x and y are rewritten between replays."""
    path = BY_NAME[name]
    side = torch.cuda.Stream()
    for mi in _some():
        mat = _matrices()[mi]
        _, v0, X0, _ = _case(mi, "wide_range", dtype)
        A, info = _handle(mat, v0, path, dtype)
        torch.cuda.synchronize()
        buf = _dev(v0, dtype)
        xd = _dev(X0[:, 0], dtype)
        yd = torch.full((mat.m,), Y0, dtype=_tdt(dtype), device=DEV)
        assert A.setStream(side) == 0 and A.setX(xd) == 0
        assert A.updateValues(buf) == 0 and A.spmv(1.0, yd) == 0
        side.synchronize()
        held = A.info().device_bytes
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            assert A.updateValues(buf) == 0, _capi.last_error()
            assert A.spmv(1.0, yd) == 0, _capi.last_error()
        assert A.info().device_bytes == held
        for dataset in ("row_scaled", "subnormal", "wide_range"):
            _, v, X, refs = _case(mi, dataset, dtype)
            buf.copy_(_dev(v, dtype))
            xd.copy_(_dev(X[:, 0], dtype))
            yd.fill_(Y0)
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            y = yd.cpu().numpy()
            B, _ = _handle(mat, v, path, dtype)
            assert _same(y, _spmv(B, mat, X[:, 0], dtype)), (name, mat.name, dataset)
            R.check(y, refs[0], R.empty_zero_rows(mat.m, info.tail_partition_start), Y0, f"graph {name} {mat.name} {dataset}")
            _close(B)
        del graph
        assert A.setStream(None) == 0
        _close(A)


def _multi(mat, val, dtype, slabs):
    rp = torch.from_numpy(mat.row_ptr.astype(np.int32)).to(DEV)
    ci = torch.from_numpy(mat.col.astype(np.int32)).to(DEV)
    A = H.MultiGpuHandle(_devices(3), mat.m, mat.n, dtype=np.dtype(dtype).name)
    assert A.inputCSR(mat.nnz, rp, ci, _dev(val, dtype)) == 0 and A.setSigma(16) == 0
    if slabs:
        assert A.setOption(_capi.OPT_COLUMN_SLABS, slabs) == 0
    assert A.asCSR5() == 0, _capi.last_error()
    return A


def _multi_spmv(A, x, dtype):
    assert A.setX(_dev(x, dtype)) == 0 and A.fill_y(0x7F) == 0
    assert A.spmv(1.0) == 0 and A.synchronize() == 0
    return A.gather_y()


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_dt)
@pytest.mark.parametrize("slabs", [0, 8])
def test_multi_handle_update_values(slabs, dtype):
    """three shards (on one GPU where there is only one: the peer-copy branch needs a second device)"""
    for mi in _some():
        mat = _matrices()[mi]
        _, v0, X0, _ = _case(mi, "wide_range", dtype)
        _, v1, X1, refs = _case(mi, "row_scaled", dtype)
        A = _multi(mat, v0, dtype, slabs)
        _multi_spmv(A, X0[:, 0], dtype)
        vd = _dev(v1, dtype)
        torch.cuda.synchronize()
        assert A.updateValues(vd) == 0, _capi.last_error()
        y = _multi_spmv(A, X1[:, 0], dtype)
        B = _multi(mat, v1, dtype, slabs)
        assert _same(y, _multi_spmv(B, X1[:, 0], dtype)), (mat.name, slabs)
        zr = np.zeros(mat.m, dtype=bool)
        for g in range(3):
            s = A.shard(g)
            zr[s.row_lo + A.shard_info(g).tail_partition_start:s.row_hi] = True
        y0 = np.frombuffer(bytes([0x7F]) * np.dtype(dtype).itemsize, dtype=dtype)[0]
        R.check(y, refs[0], zr, y0, f"multi {mat.name} slabs {slabs}")
        assert _same(vd.cpu().numpy(), v1.astype(dtype))
        for handle in (A, B):
            assert handle.destroy() == 0
            handle.close()
    fresh = H.MultiGpuHandle(_devices(3), 4, 4)
    assert fresh.updateValues(4096) == _capi.UNKOWN_FORMAT  # before inputCSR (the made-up address is never dereferenced)
    fresh.close()


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_dt)
def test_csr_format_copies_and_an_aliased_pointer_is_refused(dtype):
    mi = _some()[2]
    mat = _matrices()[mi]
    _, v0, X0, _ = _case(mi, "wide_range", dtype)
    _, v1, _, _ = _case(mi, "row_scaled", dtype)
    rp = torch.from_numpy(mat.row_ptr.astype(np.int32)).to(DEV)
    ci = torch.from_numpy(mat.col.astype(np.int32)).to(DEV)
    va = _dev(v0, dtype)
    A = H.anonymouslibHandle(mat.m, mat.n, dtype=np.dtype(dtype).name)
    assert A.inputCSR(mat.nnz, rp, ci, va) == 0
    vd = _update(A, v1, dtype)  # CSR format: a copy into the borrowed array
    torch.cuda.synchronize()
    assert _same(va.cpu().numpy(), v1.astype(dtype)) and _same(vd.cpu().numpy(), v1.astype(dtype))
    assert A.setSigma(16) == 0 and A.asCSR5() == 0
    y = _spmv(A, mat, X0[:, 0], dtype)
    B, _ = _handle(mat, v1, Path("plain", 16), dtype)
    assert _same(y, _spmv(B, mat, X0[:, 0], dtype))
    _close(B)
    with pytest.raises(ValueError, match="aliased"):
        A.updateValues(va)
    for ptr in (va.data_ptr(), va.data_ptr() + 5 * va.element_size()):  # past the Python check: the library refuses too
        assert A.updateValues_ptr(ptr) == _capi.INVALID_ARGUMENT
    assert _same(_spmv(A, mat, X0[:, 0], dtype), y)
    _close(A)
