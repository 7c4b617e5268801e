"""Every SpMV / SpMM kernel family against the exact reference of tests/exact_reference.py.

Data: row_scaled (rows 2**+-900 apart in one tile), nonfinite (Inf / NaN in x and A, x[0] included), subnormal, and
wide_range (checked with a summation-order-free bound that has no absolute floor), in fp64 and fp32.  Matrices: the zoo, a
matrix whose rows span more than 64 tiles (the k_calibrate long-run path of the fused kernel) and a hub-column matrix (the
LDS hot table of the column-slab kernel holds most gathers).

Every path entry forces its option(s) and asserts through info() that the variant ran, except where p < 2 leaves nothing
to choose.  Options that are not forced here, and why: CSR5HIP_OPT_XCD_REMAP (2) and CSR5HIP_OPT_SLAB_SHIFT (7) only
change which workgroup or slab handles which tile or column, not a kernel; CSR5HIP_OPT_SLAB_MEMORY_MIB (10) only decides
whether the slab structure is built (the plain kernel runs otherwise, covered here).
"""
import functools
from dataclasses import dataclass, field

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from benchmark_spmv_using_csr5_amd import _capi  # noqa: E402
from benchmark_spmv_using_csr5_amd import handle as H  # noqa: E402
from tests import exact_reference as R  # noqa: E402
from tests import zoo  # noqa: E402
from tests.test_gpu_multi import _devices  # noqa: E402
from tests.test_gpu_slabs import _hub_columns_matrix  # noqa: E402
from tests.test_gpu_spmm import _long_row_matrix  # noqa: E402

DEV = "cuda:0"
Y0 = 777.0
AUTO = H.ANONYMOUSLIB_AUTO_TUNED_SIGMA
KS = (1, 2, 3, 4, 5, 8, 13)


def _dt(dtype):
    return "fp64" if dtype == np.float64 else "fp32"


def _tdt(dtype):
    return torch.float64 if dtype == np.float64 else torch.float32


@functools.lru_cache(maxsize=1)
def _matrices():
    # n <= 32 768 everywhere, so that the x-window kernel's 16-bit column codes apply to every matrix with p >= 2
    return tuple(zoo.small_zoo()) + (_long_row_matrix(), _hub_columns_matrix(3000, 30000, 12, 300, 1))


@functools.lru_cache(maxsize=None)
def _case(mi, dataset, dtype, k=1, finite_matrix=False):
    """(matrix, values, X, [reference of every column of X]): computed once, shared by every path"""
    mat = _matrices()[mi]
    val, X = R.make(dataset, mat, dtype, seed=11 + mi, k=k, finite_matrix=finite_matrix)
    return mat, val, X, [R.reference(dataset, mat, val, X[:, c]) for c in range(k)]


@dataclass(frozen=True)
class Path:
    name: str
    sigma: int
    mode: int = H.SPMV_FUSED
    opts: tuple = ()                                # (setter, value) before asCSR5
    expect: dict = field(default_factory=dict)      # info() field -> value (asserted where p >= 2)
    zero_empty: bool = False


def _p(name, sigma, mode=H.SPMV_FUSED, zero_empty=False, expect=None, **opts):
    if zero_empty:
        opts["setZeroEmptyRows"] = 1
    return Path(name, sigma, mode, tuple(opts.items()), dict(expect or {}), zero_empty)


PLAIN = dict(column_slabs=0)
PATHS = [
    *[_p(f"two-pass-s{s}", s, H.SPMV_TWO_PASS, expect=dict(PLAIN, x_window_active=0, carries_deferred=0, flagged_columns=0))
      for s in (4, 7, 16, 32)],
    _p("fused-default", AUTO, expect=PLAIN),
    _p("xwin-narrow", 16, setXWindow=2, setNarrowColumns=1, expect=dict(PLAIN, x_window_active=1, narrow_columns=1)),
    _p("xwin-wide", 16, setXWindow=2, setNarrowColumns=0, expect=dict(PLAIN, x_window_active=1, narrow_columns=0)),
    _p("xwin-narrow-s32", 32, setXWindow=2, setNarrowColumns=1, expect=dict(PLAIN, x_window_active=1, narrow_columns=1)),
    _p("xwin-ldsy", 8, setXWindow=2, setLdsY=2, expect=dict(PLAIN, x_window_active=1, lds_y=1)),
    _p("ldsy", 8, setXWindow=0, setLdsY=2, expect=dict(PLAIN, x_window_active=0, lds_y=1)),
    _p("ldsy-two-pass", 16, H.SPMV_TWO_PASS, setLdsY=2, expect=dict(PLAIN, lds_y=1)),
    _p("nt", 8, setXWindow=0, setStreamNT=2, setFlaggedColumns=0, expect=dict(PLAIN, stream_nt=1, flagged_columns=0)),
    _p("nt-flagged", 6, setXWindow=0, setStreamNT=2, setFlaggedColumns=2, expect=dict(PLAIN, stream_nt=1, flagged_columns=1)),
    *[_p(f"flagged-s{s}", s, setXWindow=0, setFlaggedColumns=2, expect=dict(PLAIN, flagged_columns=1)) for s in (4, 5, 6, 7, 8)],
    _p("deferred-s7", 7, setXWindow=0, setDeferCarries=2, expect=dict(PLAIN, carries_deferred=1)),
    _p("deferred-s16-ldsy", 16, setXWindow=0, setDeferCarries=2, setLdsY=2, expect=dict(PLAIN, carries_deferred=1, lds_y=1)),
    _p("slabs8", 16, setColumnSlabs=8, setSlabHot=0, expect=dict(column_slabs=8, slab_hot=0)),
    _p("slabs8-hot", 16, setColumnSlabs=8, setSlabHot=2, expect=dict(column_slabs=8, slab_hot=1, x_snapshot=0)),
    _p("slabs8-hot-snapshot", 16, setColumnSlabs=8, setSlabHot=2, setXSnapshot=1,
       expect=dict(column_slabs=8, slab_hot=1, x_snapshot=1, slab_x_permuted=1)),
    _p("zero-empty", AUTO, zero_empty=True, expect=PLAIN),
    _p("zero-empty-two-pass", 7, H.SPMV_TWO_PASS, zero_empty=True, expect=PLAIN),
    _p("zero-empty-slabs8-hot", 16, zero_empty=True, setColumnSlabs=8, setSlabHot=2, expect=dict(column_slabs=8, slab_hot=1)),
]


def _handle(mat, val, path, dtype):
    """a converted handle on device copies of the CSR arrays (kept alive on the handle object)"""
    rp = torch.from_numpy(mat.row_ptr.astype(np.int32)).to(DEV)
    ci = torch.from_numpy(mat.col.astype(np.int32)).to(DEV)
    va = torch.from_numpy(val.astype(dtype)).to(DEV)
    A = H.anonymouslibHandle(mat.m, mat.n, dtype=np.dtype(dtype).name)
    A._arrays = (rp, ci, va)
    assert A.inputCSR(mat.nnz, rp, ci, va) == 0
    assert A.setSigma(path.sigma) == 0
    assert A.setSpmvMode(path.mode) == 0
    for setter, value in path.opts:
        assert getattr(A, setter)(value) == 0, (setter, _capi.last_error())
    assert A.asCSR5() == 0, _capi.last_error()
    info = A.info()
    if path.sigma != AUTO:
        assert info.sigma == path.sigma
    if info.p >= 2:
        got = {f: getattr(info, f) for f in path.expect}
        assert got == path.expect, (path.name, mat.name, got)
    return A, info


def _spmv(A, mat, x, dtype):
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    yd = torch.full((mat.m,), Y0, dtype=_tdt(dtype), device=DEV)
    assert A.setX(xd) == 0 and A.spmv(1.0, yd) == 0
    torch.cuda.synchronize()
    return yd.cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _close(A):
    assert A.destroy() == 0
    A.close()


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_dt)
@pytest.mark.parametrize("path", PATHS, ids=lambda p: p.name)
def test_spmv_path_exact(path, dtype):
    for mi, mat in enumerate(_matrices()):
        for dataset in R.DATASETS:
            _, val, X, refs = _case(mi, dataset, dtype)
            A, info = _handle(mat, val, path, dtype)
            y = _spmv(A, mat, X[:, 0], dtype)
            R.check(y, refs[0], R.empty_zero_rows(mat.m, info.tail_partition_start, path.zero_empty), Y0,
                    f"{path.name} {mat.name} {dataset} {_dt(dtype)} sigma {info.sigma}")
            _close(A)


def test_narrow_values_exact_and_only_where_lossless():
    """CSR5HIP_OPT_NARROW_VALUES: narrowed (and bit-identical to the fp64 stream) on fp32-exact data including values of
    exactly 2**-126 and 2**127; not narrowed, and exact, on row_scaled, subnormal and data holding 2**128."""
    mi = len(_matrices()) - 1
    mat = _matrices()[mi]
    path = _p("narrow", 16, setColumnSlabs=8, setSlabHot=2, expect=dict(column_slabs=8, slab_hot=1))
    narrow = Path("narrow", 16, H.SPMV_FUSED, path.opts + (("setNarrowValues", 1),), path.expect)
    rng = np.random.default_rng(5)
    base = rng.integers(0, 10, size=mat.nnz).astype(np.float64)
    x_int = rng.integers(0, 10, size=mat.n).astype(np.float64)
    edge = rng.choice(mat.nnz, size=40, replace=False)
    fits = base.copy()
    fits[edge[:20]] = 2.0 ** -126
    fits[edge[20:]] = 2.0 ** 127
    over = base.copy()
    over[edge[:3]] = 2.0 ** 128
    cases = [("fits", fits, x_int, "wide_range", 1), ("2**128", over, x_int, "wide_range", 0)]
    for dataset in ("row_scaled", "subnormal"):
        _, val, X, _ = _case(mi, dataset, np.float64)
        cases.append((dataset, val, X[:, 0], dataset, 0))
    for name, val, x, kind, narrowed in cases:
        ref = R.reference(kind, mat, val, x)
        ys = []
        for p in (narrow, path):
            A, info = _handle(mat, val, p, np.float64)
            want = narrowed if p is narrow else 0
            assert info.slab_values_narrowed == want, (name, p.name)
            y = _spmv(A, mat, x, np.float64)
            R.check(y, ref, R.empty_zero_rows(mat.m, info.tail_partition_start), Y0, f"narrow values {name}")
            ys.append(y)
            _close(A)
        assert np.array_equal(_bits(ys[0]), _bits(ys[1])), name


def _spmm_run(A, mat, X, k, dtype, ldx, ldy, x_offset=0):
    """Y = A X with X at leading dimension ldx (padding columns NaN) `x_offset` elements into its allocation, Y at ldy
    (everything poisoned); returns the whole (m, ldy) Y"""
    tdt = _tdt(dtype)
    Xb = torch.full((x_offset + mat.n * ldx,), float("nan"), dtype=tdt, device=DEV)
    Xv = Xb[x_offset:].view(mat.n, ldx)
    Xv[:, :k] = torch.from_numpy(np.ascontiguousarray(X[:, :k])).to(DEV)
    Yb = torch.full((mat.m, ldy), Y0, dtype=tdt, device=DEV)
    assert A.spmm_ptr(Xv, ldx, k, Yb, ldy) == 0
    torch.cuda.synchronize()
    return Yb.cpu().numpy()


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_dt)
@pytest.mark.parametrize("dataset", R.DATASETS)
def test_spmm_exact(dataset, dtype):
    """k = 1, 2, 3, 4, 5, 8, 13 on three layouts: contiguous (whole-block vector loads where the block is full), ldx = k + 1
    with NaN padding and ldy = k + 2 (element loads where ldx breaks the vector width), and X one element off its
    allocation's alignment.  In nonfinite only X's column 0 holds Inf / NaN: the other columns must come out exact.  Y's
    padding columns keep their poison."""
    kmax = max(KS)
    for mi, mat in enumerate(_matrices()):
        _, val, X, refs = _case(mi, dataset, dtype, k=kmax, finite_matrix=True)
        for sigma in (7, 16):  # fp32 sigma 7: the run-time-sigma SpMM kernel
            A, info = _handle(mat, val, Path("spmm", sigma, H.SPMV_FUSED), dtype)
            zr = R.empty_zero_rows(mat.m, info.tail_partition_start)
            for k in KS:
                for ldx, ldy, off in ((k, k, 0), (k + 1, k + 2, 0), (k, k, 1)):
                    Y = _spmm_run(A, mat, X, k, dtype, ldx, ldy, off)
                    for c in range(k):
                        R.check(Y[:, c], refs[c], zr, Y0, f"spmm {mat.name} {dataset} sigma {sigma} k {k} ldx {ldx} "
                                                         f"off {off} column {c}")
                    assert (_bits(Y[:, k:]) == _bits(np.full(1, Y0, dtype=dtype))[0]).all(), (mat.name, k, ldy)
            _close(A)


# ---- state of one spmv() surviving into the next ------------------------------------------------------------------------

STALE_PATHS = [p for p in PATHS if p.name in ("two-pass-s7", "fused-default", "xwin-narrow", "ldsy", "nt-flagged",
                                              "deferred-s7", "slabs8", "slabs8-hot", "slabs8-hot-snapshot")]


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_dt)
def test_no_state_survives_between_spmv_calls(dtype):
    """One handle per path family: spmv with the nonfinite x, then x overwritten IN PLACE with finite data + setX + spmv must
    be exact for the finite x; then back to the non-finite x."""
    picks = [i for i, m in enumerate(_matrices()) if m.name in ("hub", "scircuit-like(synthetic)", "aligned1024")]
    picks += [len(_matrices()) - 2, len(_matrices()) - 1]
    for mi in picks:
        mat, val, X, refs = _case(mi, "nonfinite", dtype, k=2, finite_matrix=True)
        assert not np.isfinite(X[:, 0]).all() and np.isfinite(X[:, 1]).all()
        for path in STALE_PATHS:
            A, info = _handle(mat, val, path, dtype)
            zr = R.empty_zero_rows(mat.m, info.tail_partition_start)
            xd = torch.from_numpy(np.ascontiguousarray(X[:, 0])).to(DEV)
            yd = torch.empty(mat.m, dtype=_tdt(dtype), device=DEV)
            assert A.setX(xd) == 0
            for c in (0, 1, 0):
                xd.copy_(torch.from_numpy(np.ascontiguousarray(X[:, c])).to(DEV))
                yd.fill_(Y0)
                assert A.setX(xd) == 0 and A.spmv(1.0, yd) == 0
                torch.cuda.synchronize()
                R.check(yd.cpu().numpy(), refs[c], zr, Y0, f"{path.name} {mat.name} after column {c}")
            _close(A)


def test_multi_gpu_exact():
    """MultiGpuHandle, G = 2 (two devices where visible, else two shards on one): row_scaled and nonfinite through
    gather_y.  Empty rows below a shard's own tail keep the fill pattern."""
    G = 2
    for dtype in R.DTYPES:
        y0 = np.frombuffer(bytes([0x7F]) * np.dtype(dtype).itemsize, dtype=dtype)[0]
        for mi, mat in enumerate(_matrices()):
            for dataset in ("row_scaled", "nonfinite"):
                _, val, X, refs = _case(mi, dataset, dtype)
                rp = torch.from_numpy(mat.row_ptr.astype(np.int32)).to(DEV)
                ci = torch.from_numpy(mat.col.astype(np.int32)).to(DEV)
                va = torch.from_numpy(val).to(DEV)
                xd = torch.from_numpy(np.ascontiguousarray(X[:, 0])).to(DEV)
                A = H.MultiGpuHandle(_devices(G), mat.m, mat.n, dtype=np.dtype(dtype).name)
                assert A.inputCSR(mat.nnz, rp, ci, va) == 0 and A.setSigma(AUTO) == 0 and A.asCSR5() == 0
                assert A.setX(xd) == 0 and A.fill_y(0x7F) == 0
                assert A.spmv(1.0) == 0 and A.synchronize() == 0
                y = A.gather_y()
                zr = np.zeros(mat.m, dtype=bool)
                for g in range(G):
                    s = A.shard(g)
                    zr[s.row_lo + A.shard_info(g).tail_partition_start:s.row_hi] = True
                R.check(y, refs[0], zr, y0, f"multi {mat.name} {dataset} {_dt(dtype)}")
                assert A.destroy() == 0
                A.close()
