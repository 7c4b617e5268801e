"""autograd.spmm on the GPU: gradcheck, exact agreement with a dense torch matrix on integer data, values replaced between a
forward and its backward, the companion built only when X needs a gradient, and a non-default stream."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from benchmark_spmv_using_csr5_amd import autograd  # noqa: E402
from benchmark_spmv_using_csr5_amd import handle as H  # noqa: E402
from tests import sddmm_reference as S  # noqa: E402
from tests import zoo  # noqa: E402
from tests.test_gpu_exact_reference import DEV, Path, _close, _handle  # noqa: E402

AUTO = H.ANONYMOUSLIB_AUTO_TUNED_SIGMA


def _tdt(dtype):
    return torch.float64 if dtype == np.float64 else torch.float32


def _ints(rng, shape, dtype, lo=-3, hi=4):
    return torch.from_numpy(rng.integers(lo, hi, size=shape).astype(dtype)).to(DEV)


def _dense(mat, val, X):
    """Y = D X with D assembled from the pattern by index_put_(accumulate=True): repeated pairs add up"""
    rows = torch.from_numpy(S.rows_of(mat)).to(DEV)
    cols = torch.from_numpy(mat.col[:mat.nnz].astype(np.int64)).to(DEV)
    D = torch.zeros((mat.m, mat.n), dtype=val.dtype, device=DEV).index_put_((rows, cols), val, accumulate=True)
    return D @ X


def _open(mat, dtype, sigma=AUTO):
    return _handle(mat, np.ones(mat.nnz, dtype=dtype), Path("autograd", sigma, H.SPMV_FUSED), dtype)[0]


def test_gradcheck():
    """fp64, torch's default tolerances.  The function is linear in val and in X, so finite differences carry only rounding.
    gradcheck perturbs its inputs through ``.data``, which does not move ``_version``: the clone hands every evaluation a tensor
    of its own, as the module's docstring asks for such writes."""
    mat = S.duplicates_matrix()
    A = _open(mat, np.float64, sigma=4)
    assert A.info().p >= 2 and (np.diff(mat.row_ptr) == 0).any()
    rng = np.random.default_rng(3)
    val = torch.from_numpy(rng.uniform(-1, 1, size=mat.nnz)).to(DEV).requires_grad_(True)
    X = torch.from_numpy(rng.uniform(-1, 1, size=(mat.n, 3))).to(DEV).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda v, x: autograd.spmm(A, v.clone(), x), (val, X))
    _close(A)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=("fp64", "fp32"))
def test_matches_a_dense_matrix_exactly_on_integer_data(dtype):
    rng = np.random.default_rng(17)
    for mat in list(zoo.small_zoo()) + [S.duplicates_matrix()]:
        for k in (1, 5):
            val = _ints(rng, mat.nnz, dtype, 0, 5).requires_grad_(True)
            X = _ints(rng, (mat.n, k), dtype).requires_grad_(True)
            dY = _ints(rng, (mat.m, k), dtype)
            vr, Xr = val.detach().clone().requires_grad_(True), X.detach().clone().requires_grad_(True)
            Yr = _dense(mat, vr, Xr)
            Yr.backward(dY)
            A = _open(mat, dtype)
            Y = autograd.spmm(A, val, X)
            Y.backward(dY)
            torch.cuda.synchronize()
            assert A.info().transpose_built == 1
            assert torch.equal(Y.detach(), Yr.detach()), (mat.name, k)
            assert torch.equal(val.grad, vr.grad), (mat.name, k)
            assert torch.equal(X.grad, Xr.grad), (mat.name, k)
            # non-contiguous dY, a second step on the same handle with the values changed in place (an optimiser step)
            with torch.no_grad():
                val += 1
            val.grad, X.grad = None, None
            wide = _ints(rng, (mat.m, 2 * k), dtype)
            autograd.spmm(A, val, X).backward(wide[:, ::2])
            vr2 = val.detach().clone().requires_grad_(True)
            Xr2 = X.detach().clone().requires_grad_(True)
            _dense(mat, vr2, Xr2).backward(wide[:, ::2])
            torch.cuda.synchronize()
            assert torch.equal(val.grad, vr2.grad) and torch.equal(X.grad, Xr2.grad), (mat.name, k)
            _close(A)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=("fp64", "fp32"))
def test_backward_after_another_forward_with_other_values(dtype):
    rng = np.random.default_rng(5)
    for mat in [m for m in zoo.small_zoo() if m.name in ("half-empty", "hub", "nonsquare")] + [S.duplicates_matrix()]:
        A = _open(mat, dtype)
        v1 = _ints(rng, mat.nnz, dtype, 0, 5).requires_grad_(True)
        v2 = _ints(rng, mat.nnz, dtype, 5, 9).requires_grad_(True)
        X1 = _ints(rng, (mat.n, 4), dtype).requires_grad_(True)
        X2 = _ints(rng, (mat.n, 4), dtype).requires_grad_(True)
        dY = _ints(rng, (mat.m, 4), dtype)
        Y1 = autograd.spmm(A, v1, X1)
        Y2 = autograd.spmm(A, v2, X2)  # the handle (and, once built, A^T) now holds v2
        Y2.backward(dY)                # builds the companion from v2
        Y1.backward(dY)
        torch.cuda.synchronize()
        for v, X, Y in ((v1, X1, Y1), (v2, X2, Y2)):
            vr, Xr = v.detach().clone().requires_grad_(True), X.detach().clone().requires_grad_(True)
            Yr = _dense(mat, vr, Xr)
            Yr.backward(dY)
            assert torch.equal(Y.detach(), Yr.detach()), mat.name
            assert torch.equal(v.grad, vr.grad) and torch.equal(X.grad, Xr.grad), mat.name
        _close(A)


def test_companion_is_built_only_for_a_gradient_of_x():
    mat = S.duplicates_matrix()
    rng = np.random.default_rng(6)
    A = _open(mat, np.float64)
    val = _ints(rng, mat.nnz, np.float64).requires_grad_(True)
    X = _ints(rng, (mat.n, 3), np.float64)
    dY = _ints(rng, (mat.m, 3), np.float64)
    autograd.spmm(A, val, X).backward(dY)
    torch.cuda.synchronize()
    assert A.info().transpose_built == 0
    vr = val.detach().clone().requires_grad_(True)
    _dense(mat, vr, X).backward(dY)
    assert torch.equal(val.grad, vr.grad)
    X.requires_grad_(True)
    autograd.spmm(A, val, X).backward(dY)
    assert A.info().transpose_built == 1
    _close(A)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=("fp64", "fp32"))
def test_forward_on_a_side_stream_gives_the_same_bits(dtype):
    mat = [m for m in zoo.small_zoo() if m.name == "half-empty"][0]
    rng = np.random.default_rng(7)
    A = _open(mat, dtype)
    val = torch.from_numpy(rng.uniform(-1, 1, size=mat.nnz).astype(dtype)).to(DEV)
    X = torch.from_numpy(rng.uniform(-1, 1, size=(mat.n, 5)).astype(dtype)).to(DEV)
    Y0 = autograd.spmm(A, val, X)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        Y1 = autograd.spmm(A, val.clone(), X)
    side.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(Y0, Y1)
    Y2 = autograd.spmm(A, val, X)  # and back on the default stream
    torch.cuda.synchronize()
    assert torch.equal(Y0, Y2)
    _close(A)
