"""tests/handle_history.py on the host (no GPU): the comparator rejects every single-element difference it is there to find, the
second matrix of the ``second-matrix`` history is what that history needs, the values keep the products of the battery exact,
every history of the registry names a twin that ``test_gpu_exact_reference._handle`` can build, and ``updateValues`` sees no alias
between tensors without elements (the one defect the histories met)."""
import numpy as np
import pytest

from benchmark_spmv_using_csr5_amd import handle as H
from tests import attention_edges as E
from tests import handle_history as HH
from tests import zoo

DTYPES = (np.float64, np.float32)


def _results(dtype):
    rng = np.random.default_rng(3)
    a = rng.uniform(-1, 1, size=(7, 3)).astype(dtype)
    a[2, 1] = 0.0
    b = rng.uniform(-1, 1, size=11).astype(dtype)
    b[4] = np.nan  # (a NaN that is expected: the twin has it)
    return {"first": a, "second": b, "words": rng.integers(0, 2 ** 16, size=(5, 2)).astype(np.uint16)}


def _copy(res):
    return {k: v.copy() for k, v in res.items()}


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp64", "fp32"))
def test_the_comparator_rejects_one_wrong_element_of_one_output(dtype):
    want = _results(dtype)
    assert HH.same(_copy(want), want) is None
    got = _copy(want)
    got["second"][4] = -np.nan  # any NaN will do where a NaN is expected
    assert HH.same(got, want) is None
    got = _copy(want)
    got["first"][5, 2] = np.nextafter(got["first"][5, 2], dtype(9))  # one unit in the last place
    assert HH.same(got, want) == ("first", (5, 2))
    got = _copy(want)
    got["first"][2, 1] = -0.0  # the sign of zero
    assert got["first"][2, 1] == want["first"][2, 1] and HH.same(got, want) == ("first", (2, 1))
    got = _copy(want)
    del got["second"]  # a missing key, on either side
    assert HH.same(got, want) == ("second", None) and HH.same(want, got) == ("second", None)
    got = _copy(want)
    other = np.float32 if dtype == np.float64 else np.float64
    got["first"] = np.zeros((7, 3), dtype=other)
    ref = dict(want, first=np.zeros((7, 3), dtype=dtype))
    assert np.array_equal(got["first"], ref["first"]) and HH.same(got, ref) == ("first", None)  # equal values, another dtype
    got = _copy(want)
    got["first"] = got["first"].reshape(3, 7)
    assert HH.same(got, want) == ("first", None)
    got = _copy(want)
    got["second"][7] = np.nan  # a NaN where a number is expected
    assert HH.same(got, want) == ("second", (7,))
    got = _copy(want)
    got["second"][4] = 1.0  # a number where a NaN is expected
    assert HH.same(got, want) == ("second", (4,))
    got = _copy(want)
    got["words"][3, 1] ^= 1
    assert HH.same(got, want) == ("words", (3, 1))
    got = _copy(want)
    got["first"][0, 0] += dtype(1)
    got["second"][0] += dtype(1)
    assert HH.same(got, want) == ("first", (0, 0))  # the first one, in the twin's order


def test_the_second_matrix_has_the_shape_fewer_entries_another_profile_and_every_class():
    P = E.class_edges()
    Q = HH.second_pattern(P)
    assert (Q.m, Q.n) == (P.m, P.n) and 0 < Q.nnz < P.nnz and Q.row_ptr[-1] == Q.nnz == Q.col.size
    pl, ql = np.diff(P.row_ptr), np.diff(Q.row_ptr)
    assert (ql[::3] == 0).all() and not np.array_equal(np.sort(pl), np.sort(ql)) and not np.array_equal(pl, ql)
    assert ((ql > 0) & (ql <= E.AT_G)).any() and ((ql > E.AT_G) & (ql <= E.AT_WAVE_ROW)).any()
    assert ((ql > E.AT_WAVE_ROW) & (ql <= E.AT_STAGE)).any() and (ql > E.AT_STAGE).any()
    # a kept row holds the columns of the row of P it mirrors, in their order
    for i in (1, 68, 257, P.m - 2):
        s = P.m - 1 - i
        assert np.array_equal(Q.col[Q.row_ptr[i]:Q.row_ptr[i + 1]], P.col[P.row_ptr[s]:P.row_ptr[s + 1]])
    assert Q.col.min() >= 0 and Q.col.max() < Q.n
    assert -(-Q.nnz // (64 * 32)) >= 2  # p >= 2 at every sigma


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp64", "fp32"))
def test_the_values_are_distinct_and_their_products_exact(dtype):
    for mat in (E.class_edges(), [m for m in zoo.small_zoo() if m.name == "tiny-p1"][0], zoo.empty_matrix()):
        for seed in (1, 2):
            v = HH.values(mat, seed, dtype)
            assert v.dtype == dtype and v.shape == (mat.nnz,) and len(np.unique(v)) == mat.nnz
            assert not mat.nnz or (np.abs(v) < 2).all()
            p = v.astype(np.float64)[:, None] * np.arange(10.0)[None, :]
            assert np.array_equal(p.astype(dtype).astype(np.float64), p)
        assert not np.array_equal(HH.values(mat, 1, dtype), HH.values(mat, 2, dtype)) or mat.nnz < 2
    fine = HH.values(E.class_edges(), 1, np.float64, fine=True)
    assert (fine.astype(np.float32).astype(np.float64) != fine).sum() >= fine.size - 1
    from fractions import Fraction
    assert all(Fraction(float(f)) * 9 == Fraction(float(f) * 9.0) for f in fine[:200])  # still exact with x in fp64


def test_the_operands_are_a_function_of_the_seed_alone():
    mat = [m for m in zoo.small_zoo() if m.name == "tiny-p1"][0]
    a, b = HH.operands(mat, np.float32, 5), HH.operands(mat, np.float32, 6)
    HH._OPERANDS.clear()
    c = HH.operands(mat, np.float32, 5)
    assert set(a) == set(c) and all(np.array_equal(np.asarray(a[k]), np.asarray(c[k]), equal_nan=True) for k in a if not k.startswith("lowp"))
    assert all(np.array_equal(x, y) for k in a if k.startswith("lowp") for x, y in zip(a[k], c[k]))
    assert not np.array_equal(a["Q"], b["Q"])
    e = HH.operands(zoo.empty_matrix(), np.float64, 5)  # the empty matrix has operands too
    assert e["B"].shape == (0, HH.MHA[0]) and e["v2"].shape == (0,) and e["scores"].shape == (0,)


def test_every_history_names_a_twin_that_can_be_built():
    wanted = {"loaded", "loaded-from-slabs-hot", "loaded-from-narrow", "saved-behind-a-side-stream", "reconverted",
              "loaded-then-reconverted", "second-matrix", "second-matrix-under-slabs", "options-toggled", "options-toggled-and-back"}
    assert set(HH.HISTORIES) == wanted
    for name, hist in HH.HISTORIES.items():
        twin = hist.twin()
        path = twin.path()
        assert callable(hist.build) and (path.sigma == HH.AUTO or 1 <= path.sigma <= 32), name
        assert path.mode == H.SPMV_FUSED and path.expect == {}, name
        for setter, value in path.opts:
            assert callable(getattr(H.anonymouslibHandle, setter, None)) and isinstance(value, int), (name, setter)
        assert (hist.file_sigma > 0) == hist.loaded, name
    assert HH.HISTORIES["options-toggled"].opts == HH.TOGGLED and HH.HISTORIES["options-toggled-and-back"].opts == ()
    assert [s for s, _ in HH.TOGGLED] == [s for s, _ in HH.DEFAULTS]
    # what the named paths that three histories start from are today
    assert dict(HH.BY_NAME["slabs8-hot"].opts) == {"setColumnSlabs": 8, "setSlabHot": 2} and HH.BY_NAME["slabs8-hot"].sigma == 16
    assert dict(HH.BY_NAME["xwin-narrow"].opts) == {"setXWindow": 2, "setNarrowColumns": 1} and HH.BY_NAME["xwin-narrow"].sigma == 16


def test_update_values_on_a_matrix_without_entries_finds_no_alias():
    """tensors without elements own no memory: their storages all report the null pointer, which must not read as sharing a
    storage with the tensor given to inputCSR (met by the battery on the empty matrix).  Host tensors: the call then ends at the
    check that FOLLOWS the aliasing one; a tensor with elements that does share the storage is refused as before."""
    torch = pytest.importorskip("torch")
    A = H.anonymouslibHandle(5, 5)
    calls = []
    A.updateValues_ptr = lambda *a: calls.append(a) or 0  # nothing may reach the library
    mine = torch.zeros(0, dtype=torch.float64)
    assert A.inputCSR(0, torch.zeros(6, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), mine) == 0
    new = torch.zeros(0, dtype=torch.float64)
    assert new.untyped_storage().data_ptr() == mine.untyped_storage().data_ptr()  # (what made the old check fire)
    with pytest.raises(ValueError, match="must live on the GPU"):
        A.updateValues(new)
    A.close()
    A = H.anonymouslibHandle(5, 5)
    A.updateValues_ptr = lambda *a: calls.append(a) or 0
    mine = torch.zeros(8, dtype=torch.float64)
    assert A.inputCSR(4, None, None, 1 << 20) == 0  # (a made-up device address: never dereferenced)
    A._keep["val"] = mine
    with pytest.raises(ValueError, match="shares storage"):
        A.updateValues(mine[4:])
    assert not calls
    A.close()
