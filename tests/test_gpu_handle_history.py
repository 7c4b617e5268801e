"""Every pattern operation on handles with a history (tests/handle_history.py): loaded from a checkpoint, reconverted at another
sigma, given a second matrix, options switched after the conversion, saved behind a side stream.  One test per history, matrix and
dtype; what it asserts, in order:

E  (second-matrix) before buildTranspose is called again spmvT is refused with the csr5hip_build_transpose text;
C  a save of the history handle is byte-identical to a save of its twin -- the fresh handle of the same sigma and effective options
   (``Twin``) -- and, where the handle was loaded and not reconverted, to the file it was loaded from;
A  info() agrees with the twin's in every field that is no timing, pointer or byte count, and the battery gives the twin's bits in
   EVERY output, products included;
B  the twin's own numbers are anchored: the products of every twin by tests/exact_reference.py's order-free bound (the values
   keep every product exact, tests/handle_history.py), everything else ONCE per (matrix, dtype, values) by the float64 references
   of the existing modules under their allowances (``_within`` / FIRST_ORDER of tests/test_gpu_attention_autograd.py,
   tests/edge_bias_reference.py, tests/test_gpu_mha_bias.py's ``_reference`` / ``_bias_allowances``, tests/lowp_reference.py,
   tests/sddmm_reference.py, tests/softmax_reference.py) -- no tolerance is introduced here; a later twin of the same matrix, dtype
   and values (another sigma, other options) must then have the anchored twin's bits in every output whose bits depend on
   neither, and gets its own comparison where they do (the products, and autograd.attention, which multiplies through spmm);
D  on both handles: the companion is built, and one more mhaEdgeBiasBackward replayed from a captured graph gives the eager bits
   with the device bytes unchanged -- no history leaves a call that allocates or synchronises;
E  (second-matrix) the device bytes held do not exceed those of the first matrix' phase;
C  asCSR() gives back row_ptr, the original column bits and the values given last; close() raises nothing; a loaded handle's
   file loads a second time (and, where the twin has the file's sigma, multiplies to the twin's bits).

The matrices are the smallest at which the paths differ: class_edges() (769 x 4 608: every line class on both sides of its edges,
hubs beyond workgroup 0, empty rows, p >= 2 at every sigma, a CSR tail) carries every history but the three that start from a named
path of tests/test_gpu_exact_reference.py; those, and options-toggled once more, run on its hub-columns matrix, where the hot table
holds most gathers and ``slabs8-hot``'s ``expect`` holds; tiny-p1 (the tail only) and the empty matrix get ``loaded`` and ``reconverted``
(on the empty matrix every call of the battery is legal -- tests/test_gpu_transpose.py::test_empty_matrix and the degenerate-shape
tests of the attention modules -- but the autograd wrappers, which are not defined for tensors without elements, are left out, and
there is no number to anchor: every written output must be +0 and every product Y0)."""
import functools
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from benchmark_spmv_using_csr5_amd import _capi  # noqa: E402
from benchmark_spmv_using_csr5_amd import handle as H  # noqa: E402
from tests import edge_bias_reference as EB  # noqa: E402
from tests import exact_reference as R  # noqa: E402
from tests import handle_history as HH  # noqa: E402
from tests import lowp_reference as L  # noqa: E402
from tests import sddmm_reference as S  # noqa: E402
from tests import softmax_reference as SM  # noqa: E402
from tests import zoo  # noqa: E402
from tests.test_gpu_attention_autograd import FIRST_ORDER, STAGES, _allowances, _index, _reference, _within  # noqa: E402
from tests.test_gpu_exact_reference import DEV, Y0, _close, _matrices  # noqa: E402
from tests.test_gpu_mha_bias import _bias_allowances  # noqa: E402
from tests.test_gpu_mha_bias import _reference as _bias_reference  # noqa: E402

SEED = 4242
POISON = -777.25
MAIN = ("loaded", "saved-behind-a-side-stream", "reconverted", "loaded-then-reconverted", "second-matrix", "options-toggled",
        "options-toggled-and-back")
CASES = ([("class-edges", h) for h in MAIN] +
         [("hub-columns", h) for h in ("loaded-from-slabs-hot", "loaded-from-narrow", "options-toggled", "second-matrix-under-slabs")] +
         [(m, h) for m in ("tiny-p1", "empty") for h in ("loaded", "reconverted")])
# outputs whose bits depend on sigma, path or options: the products, and whatever goes through them
BY_CONVERSION = ("spmv", "spmm", "spmvT", "spmmT", "v2.spmv", "v2.spmvT", "autograd.spmm.Y", "autograd.spmm.dX", "autograd.attention.")


def _dt(dtype):
    return "fp64" if dtype == np.float64 else "fp32"


@functools.lru_cache(maxsize=1)
def _mats():
    hub = _matrices()[-1]
    assert hub.name.startswith("hubcols")
    return {"class-edges": HH.E.class_edges(), "hub-columns": hub, "empty": zoo.empty_matrix(),
            "tiny-p1": [m for m in zoo.small_zoo() if m.name == "tiny-p1"][0]}


def _info(A):
    i = A.info()
    return {n: getattr(i, n) for n, _ in i._fields_ if not (n.endswith("_ms") or n.startswith("d_") or n == "device_bytes")}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- B. the anchors ------------------------------------------------------------------------------------------------------------------
_ANCHORS = {}


@functools.lru_cache(maxsize=None)
def _product_refs(key):
    """the references of every product of the battery for (matrix, dtype, values): name -> [Reference per column]"""
    mat, dtype, val = _KEYED[key]
    o = HH.operands(mat, dtype, SEED)
    refs = {}
    for prefix, v in (("", val), ("v2.", o["v2"])):
        matT, vT = HH.transposed(mat, v)
        refs[prefix + "spmv"] = [R.reference("wide_range", mat, v, o["x"])]
        refs[prefix + "spmvT"] = [R.reference("wide_range", matT, vT, o["xt"])]
        if not prefix:
            refs["spmm"] = [R.reference("wide_range", mat, v, o["X3"][:, c]) for c in range(3)]
            refs["spmmT"] = [R.reference("wide_range", matT, vT, o["Xt3"][:, c]) for c in range(3)]
    matT, vT = HH.transposed(mat, o["v3"])
    refs["autograd.spmm.Y"] = [R.reference("wide_range", mat, o["v3"], o["X3i"][:, c]) for c in range(3)]
    refs["autograd.spmm.dX"] = [R.reference("wide_range", matT, vT, o["dY3"][:, c]) for c in range(3)]
    return refs


_KEYED = {}


def _key(mat, dtype, val):
    key = (mat.name, _dt(dtype), hash(np.ascontiguousarray(val).tobytes()))
    _KEYED[key] = (mat, dtype, val)
    return key


def _check_products(key, res, info, zero_empty, what):
    mat, dtype, _ = _KEYED[key]
    rows = {"m": R.empty_zero_rows(mat.m, info["tail_partition_start"], zero_empty),
            "n": R.empty_zero_rows(mat.n, info["t_tail_partition_start"], zero_empty)}
    every = {"m": np.ones(mat.m, dtype=bool), "n": np.ones(mat.n, dtype=bool)}  # (autograd multiplies into torch.zeros)
    for name, refs in _product_refs(key).items():
        if name not in res:
            continue
        side = "n" if name.endswith(("spmvT", "spmmT", ".dX")) else "m"
        zr, y0 = (every[side], 0.0) if name.startswith("autograd") else (rows[side], Y0)
        y = res[name].reshape(res[name].shape[0], -1)
        for c, ref in enumerate(refs):
            R.check(np.ascontiguousarray(y[:, c]), ref, zr, y0, f"{what} {name} column {c}")


def _anchor_empty(mat, res):
    for name, a in res.items():
        if name in ("spmv", "spmm", "spmvT", "spmmT", "v2.spmv", "v2.spmvT"):
            assert (a == Y0).all(), name  # nothing to write: in front of the tail every row keeps what it held
        else:
            assert not a.view(np.uint8).any(), name  # +0 (16-bit: the word 0) wherever something is written


def _anchor_attention(key, res, what):
    """everything but the products against the float64 references; returns what a later twin of the same key is compared with"""
    mat, dtype, val = _KEYED[key]
    o = HH.operands(mat, dtype, SEED)
    rows, cols = _index(mat)
    u = R.unit_roundoff(dtype)
    rhos = {}
    # the pattern operations: exact (integer operands) / the softmax references' own bounds
    for k in (13, 8):
        S.check(res[f"sddmm{k}"], S.reference("integer", mat, o[f"U{k}"], o[f"V{k}"]), f"{what} sddmm k = {k}")
    S.check(res["autograd.spmm.dval"], S.reference("integer", mat, o["dY3"], o["X3i"]), f"{what} autograd.spmm dval")
    SM.check(res["rowSoftmax"], SM.softmax_reference(mat.row_ptr, o["scores"]), f"{what} rowSoftmax")
    SM.check(res["rowSoftmaxGrad"], SM.grad_reference(mat.row_ptr, o["p"], o["g"]), f"{what} rowSoftmaxGrad")
    # single head, (k, d) = (8, 16): the fused calls and the composed autograd.attention share reference and allowances
    Q, K, V, dO = (_t(o[n]) for n in ("Q1", "K1", "V1", "dO1"))
    want = _reference(mat, rows, cols, Q, K, V, dO)
    allow = _allowances(mat, rows, cols, Q, K, V, dO, dtype)
    rhos["attention"] = allow[0]
    assert STAGES * allow[0] <= FIRST_ORDER, (what, allow[0])
    single = (want, allow[1:])
    for n, w, a in zip(("O", "dQ", "dK", "dV"), want, allow[1:]):
        _within(_t(res["attention." + n]), w, a, f"{what} attention {n}")
    # plain multi-head: head by head on the slices, under the single-head allowances
    Q, K, V, dO, Bt, sl = (_t(o[n]) for n in ("Q", "K", "V", "dO", "B", "slopes"))
    for h in range(HH.MHA[0]):
        sl_h = [t[:, h].contiguous() for t in (Q, K, V, dO)]
        want = _reference(mat, rows, cols, *sl_h)
        allow = _allowances(mat, rows, cols, *sl_h, dtype)
        rhos["mha"] = max(rhos.get("mha", 0.0), allow[0])
        assert STAGES * allow[0] <= FIRST_ORDER, (what, h, allow[0])
        for n, w, a in zip(("O", "dQ", "dK", "dV"), want, allow[1:]):
            _within(_t(res["mha." + n])[:, h], w, a, f"{what} mha head {h} {n}")
    # biased: the held values times the slopes, scale 0.25
    for prefix, held, names in (("mhaBiased", val, ("O", "dQ", "dK", "dV", "dS")), ("v2.mhaBiased", o["v2"], ("O",)),
                                ("autograd.mha", o["bias1d"], ("O", "dQ", "dK", "dV"))):
        vt = _t(np.asarray(held, dtype=dtype))
        want = _bias_reference(mat, rows, cols, HH.SCALE, vt, sl, Q, K, V, dO)
        allow = _bias_allowances(mat, rows, cols, HH.SCALE, vt, sl, Q, K, V, dO, dtype)
        rhos[prefix] = allow[0]
        assert STAGES * allow[0] <= FIRST_ORDER, (what, prefix, allow[0])
        for n, w, a in zip(("O", "dQ", "dK", "dV", "dS"), want, allow[1:]):
            if n in names:
                _within(_t(res[f"{prefix}.{n}"]), w, a, f"{what} {prefix} {n}")
        if prefix == "autograd.mha":  # the two reductions of dS, as tests/test_gpu_mha_bias.py bounds them
            a_S, dSr, sd, ad = allow[5], want[4], sl.double(), vt.double()
            gam = lambda n: n * u / (1 - n * u)  # noqa: E731
            a_bias = (a_S * sd.abs()[None, :]).sum(1) + gam(HH.MHA[0] + 1) * (dSr.abs() * sd.abs()[None, :]).sum(1)
            a_slopes = (a_S * ad.abs()[:, None]).sum(0) + gam(mat.nnz + 1) * (dSr.abs() * ad.abs()[:, None]).sum(0)
            _within(_t(res["autograd.mha.dbias"]), want[5], a_bias, f"{what} autograd.mha dbias")
            _within(_t(res["autograd.mha.dslopes"]), want[6], a_slopes, f"{what} autograd.mha dslopes")
    # edge bias
    want = EB.reference(mat, rows, cols, HH.SCALE, Bt, Q, K, V, dO)
    allow = EB.allowances(mat, rows, cols, HH.SCALE, Bt, Q, K, V, dO, dtype, STAGES)
    rhos["mhaEdgeBias"] = allow[0]
    assert STAGES * allow[0] <= FIRST_ORDER, (what, allow[0])
    for n, w, a in zip(("O", "dQ", "dK", "dV", "dB"), want, allow[1:]):
        _within(_t(res["mhaEdgeBias." + n]), w, a, f"{what} mhaEdgeBias {n}")
    # 16-bit operands: the fp32 allowance of the edge call on the widened operands + one rounding to the operand type
    for kind in L.KINDS:
        wide = [_t(L.widen(w, kind)) for w in o["lowp." + kind]]
        zero = torch.zeros((mat.m, HH.LOWP[0], HH.LOWP[2]), dtype=torch.float32, device=DEV)
        want = EB.reference(mat, rows, cols, HH.SCALE, wide[0], wide[1], wide[2], wide[3], zero)[0]
        rho, a_out = EB.allowances(mat, rows, cols, HH.SCALE, wide[0], wide[1], wide[2], wide[3], zero, np.float32, STAGES)[:2]
        rhos["mhaLowp." + kind] = rho
        assert STAGES * rho <= FIRST_ORDER, (what, kind, rho)
        allowed = a_out + _t(L.round_allowance(want.cpu().numpy(), kind))
        _within(_t(L.widen(res["mhaLowp." + kind], kind)), want, allowed, f"{what} mhaLowp {kind}")
    print(f"{what}: rho " + ", ".join(f"{n} {r:.3e}" for n, r in rhos.items()))
    return single


def _anchor(key, res, info, zero_empty, what):
    mat, dtype, _ = _KEYED[key]
    if mat.nnz == 0:
        return _anchor_empty(mat, res)
    _check_products(key, res, info, zero_empty, what)
    first = _ANCHORS.get(key)
    if first is None:
        first = _ANCHORS[key] = (res, _anchor_attention(key, res, what))
    else:  # a twin of another sigma or other options: the anchored twin's bits wherever they depend on neither
        mine = {n: a for n, a in res.items() if not n.startswith(BY_CONVERSION)}
        assert mine and HH.same(mine, {n: first[0][n] for n in mine}) is None, (what, HH.same(mine, {n: first[0][n] for n in mine}))
    want, allow = first[1]
    for n, w, a in zip(("O", "dQ", "dK", "dV"), want, allow):
        _within(_t(res["autograd.attention." + n]), w, a, f"{what} autograd.attention {n}")


# ---- D. one more call from a graph -----------------------------------------------------------------------------------------------------
def _replays_from_a_graph(A, mat, dtype, res):
    """the pattern of tests/test_gpu_mha_edge_bias.py::test_both_calls_replay_from_a_graph, for the backward alone"""
    o = HH.operands(mat, dtype, SEED)
    Q, K, V, dO, Bt = (_t(o[n]) for n in ("Q", "K", "V", "dO", "B"))
    outs = [torch.full(t.shape, POISON, dtype=t.dtype, device=DEV) for t in (Q, K, V, Bt)]
    work = torch.empty(4 * mat.m * HH.MHA[0], dtype=Q.dtype, device=DEV)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert A.setStream(side) == 0

    def call():
        assert A.mhaEdgeBiasBackward(Q, K, V, dO, outs[0], outs[1], outs[2], work, B=Bt, scale=HH.SCALE, dB=outs[3]) == 0, _capi.last_error()
    with torch.cuda.stream(side):
        call()  # (the stream has run the call once before the capture)
    torch.cuda.synchronize()
    held = A.info().device_bytes
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        call()
    assert A.info().device_bytes == held
    torch.cuda.synchronize()
    for t in outs:
        t.fill_(POISON)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    got = {"mhaEdgeBias." + n: t.cpu().numpy() for n, t in zip(("dQ", "dK", "dV", "dB"), outs)}
    del graph
    assert A.setStream(None) == 0
    assert HH.same(got, {n: res[n] for n in got}) is None, HH.same(got, {n: res[n] for n in got})


# ---- C. back to CSR ----------------------------------------------------------------------------------------------------------------
def _back_to_csr(A, mat, dtype, loaded):
    assert A.asCSR() == 0, _capi.last_error()
    torch.cuda.synchronize()
    if loaded:
        own = A.arrays.to_host()
        rp, ci, va = own.row_ptr, own.col, own.val
    else:
        rp, ci, va = (t.cpu().numpy() for t in A._arrays)
    assert np.array_equal(rp, mat.row_ptr.astype(np.int32)) and np.array_equal(ci, mat.col[:mat.nnz].astype(np.int32))
    assert va.dtype == dtype and np.array_equal(HH._bits(va), HH._bits(np.asarray(A.last_values, dtype=dtype)))


def _read(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_dt)
@pytest.mark.parametrize("which, history", CASES, ids=[f"{m}-{h}" for m, h in CASES])
def test_a_history_leaves_no_trace(which, history, dtype, tmp_path):
    t0 = time.perf_counter()
    mat = _mats()[which]
    hist = HH.HISTORIES[history]
    val = HH.values(mat, 880, dtype)
    what = f"{which} {history} {_dt(dtype)}"
    A, twin = hist.build(mat, val, dtype, tmp_path)
    tmat = mat if twin.mat is None else twin.mat
    tval = val if twin.val is None else twin.val
    T = HH.fresh(tmat, tval, dtype, twin.path())
    parts = HH.PARTS if tmat.nnz else tuple(p for p in HH.PARTS if p != "autograd")
    if history.startswith("second-matrix"):  # E: the companion went with the first matrix and is never built lazily
        x, y = torch.ones(tmat.m, dtype=HH._tdt(dtype), device=DEV), torch.full((tmat.n,), Y0, dtype=HH._tdt(dtype), device=DEV)
        assert A.info().transpose_built == 0
        assert A.spmvT(x, y) == _capi.INVALID_ARGUMENT and "csr5hip_build_transpose" in _capi.last_error()
        torch.cuda.synchronize()
        assert bool((y == Y0).all())
    # C: what a save writes
    mine, twins = str(tmp_path / "again.csr5"), str(tmp_path / "twin.csr5")
    assert A.save(mine) == 0 and T.save(twins) == 0, _capi.last_error()
    assert _read(mine) == _read(twins), what
    if hist.loaded and hist.file_sigma == hist.sigma:
        assert _read(mine) == _read(A.saved_file), what
    # A: the same conversion, then the same bits
    assert A.buildTranspose() == 0 and T.buildTranspose() == 0, _capi.last_error()
    ia, it = _info(A), _info(T)
    assert ia == it, (what, {n: (ia[n], it[n]) for n in ia if ia[n] != it[n]})
    if which == "hub-columns":  # the slab structure is really there where the history asks for it, and nowhere else
        slabs = (8, 1) if history in ("options-toggled", "second-matrix-under-slabs") else (0, 0)
        assert (it["column_slabs"], it["slab_hot"]) == slabs, (what, it)
    res_a = HH.battery(A, tmat, dtype, SEED, parts)
    res_t = HH.battery(T, tmat, dtype, SEED, parts)
    assert HH.same(res_a, res_t) is None, (what, HH.same(res_a, res_t))
    assert _info(A) == _info(T), what
    # B: the twin's numbers are checked numbers
    _anchor(_key(tmat, dtype, tval), res_t, _info(T), dict(twin.opts).get("setZeroEmptyRows", 0) == 1, what)
    # D: the companion is there and a backward replays from a graph
    for X in (T, A):
        assert X.info().transpose_built == 1
        _replays_from_a_graph(X, tmat, dtype, res_t)
    if history == "second-matrix":
        assert A.info().device_bytes <= A.bytes_first, (what, A.info().device_bytes, A.bytes_first)
    # C: back to CSR, close, and the file once more
    _back_to_csr(A, tmat, dtype, hist.loaded)
    _back_to_csr(T, tmat, dtype, False)
    if hist.loaded:
        A.close()
        B = H.anonymouslibHandle.load(A.saved_file)
        ib = B.info()
        assert (ib.sigma, ib.m, ib.n, ib.nnz, ib.format) == (hist.file_sigma, mat.m, mat.n, mat.nnz, _capi.FORMAT_CSR5)
        if hist.file_sigma == hist.sigma:  # the file's values are the twin's: its first product once more
            x, y = _t(HH.operands(mat, dtype, SEED)["x"]), torch.full((mat.m,), Y0, dtype=HH._tdt(dtype), device=DEV)
            assert B.setX(x) == 0 and B.spmv(1.0, y) == 0, _capi.last_error()
            torch.cuda.synchronize()
            assert HH.same({"spmv": y.cpu().numpy()}, {"spmv": res_t["spmv"]}) is None, what
        B.close()
    else:
        _close(A)
    _close(T)
    print(f"{what}: {time.perf_counter() - t0:.2f} s")
