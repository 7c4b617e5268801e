"""csr5hip_mha_lowp_backward (``A.mhaLowpBackward``) and the fp32-handle backward of ``autograd.multihead_attention``'s 16-bit route
on the GPU: the gradients of softmax(scale Q K^T + B) V on the pattern with Q, K, V, B and dO STORED in bf16 or fp16, dQ, dK, dV
and dB written in that type, and everything computed in fp32 (the workspace included).

THE DEFINITION, and test 1: the kernels run ``mhaEdgeBiasBackward``'s fp32 statements in their order on the widened operands and
round each output once where they store it, so, for each of dQ, dK, dV and dB,

    mhaLowpBackward(Q, K, V, dO, B, scale)  ==  mhaEdgeBiasBackward(Q.float(), K.float(), V.float(), dO.float(), B.float(), scale).to(type)

on an fp32 handle of the same pattern, as 16-bit words (a NaN wherever a NaN is expected: payloads are no part of the contract),
and the row kernel's workspace values M, 1 / Z and D are the fp32 call's bits.  Tests 2, 3, 4, 5, 8 and 9 are further identities of
words; 6 goes to a float64 torch reference under tests/edge_bias_reference.py's fp32 allowances plus ONE rounding to the operand
type (tests/lowp_reference.round_allowance: derived, not measured).

B: 16 bits cannot give nnz H distinct values, so B is drawn uniformly in [-2, 2) and rounded to the operand type, as in
tests/test_gpu_mha_lowp.py; a bias read from another entry or head still differs from the right one in all but a few hundred of the
values.  In test 1 head 0 of it holds -Inf in every seventh entry and in one whole row (tests/lowp_backward_reference.masked_bias).

Every output is pre-filled with the word 0x5A5A (2^53-ish in bf16, 203.25 in fp16: no gradient of these inputs) and must have been
overwritten everywhere."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from benchmark_spmv_using_csr5_amd import _capi  # noqa: E402
from benchmark_spmv_using_csr5_amd import autograd  # noqa: E402
from benchmark_spmv_using_csr5_amd import handle as H  # noqa: E402
from tests import attention_edges as E  # noqa: E402
from tests import edge_bias_reference as EB  # noqa: E402
from tests import lowp_backward_reference as LB  # noqa: E402
from tests import lowp_reference as L  # noqa: E402
from tests import sddmm_reference as S  # noqa: E402
from tests import zoo  # noqa: E402
from tests.test_gpu_attention_autograd import FIRST_ORDER, STAGES, _index  # noqa: E402
from tests.test_gpu_exact_reference import DEV, Path, _close, _handle  # noqa: E402

AUTO = H.ANONYMOUSLIB_AUTO_TUNED_SIGMA
TDT = {"bf16": torch.bfloat16, "f16": torch.float16}
POISON_WORD = 0x5A5A
SCALE = 0.25
SHAPES = ((1, 16, 16), (3, 3, 5), (2, 24, 8), (3, 12, 65))
MATRICES = ("kat0", "half-empty", "two-hubs", "duplicates", "class-edges", "class-edges^T", "dealt")
NAMES = ("dQ", "dK", "dV", "dB")


@functools.lru_cache(maxsize=1)
def _zoo():
    z = {m.name: m for m in zoo.small_zoo()}
    z["kat0"] = zoo.kat0()
    z["duplicates"] = S.duplicates_matrix()
    z["class-edges"] = E.class_edges()
    z["class-edges^T"] = EB.transposed(E.class_edges())
    z["dealt"] = E.dealt()
    return z


def _open(mat, dtype=np.float32, val=None, transpose=True):
    val = np.ones(mat.nnz) if val is None else val
    A = _handle(mat, np.asarray(val, dtype=dtype), Path("lowp-bwd", AUTO, H.SPMV_FUSED), dtype)[0]
    if transpose:
        assert A.buildTranspose() == 0, _capi.last_error()
    return A


def _kind(t):
    return "bf16" if t.dtype == torch.bfloat16 else "f16"


def _draw(rng, shape, kind, lo=-1.0, hi=1.0):
    """uniform in [lo, hi), rounded once to the operand type"""
    return torch.from_numpy(rng.uniform(lo, hi, size=shape).astype(np.float32)).to(DEV).to(TDT[kind])


def _operands(mat, heads, k, d, kind, seed):
    """(B, Q, K, V, dO) of the operand type: B and Q in [-2, 2), K, V and dO in [-1, 1)"""
    rng = np.random.default_rng([seed, heads, k, d, len(kind)])
    return (_draw(rng, (mat.nnz, heads), kind, -2, 2), _draw(rng, (mat.m, heads, k), kind, -2, 2), _draw(rng, (mat.n, heads, k), kind),
            _draw(rng, (mat.n, heads, d), kind), _draw(rng, (mat.m, heads, d), kind))


def _words(t):
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _of_words(w, kind):
    return torch.from_numpy(np.ascontiguousarray(w).view(np.int16)).to(DEV).view(TDT[kind])


def _poison(shape, kind):
    return torch.full(tuple(shape), POISON_WORD, dtype=torch.int16, device=DEV).view(TDT[kind])


def _work(mat, heads):
    return torch.full((4 * mat.m * heads,), float("nan"), dtype=torch.float32, device=DEV)


def _lowp(A, mat, Q, K, V, dO, Bt=None, scale=SCALE, want="QKVB"):
    """(dQ, dK, dV, dB, work) of one mhaLowpBackward; ``want``: the outputs asked for (B only with a bias), None for the others"""
    kind, heads = _kind(Q), Q.shape[1]
    dQ = _poison(Q.shape, kind) if "Q" in want else None
    dK = _poison(K.shape, kind) if "K" in want else None
    dV = _poison(V.shape, kind) if "V" in want else None
    dB = _poison(Bt.shape, kind) if "B" in want and Bt is not None else None
    work = _work(mat, heads) if dK is not None or dV is not None else None
    assert A.mhaLowpBackward(Q, K, V, dO, dQ, dK, dV, work, B=Bt, scale=scale, dB=dB) == 0, _capi.last_error()
    torch.cuda.synchronize()
    for t, what in zip((dQ, dK, dV, dB), NAMES):
        assert t is None or not (_words(t) == POISON_WORD).any(), f"an element of {what} was not written"
    return dQ, dK, dV, dB, work


def _rounded_fp32(A32, mat, Q, K, V, dO, Bt=None, scale=SCALE):
    """the definition's right-hand side: mhaEdgeBiasBackward on an fp32 handle on the widened operands, each output cast to the
    operand type; and its workspace"""
    outs = [torch.full(t.shape, float("nan"), dtype=torch.float32, device=DEV) for t in (Q, K, V)]
    dB = torch.full(Bt.shape, float("nan"), dtype=torch.float32, device=DEV) if Bt is not None else None
    work = _work(mat, Q.shape[1])
    assert A32.mhaEdgeBiasBackward(Q.float(), K.float(), V.float(), dO.float(), outs[0], outs[1], outs[2], work,
                                   B=None if Bt is None else Bt.float(), scale=scale, dB=dB) == 0, _capi.last_error()
    torch.cuda.synchronize()
    return tuple(o.to(Q.dtype) for o in outs) + (dB.to(Q.dtype) if dB is not None else None, work)


def _same(got, want, kind):
    return L.same_words(_words(got), _words(want), kind)


def _same_work(got, want, mat, heads):
    """M, 1 / Z and D of every (row, head) as float32 bits (the fourth value is unused); NaN positionally"""
    g = got.cpu().numpy().reshape(mat.m, heads, 4)[:, :, :3]
    w = want.cpu().numpy().reshape(mat.m, heads, 4)[:, :, :3]
    return bool(((g.view(np.uint32) == w.view(np.uint32)) | (np.isnan(g) & np.isnan(w))).all())


def _all_same(got, want, kind, where):
    for g, w, what in zip(got[:4], want[:4], NAMES):
        assert (g is None) == (w is None), where + (what,)
        if g is not None:
            assert _same(g, w, kind), where + (what,)


# ---- 1. the rounding identity ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", L.KINDS)
@pytest.mark.parametrize("name", MATRICES)
def test_every_gradient_is_the_rounding_of_the_fp32_calls_on_either_handle(name, kind):
    mat = _zoo()[name]
    A32, A64 = _open(mat, np.float32), _open(mat, np.float64)
    if name == "duplicates":  # (the map must be the stable one: the companion of either handle holds a column's entries in A's order)
        assert (np.diff(mat.row_ptr) > 1).any()
    for si, (heads, k, d) in enumerate(SHAPES):
        Bt, Q, K, V, dO = _operands(mat, heads, k, d, kind, seed=3000 + si)
        Bw, dead = LB.masked_bias(mat, _words(Bt), kind)
        Bt = _of_words(Bw, kind)
        want = _rounded_fp32(A32, mat, Q, K, V, dO, Bt)
        got32, got64 = _lowp(A32, mat, Q, K, V, dO, Bt), _lowp(A64, mat, Q, K, V, dO, Bt)
        where = (name, kind, heads, k, d)
        _all_same(got32, want, kind, where + ("against the rounded fp32 call",))
        assert L.is_nan(_words(got32[0])[dead, 0], kind).all() and not L.is_nan(_words(got32[0])[:, 1:], kind).any()  # one head only
        assert _same_work(got32[4], want[4], mat, heads), where + ("the workspace",)
        for g64, g32, what in zip(got64[:4], got32[:4], NAMES):
            assert np.array_equal(_words(g64), _words(g32)), where + ("the fp64 handle", what)
        assert np.array_equal(got64[4].cpu().numpy().view(np.uint32), got32[4].cpu().numpy().view(np.uint32)), where + ("fp64 handle: work",)
        # a null B is scaled attention and has no dB
        none = _lowp(A32, mat, Q, K, V, dO, None)
        _all_same(none, _rounded_fp32(A32, mat, Q, K, V, dO, None), kind, where + ("B = None",))
    _close(A32)
    _close(A64)


# ---- 2. the load width decides no bit -----------------------------------------------------------------------------------------------
def _shifted(t):
    """the same numbers in a view that starts ONE element into a larger buffer"""
    buf = torch.empty(t.numel() + 9, dtype=t.dtype, device=DEV)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def _odd_ld(t):
    """the same numbers in rows of an ODD leading dimension, NaN in the padding"""
    w = int(np.prod(t.shape[1:]))
    ld = w + 1 + w % 2
    buf = torch.full((t.shape[0], ld), float("nan"), dtype=t.dtype, device=DEV)
    v = buf[:, :w] if t.dim() == 2 else buf[:, :w].unflatten(1, tuple(t.shape[1:]))
    v.copy_(t)
    assert v.stride(0) % 2 == 1
    return v


@pytest.mark.parametrize("kind", L.KINDS)
@pytest.mark.parametrize("k", (16, 40))
@pytest.mark.parametrize("name", ("class-edges", "class-edges^T"))
def test_the_load_width_decides_no_bit(name, k, kind):
    mat = _zoo()[name]
    A = _open(mat)
    heads, d = 2, 16
    Bt, Q, K, V, dO = _operands(mat, heads, k, d, kind, seed=3100 + k)
    for t, w in ((Q, k), (K, k), (V, d), (dO, d)):  # the vector path: attention_bwd_vec's rule in 2-byte elements
        assert t.data_ptr() % 16 == 0 and t.is_contiguous() and (heads * w * 2) % 16 == 0 and (w * 2) % 16 == 0
    vec = _lowp(A, mat, Q, K, V, dO, Bt)
    _all_same(vec, _rounded_fp32(A, mat, Q, K, V, dO, Bt), kind, (name, k, kind, "16-byte loads"))
    shifted = tuple(_shifted(t) for t in (Q, K, V, dO, Bt))
    assert all(t.data_ptr() % 16 == 2 for t in shifted[:4])
    odd = tuple(_odd_ld(t) for t in (Q, K, V, dO, Bt))
    for what, (q, k_, v, do, b) in (("one element into a buffer", shifted), ("odd leading dimensions", odd),
                                    ("only dO off the boundary", (Q, K, V, shifted[3], Bt))):
        got = _lowp(A, mat, q, k_, v, do, b)
        for g, w, out in zip(got[:4], vec[:4], NAMES):
            assert np.array_equal(_words(g), _words(w)), (name, k, kind, what, out)
    _close(A)


# ---- 3. a head of the packed call is the one-head call on its slices -------------------------------------------------------------
def _head_by_head(A, mat, heads, k, d, kind, seed):
    Bt, Q, K, V, dO = _operands(mat, heads, k, d, kind, seed)
    packed = [_words(t) for t in _lowp(A, mat, Q, K, V, dO, Bt)[:4]]
    for h in range(heads):
        s = slice(h, h + 1)
        one = _lowp(A, mat, Q[:, s], K[:, s], V[:, s], dO[:, s], Bt[:, s])
        for o, p, what in zip(one[:4], packed, NAMES):
            assert np.array_equal(_words(o)[:, 0], p[:, h]), (mat.name, kind, heads, "head", h, what)


@pytest.mark.parametrize("kind", L.KINDS)
@pytest.mark.parametrize("name", ("class-edges", "class-edges^T"))
def test_three_heads_on_the_class_edges_are_three_one_head_calls(name, kind):
    mat = _zoo()[name]
    A = _open(mat)
    _head_by_head(A, mat, 3, 16, 8, kind, seed=3200)
    _head_by_head(A, mat, 3, 12, 65, kind, seed=3201)
    _close(A)


@pytest.mark.parametrize("kind", L.KINDS)
@pytest.mark.parametrize("lines, per_group", ((90113, 3), (256 * 1023 + 1, 8)), ids=("groups-3-3-2", "one-group"))
def test_eight_heads_in_head_groups_are_eight_one_head_calls(lines, per_group, kind):
    """tests/test_gpu_mha_lowp.py's two line counts; the matrices are square, so both kernels see these head groups"""
    assert E.heads_per_group(lines, 8) == per_group
    mat = E.many_lines(lines)
    assert mat.n == lines
    A = _open(mat)
    _head_by_head(A, mat, 8, 16, 1, kind, seed=3210)
    _close(A)


# ---- 4. subsets of the outputs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", L.KINDS)
def test_a_subset_of_the_outputs_has_the_words_of_the_whole_call(kind):
    mat = _zoo()["class-edges"]
    heads, k, d = 3, 12, 5
    Bt, Q, K, V, dO = _operands(mat, heads, k, d, kind, seed=3300)
    bare = _open(mat, transpose=False)  # dQ and dB need neither the companion nor the workspace
    only_q = _lowp(bare, mat, Q, K, V, dO, Bt, want="Q")
    only_b = _lowp(bare, mat, Q, K, V, dO, Bt, want="B")
    assert bare.info().transpose_built == 0
    _close(bare)
    A = _open(mat)
    full = _lowp(A, mat, Q, K, V, dO, Bt)
    only_k, only_v = _lowp(A, mat, Q, K, V, dO, Bt, want="K"), _lowp(A, mat, Q, K, V, dO, Bt, want="V")
    _close(A)
    for i, got in enumerate((only_q, only_k, only_v, only_b)):
        assert [t is not None for t in got[:4]] == [j == i for j in range(4)]
        assert np.array_equal(_words(got[i]), _words(full[i])), (kind, NAMES[i], "alone")


# ---- 5. writes and reads ----------------------------------------------------------------------------------------------------------
def _guarded(rows, width, kind, guard=64, extra=3):
    """(buffer, view (rows, width) with leading dimension width + extra inside it, that leading dimension)"""
    ld = width + extra
    buf = _poison((guard + rows * ld + guard,), kind)
    return buf, buf[guard:guard + rows * ld].view(rows, ld)[:, :width], ld


def _guard_intact(buf, rows, width, ld, what, guard=64):
    whole = _words(buf)
    body = whole[guard:guard + rows * ld].reshape(rows, ld)
    assert (whole[:guard] == POISON_WORD).all() and (whole[-guard:] == POISON_WORD).all() and (body[:, width:] == POISON_WORD).all(), what
    assert not (body[:, :width] == POISON_WORD).any(), f"an element of {what} was not written"
    return body[:, :width]


def _padded(t, extra):
    """(buffer, view): the same numbers in rows ``extra`` elements wider, NaN in the padding"""
    w = int(np.prod(t.shape[1:]))
    buf = torch.full((t.shape[0], w + extra), float("nan"), dtype=t.dtype, device=DEV)
    buf[:, :w] = t.reshape(t.shape[0], w)
    return buf, (buf[:, :w] if t.dim() == 2 else buf[:, :w].unflatten(1, tuple(t.shape[1:])))


@pytest.mark.parametrize("kind", L.KINDS)
def test_only_the_declared_elements_are_read_and_written(kind):
    heads, k, d = 3, 16, 5
    for name in ("half-empty", "class-edges"):
        mat = _zoo()[name]
        A = _open(mat, val=np.full(mat.nnz, np.nan))  # (NaN in the handle's values, the parent's and the companion's: they are not read)
        Bt, Q, K, V, dO = _operands(mat, heads, k, d, kind, seed=3500)
        want = _lowp(A, mat, Q, K, V, dO, Bt)
        assert not any(L.is_nan(_words(t), kind).any() for t in want[:4])
        info0, bytes0 = bytes(A.info()), A.info().device_bytes
        (bw, Bv), (_, Qv), (_, Kv), (_, Vv), (_, dOv) = _padded(Bt, 3), _padded(Q, 8), _padded(K, 3), _padded(V, 2), _padded(dO, 5)
        kept = bw.clone()
        bufs = [_guarded(r, heads * w, kind) for r, w in ((mat.m, k), (mat.n, k), (mat.n, d))] + [_guarded(mat.nnz, heads, kind)]
        views = [b[1].unflatten(1, (heads, w)) for b, w in zip(bufs[:3], (k, k, d))] + [bufs[3][1]]  # dB: a slice of a wider tensor
        assert A.mhaLowpBackward(Qv, Kv, Vv, dOv, views[0], views[1], views[2], _work(mat, heads), B=Bv, scale=SCALE, dB=views[3]) == 0, \
            _capi.last_error()
        torch.cuda.synchronize()
        for (b, _, ld), w, width, rws, what in zip(bufs, want, (heads * k, heads * k, heads * d, heads), (mat.m, mat.n, mat.n, mat.nnz), NAMES):
            body = _guard_intact(b, rws, width, ld, what)
            assert not L.is_nan(body, kind).any(), "padding was read"
            assert np.array_equal(body, _words(w).reshape(rws, -1)), (name, kind, what)
        assert np.array_equal(_words(bw), _words(kept))  # B is only read
        assert bytes(A.info()) == info0 and A.info().device_bytes == bytes0
        _close(A)


# ---- 6. the float64 reference -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", L.KINDS)
@pytest.mark.parametrize("which", ("class-edges", "random"))
def test_the_gradients_match_the_float64_reference(which, kind):
    """|got - ref| <= the fp32 allowance of tests/edge_bias_reference.py for that gradient (on the widened operands: what the kernels
    compute before they store) + one rounding to the operand type"""
    mat = _zoo()["class-edges"] if which == "class-edges" else EB.random_matrix()
    rows, cols = _index(mat)
    heads, k, d = EB.F_HEADS, EB.F_K, EB.F_D
    words, scale = LB.f64_case(mat, kind, heads, k, d)  # (the condition on rho for these inputs: tests/test_mha_lowp_backward_host.py too)
    Bt, Q, K, V, dO = (_of_words(w, kind) for w in words)
    A = _open(mat)
    got = _lowp(A, mat, Q, K, V, dO, Bt, scale=scale)
    _close(A)
    wide = [t.float() for t in (Bt, Q, K, V, dO)]
    want = EB.reference(mat, rows, cols, scale, *wide)[1:]
    allow = EB.allowances(mat, rows, cols, scale, *wide, np.float32, STAGES)
    assert STAGES * allow[0] <= FIRST_ORDER, (mat.name, allow[0])
    for g, w, a, what in zip(got[:4], want, allow[2:], NAMES):
        allowed = a + torch.from_numpy(L.round_allowance(w.cpu().numpy(), kind)).to(DEV)
        err = (g.double() - w).abs()
        print(f"{mat.name} {kind} {what}: rho {allow[0]:.3e}, worst |error| / allowance {float((err / allowed.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= allowed).all()), (mat.name, kind, what)


# ---- 7. degenerate shapes and the order of errors ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", L.KINDS)
def test_degenerate_shapes_and_the_error_order(kind):
    ot = _capi.BF16 if kind == "bf16" else _capi.F16
    mat = _zoo()["half-empty"]
    A = _open(mat, transpose=False)
    Bt, Q, K, V, dO = _operands(mat, 3, 4, 6, kind, seed=3600)
    dQ, dK, dB = _poison(Q.shape, kind), _poison(K.shape, kind), _poison(Bt.shape, kind)
    work = _work(mat, 3)
    INV = _capi.INVALID_ARGUMENT

    def call(t, heads, scale, ldb, q, dq, dk, lddb, k=4, d=6, wk=None):
        return A.mha_lowp_backward_ptr(t, heads, scale, Bt, ldb, q, 12, K, 12, k, V, 18, d, dO, 18, dq, 12, dk, 12, None, 18, wk, dB, lddb)
    assert call(ot, 0, 1.0, 3, Q, dQ, None, 3) == 0, _capi.last_error()  # heads = 0
    for bad in (_capi.F64, _capi.F32, 4, -1):
        assert call(bad, 3, 1.0, 3, Q, dQ, None, 3) == _capi.UNSUPPORTED_VALUE_TYPE
    assert call(7, -1, float("nan"), 3, Q, dQ, None, 3) == _capi.UNSUPPORTED_VALUE_TYPE  # the type comes before everything but the handle
    assert call(ot, -1, 1.0, 3, Q, dQ, None, 3) == INV
    assert call(ot, 3, float("nan"), 3, None, dQ, None, 3) == INV
    assert call(ot, 3, float("inf"), 3, Q, dQ, None, 3) == INV
    assert call(ot, 3, 1.0, 2, Q, dQ, None, 3) == INV  # ldb < heads
    assert call(ot, 3, 1.0, 3, Q, dQ, None, 2) == INV  # lddb < heads
    assert call(ot, 3, 1.0, 3, Q, None, dK, 3, wk=None) == INV  # dK without the workspace
    # dK without a companion: INVALID_ARGUMENT and a text under this call's name
    assert A.mhaLowpBackward(Q, K, V, dO, dK=dK, work=work, B=Bt) == INV
    assert "transposed companion" in _capi.last_error() and "csr5hip_mha_lowp_backward" in _capi.last_error()
    torch.cuda.synchronize()
    assert all((_words(t) == POISON_WORD).all() for t in (dQ, dK, dB)) and bool(torch.isnan(work).all())
    assert A.buildTranspose() == 0, _capi.last_error()
    # k = 0: every score is the bias alone -- the words of Q = +0 at k = 4 (qk = +0 either way); dQ and dK have no element
    Q0, K0 = (torch.zeros((r, 3, 0), dtype=TDT[kind], device=DEV) for r in (mat.m, mat.n))
    zeroed = _lowp(A, mat, torch.zeros_like(Q), K, V, dO, Bt, scale=0.7, want="VB")
    dV0, dB0 = _poison(V.shape, kind), _poison(Bt.shape, kind)
    assert A.mhaLowpBackward(Q0, K0, V, dO, dV=dV0, work=work, B=Bt, scale=0.7, dB=dB0) == 0, _capi.last_error()
    torch.cuda.synchronize()
    assert np.array_equal(_words(dV0), _words(zeroed[2])) and np.array_equal(_words(dB0), _words(zeroed[3]))
    # d = 0: dB is the score gradient of an empty product, a zero wherever p is finite
    V0, dO0 = (torch.zeros((r, 3, 0), dtype=TDT[kind], device=DEV) for r in (mat.n, mat.m))
    dB0 = _poison(Bt.shape, kind)
    assert A.mhaLowpBackward(Q, K, V0, dO0, B=Bt, dB=dB0) == 0, _capi.last_error()
    torch.cuda.synchronize()
    assert not (_words(dB0) & 0x7FFF).any()
    # nothing wanted: a successful no-op
    assert A.mhaLowpBackward(Q, K, V, dO, B=Bt) == 0, _capi.last_error()
    _close(A)
    none = zoo.empty_matrix()  # nnz = 0 with m > 0: the word 0x0000 in every wanted output, no element of dB
    assert none.m > 0 and none.nnz == 0
    A = _open(none)
    Bt, Q, K, V, dO = _operands(none, 3, 4, 6, kind, seed=3601)
    for t in _lowp(A, none, Q, K, V, dO, Bt)[:4]:
        assert not _words(t).any()
    _close(A)
    nothing = type(none)(0, 5, np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0), "no-rows")  # m = 0
    A = _open(nothing)
    K, V = _draw(np.random.default_rng(1), (5, 3, 4), kind), _draw(np.random.default_rng(2), (5, 3, 6), kind)
    Q, dO = (torch.zeros((0, 3, w), dtype=TDT[kind], device=DEV) for w in (4, 6))
    dK, dV = _poison(K.shape, kind), _poison(V.shape, kind)
    assert A.mhaLowpBackward(Q, K, V, dO, torch.zeros_like(Q), dK, dV, torch.zeros(0, dtype=torch.float32, device=DEV)) == 0, _capi.last_error()
    torch.cuda.synchronize()
    assert not _words(dK).any() and not _words(dV).any()  # no row attends to anything: every gradient of K and V is +0
    _close(A)


# ---- 8. graph capture on the first use ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", L.KINDS)
def test_the_call_is_captured_on_its_first_use_and_replays_with_new_operands(kind):
    mat = _zoo()["half-empty"]
    A = _open(mat)  # (a fresh handle with its companion: the captured call is the first mhaLowpBackward it sees)
    Bt, Q, K, V, dO = _operands(mat, 3, 16, 6, kind, seed=3700)
    outs = [_poison(t.shape, kind) for t in (Q, K, V, Bt)]
    work = _work(mat, 3)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert A.setStream(side) == 0
    held = A.info().device_bytes
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        assert A.mhaLowpBackward(Q, K, V, dO, outs[0], outs[1], outs[2], work, B=Bt, scale=SCALE, dB=outs[3]) == 0, _capi.last_error()
    assert A.info().device_bytes == held
    torch.cuda.synchronize()
    new = _operands(mat, 3, 16, 6, kind, seed=3701)
    for t, n in zip((Bt, Q, K, V, dO), new):
        assert not torch.equal(t, n)
        t.copy_(n)  # changed in place: the graph reads the same addresses
    for o in outs:
        o.view(torch.int16).fill_(POISON_WORD)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    replayed = [_words(o).copy() for o in outs]
    del graph
    assert A.setStream(None) == 0
    eager = _lowp(A, mat, new[1], new[2], new[3], new[4], new[0])
    for r, e, what in zip(replayed, eager[:4], NAMES):
        assert not (r == POISON_WORD).any() and np.array_equal(r, _words(e)), (kind, what)
    _close(A)


# ---- 9. autograd ------------------------------------------------------------------------------------------------------------------
def _counted(A, name, calls):
    real = getattr(A, name)
    setattr(A, name, lambda *a, **kw: calls.append(name) or real(*a, **kw))


@pytest.mark.parametrize("kind", L.KINDS)
def test_autograd_on_an_fp32_handle_is_one_16_bit_backward_call(kind):
    mat = _zoo()["class-edges"]
    A = _open(mat, transpose=False)
    heads, k, d = 3, 8, 16
    Bt, Q, K, V, dO = _operands(mat, heads, k, d, kind, seed=3800)
    calls = []
    _counted(A, "mhaLowpBackward", calls)
    _counted(A, "mhaEdgeBiasBackward", calls)
    _counted(A, "buildTranspose", calls)
    # only Q and the bias want a gradient: no companion, no workspace
    q, b = Q.clone().requires_grad_(True), Bt.clone().requires_grad_(True)
    autograd.multihead_attention(A, q, K, V, scale=SCALE, bias=b).backward(dO)
    torch.cuda.synchronize()
    assert calls == ["mhaLowpBackward"] and A.info().transpose_built == 0
    q_, k_, v, b_ = (t.clone().requires_grad_(True) for t in (Q, K, V, Bt))
    del calls[:]
    out = autograd.multihead_attention(A, q_, k_, v, scale=SCALE, bias=b_)
    out.backward(dO)
    torch.cuda.synchronize()
    assert calls == ["buildTranspose", "mhaLowpBackward"]
    direct = _lowp(A, mat, Q, K, V, dO, Bt)
    for g, w, what in zip((q_.grad, k_.grad, v.grad, b_.grad), direct[:4], NAMES):
        assert g.dtype == TDT[kind] and g.shape == w.shape and np.array_equal(_words(g), _words(w)), (kind, what)
    assert np.array_equal(_words(q.grad), _words(direct[0])) and np.array_equal(_words(b.grad), _words(direct[3]))
    # a strided dO is packed, not widened
    del calls[:]
    q2 = Q.clone().requires_grad_(True)
    out2 = autograd.multihead_attention(A, q2, K, V, scale=SCALE, bias=Bt)
    out2.backward(dO.transpose(1, 2).contiguous().transpose(1, 2))
    torch.cuda.synchronize()
    assert calls == ["mhaLowpBackward"] and np.array_equal(_words(q2.grad), _words(direct[0]))
    # nothing runs in backward when no input needs a gradient
    del calls[:]
    assert not autograd.multihead_attention(A, Q, K, V, scale=SCALE, bias=Bt).requires_grad
    other = torch.ones((), dtype=TDT[kind], device=DEV, requires_grad=True)
    (autograd.multihead_attention(A, Q, K, V, scale=SCALE, bias=Bt).float().sum() * other.float()).backward()
    torch.cuda.synchronize()
    assert calls == []
    _close(A)


@pytest.mark.parametrize("kind", L.KINDS)
def test_autograd_on_an_fp64_handle_still_takes_the_stopgap_and_gives_what_it_gave(kind):
    mat = _zoo()["class-edges"]
    A = _open(mat, np.float64)
    heads, k, d = 3, 8, 16
    Bt, Q, K, V, dO = _operands(mat, heads, k, d, kind, seed=3810)
    calls = []
    _counted(A, "mhaLowpBackward", calls)
    _counted(A, "mhaEdgeBiasBackward", calls)
    q, k_, v, b = (t.clone().requires_grad_(True) for t in (Q, K, V, Bt))
    autograd.multihead_attention(A, q, k_, v, scale=SCALE, bias=b).backward(dO)
    torch.cuda.synchronize()
    assert calls == ["mhaEdgeBiasBackward"]
    del A.mhaLowpBackward, A.mhaEdgeBiasBackward
    # what the stopgap gave: the fp64 call on the widened operands, each gradient cast once
    outs = [torch.full(t.shape, float("nan"), dtype=torch.float64, device=DEV) for t in (Q, K, V, Bt)]
    work = torch.empty(4 * mat.m * heads, dtype=torch.float64, device=DEV)
    assert A.mhaEdgeBiasBackward(Q.double(), K.double(), V.double(), dO.double(), outs[0], outs[1], outs[2], work, B=Bt.double(), scale=SCALE,
                                 dB=outs[3]) == 0, _capi.last_error()
    torch.cuda.synchronize()
    for g, w, what in zip((q.grad, k_.grad, v.grad, b.grad), outs, NAMES):
        assert g.dtype == TDT[kind] and _same(g, w.to(TDT[kind]), kind), (kind, what)
    _close(A)
