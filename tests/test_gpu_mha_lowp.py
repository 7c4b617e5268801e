"""csr5hip_mha_lowp (``A.mhaLowp``) and the 16-bit route of ``autograd.multihead_attention`` on the GPU: softmax(scale Q K^T + B) V
on the pattern with Q, K, V, B and O STORED in bf16 or fp16 and everything computed in fp32.

THE DEFINITION, and test 1: a bf16 or fp16 number is an fp32 number exactly, the kernel runs ``mhaEdgeBias``'s fp32 statements in
their order on the widened operands and rounds O once where it stores it, so

    mhaLowp(Q, K, V, B, scale)  ==  mhaEdgeBias(Q.float(), K.float(), V.float(), B.float(), scale).to(operand type)

on an fp32 handle of the same pattern, as 16-bit words (a NaN wherever a NaN is expected: payloads are no part of the contract).
Tests 2, 3 and 8 are further identities of words; 4 is exact by construction and uses no other kernel; 5 goes to a float64 torch
reference under tests/edge_bias_reference.py's fp32 allowance plus ONE rounding to the operand type
(tests/lowp_reference.round_allowance: derived, not measured).

B: 16 bits cannot give nnz H distinct values, so B is drawn uniformly in [-2, 2) and rounded to the operand type; a bias read from
another entry or head still differs from the right one in all but a few hundred of the values."""
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
from tests import lowp_reference as L  # noqa: E402
from tests import sddmm_reference as S  # noqa: E402
from tests import zoo  # noqa: E402
from tests.test_gpu_attention_autograd import FIRST_ORDER, STAGES, _index  # noqa: E402
from tests.test_gpu_exact_reference import DEV, Path, _close, _handle  # noqa: E402

AUTO = H.ANONYMOUSLIB_AUTO_TUNED_SIGMA
TDT = {"bf16": torch.bfloat16, "f16": torch.float16}
POISON_WORD = 0x5A5A  # (a finite number in both types)
SCALE = 0.25
SHAPES = ((1, 16, 16), (3, 3, 5), (2, 24, 70), (3, 12, 65), (8, 16, 1))
MATRICES = ("kat0", "half-empty", "aligned64", "aligned1024", "two-hubs", "duplicates", "class-edges")


@functools.lru_cache(maxsize=1)
def _zoo():
    z = {m.name: m for m in zoo.small_zoo()}
    z["kat0"] = zoo.kat0()
    z["duplicates"] = S.duplicates_matrix()
    z["class-edges"] = E.class_edges()
    return z


def _open(mat, dtype=np.float32, val=None, sigma=AUTO):
    val = np.ones(mat.nnz) if val is None else val
    return _handle(mat, np.asarray(val, dtype=dtype), Path("lowp", sigma, H.SPMV_FUSED), dtype)[0]


def _draw(rng, shape, kind, lo=-1.0, hi=1.0):
    """uniform in [lo, hi), rounded once to the operand type"""
    return torch.from_numpy(rng.uniform(lo, hi, size=shape).astype(np.float32)).to(DEV).to(TDT[kind])


def _operands(mat, heads, k, d, kind, seed):
    """(B, Q, K, V) of the operand type: B in [-2, 2) per (entry, head), Q in [-2, 2), K and V in [-1, 1)"""
    rng = np.random.default_rng([seed, heads, k, d, len(kind)])
    return (_draw(rng, (mat.nnz, heads), kind, -2, 2), _draw(rng, (mat.m, heads, k), kind, -2, 2), _draw(rng, (mat.n, heads, k), kind),
            _draw(rng, (mat.n, heads, d), kind))


def _words(t):
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _poison(shape, kind):
    return torch.full(tuple(shape), POISON_WORD, dtype=torch.int16, device=DEV).view(TDT[kind])


def _lowp(A, mat, Q, K, V, Bt=None, scale=SCALE):
    O = _poison((mat.m,) + tuple(V.shape[1:]), "bf16" if Q.dtype == torch.bfloat16 else "f16")
    assert A.mhaLowp(Q, K, V, O, B=Bt, scale=scale) == 0, _capi.last_error()
    torch.cuda.synchronize()
    return O


def _rounded_fp32(A32, mat, Q, K, V, Bt=None, scale=SCALE):
    """the definition's right-hand side: mhaEdgeBias on an fp32 handle on the widened operands, cast to the operand type"""
    O = torch.full((mat.m,) + tuple(V.shape[1:]), float("nan"), dtype=torch.float32, device=DEV)
    assert A32.mhaEdgeBias(Q.float(), K.float(), V.float(), O, B=None if Bt is None else Bt.float(), scale=scale) == 0, _capi.last_error()
    torch.cuda.synchronize()
    return O.to(Q.dtype)


def _same(got, want, kind):
    return L.same_words(_words(got), _words(want), kind)


# ---- 1. the rounding identity ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", L.KINDS)
@pytest.mark.parametrize("name", MATRICES)
def test_the_result_is_the_rounding_of_the_fp32_call_on_either_handle(name, kind):
    mat = _zoo()[name]
    A32, A64 = _open(mat, np.float32), _open(mat, np.float64)
    for si, (heads, k, d) in enumerate(SHAPES):
        Bt, Q, K, V = _operands(mat, heads, k, d, kind, seed=2000 + si)
        want = _rounded_fp32(A32, mat, Q, K, V, Bt)
        got32, got64 = _lowp(A32, mat, Q, K, V, Bt), _lowp(A64, mat, Q, K, V, Bt)
        assert not (_words(got32) == POISON_WORD).any(), "an element of O was not written"
        assert _same(got32, want, kind), (name, kind, heads, k, d, "against the rounded fp32 call")
        assert np.array_equal(_words(got64), _words(got32)), (name, kind, heads, k, d, "the fp64 handle")
        # a null B is scaled attention; with scale = 1, mha
        none = _lowp(A32, mat, Q, K, V, None, scale=1.0)
        O = torch.full(want.shape, float("nan"), dtype=torch.float32, device=DEV)
        assert A32.mha(Q.float(), K.float(), V.float(), O) == 0, _capi.last_error()
        torch.cuda.synchronize()
        assert _same(none, O.to(Q.dtype), kind), (name, kind, heads, k, d, "B = None, scale = 1 against mha")
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
    """the same numbers in rows of an ODD leading dimension"""
    w = int(np.prod(t.shape[1:]))
    ld = w + 1 + w % 2
    buf = torch.full((t.shape[0], ld), float("nan"), dtype=t.dtype, device=DEV)
    v = buf[:, :w].view((t.shape[0],) + tuple(t.shape[1:])) if t.dim() == 2 else buf[:, :w].unflatten(1, tuple(t.shape[1:]))
    v.copy_(t)
    assert v.stride(0) % 2 == 1
    return v


@pytest.mark.parametrize("kind", L.KINDS)
@pytest.mark.parametrize("k", (16, 24, 32))
def test_the_load_width_decides_no_bit(k, kind):
    mat = _zoo()["class-edges"]
    A = _open(mat)
    heads, d = 2, 5
    Bt, Q, K, V = _operands(mat, heads, k, d, kind, seed=2100 + k)
    for t in (Q, K):
        assert t.data_ptr() % 16 == 0 and t.is_contiguous() and (heads * k * 2) % 16 == 0 and (k * 2) % 16 == 0  # the vector path
    want = _rounded_fp32(A, mat, Q, K, V, Bt)
    vec = _lowp(A, mat, Q, K, V, Bt)
    assert _same(vec, want, kind), (k, kind, "16-byte loads")
    Qs, Ks, Vs, Bs = (_shifted(t) for t in (Q, K, V, Bt))
    assert Qs.data_ptr() % 16 == 2 and Ks.data_ptr() % 16 == 2
    Qo, Ko, Vo, Bo = (_odd_ld(t) for t in (Q, K, V, Bt))
    for what, ops in (("one element into a buffer", (Qs, Ks, Vs, Bs)), ("odd leading dimensions", (Qo, Ko, Vo, Bo)),
                      ("only K off the boundary", (Q, Ks, V, Bt))):
        got = _lowp(A, mat, ops[0], ops[1], ops[2], ops[3])
        assert np.array_equal(_words(got), _words(vec)), (k, kind, what)
    _close(A)


# ---- 3. a head of the packed call is the one-head call on its slices -------------------------------------------------------------
def _head_by_head(A, mat, heads, k, d, kind, seed):
    Bt, Q, K, V = _operands(mat, heads, k, d, kind, seed)
    packed = _words(_lowp(A, mat, Q, K, V, Bt))
    assert not (packed == POISON_WORD).any()
    for h in range(heads):
        one = _lowp(A, mat, Q[:, h:h + 1], K[:, h:h + 1], V[:, h:h + 1], Bt[:, h:h + 1])
        assert np.array_equal(_words(one)[:, 0], packed[:, h]), (mat.name, kind, heads, "head", h)


@pytest.mark.parametrize("kind", L.KINDS)
def test_three_heads_on_the_class_edges_are_three_one_head_calls(kind):
    mat = _zoo()["class-edges"]
    A = _open(mat)
    _head_by_head(A, mat, 3, 16, 5, kind, seed=2200)
    _head_by_head(A, mat, 3, 12, 65, kind, seed=2201)
    _close(A)


@pytest.mark.parametrize("kind", L.KINDS)
@pytest.mark.parametrize("lines, per_group", ((90113, 3), (256 * 1023 + 1, 8)), ids=("groups-3-3-2", "one-group"))
def test_eight_heads_in_head_groups_are_eight_one_head_calls(lines, per_group, kind):
    """90 113 lines are 353 workgroups: the rule gives three head groups, of 3, 3 and 2 heads; from 1 024 workgroups on all eight
    heads are one group"""
    assert E.heads_per_group(lines, 8) == per_group
    mat = E.many_lines(lines)
    A = _open(mat)
    _head_by_head(A, mat, 8, 16, 1, kind, seed=2210)
    _close(A)


# ---- 4. a mask with exact means ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", L.KINDS)
@pytest.mark.parametrize("name", ("class-edges", "half-empty"))
def test_a_mask_gives_exact_means(name, kind):
    """Q = +0: qk = +0 and s = fma(+0, c, b) = b in {0, -Inf}; the weights are 1 and +0, Z is a count, and O is
    float32(1) / float32(count) * float32(sum of the unmasked integer rows of V), rounded once.  B[e, h] = -Inf where
    (e + h) % 3 == 0: of two consecutive entries one is unmasked, of three one is masked."""
    mat = _zoo()[name]
    heads, k, d = 3, 3, 5
    rng = np.random.default_rng([2300, mat.nnz])
    Vn = rng.integers(-128, 129, size=(mat.n, heads, d)).astype(np.float32)
    keep = [(np.arange(mat.nnz) + h) % 3 != 0 for h in range(heads)]
    lens = np.diff(mat.row_ptr)
    for kh in keep:
        kept = np.bincount(E.rows_of(mat)[kh], minlength=mat.m)
        assert (kept[lens >= 2] > 0).all() and (kept[lens >= 3] < lens[lens >= 3]).all()
    Bt = torch.from_numpy(np.stack([np.where(kh, 0.0, -np.inf) for kh in keep], axis=1).astype(np.float32)).to(DEV).to(TDT[kind])
    V = torch.from_numpy(Vn).to(DEV).to(TDT[kind])
    assert torch.equal(V.float().cpu(), torch.from_numpy(Vn))  # (integers up to 128 are exact in both types)
    Q = torch.zeros((mat.m, heads, k), dtype=TDT[kind], device=DEV)
    K = _draw(rng, (mat.n, heads, k), kind)
    A = _open(mat)
    got = _words(_lowp(A, mat, Q, K, V, Bt, scale=0.5))
    _close(A)
    dead = 0
    for h in range(heads):
        want, mag = E.exact_forward(mat, Vn[:, h], keep[h], np.float32)
        assert mag < E.EXACT_LIMIT
        dead += int(np.isnan(want).any(axis=1).sum())
        assert L.same_words(got[:, h], L.to_words(want, kind), kind), (name, kind, "head", h)
    assert dead > 0  # (a one-entry row whose entry is masked is NaN: the case exists)


# ---- 5. the float64 reference -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", L.KINDS)
@pytest.mark.parametrize("which", ("class-edges", "random"))
def test_the_call_matches_the_float64_reference(which, kind):
    """|got - ref| <= the fp32 allowance of tests/edge_bias_reference.py for O (rho times the expression on absolute values, on the
    widened operands: what the kernel computes before it stores) + one rounding to the operand type"""
    mat = _zoo()["class-edges"] if which == "class-edges" else EB.random_matrix()
    rows, cols = _index(mat)
    heads, k, d = EB.F_HEADS, EB.F_K, EB.F_D
    words, scale = L.f64_case(mat, kind, heads, k, d)  # (the condition on rho for these inputs is judged in tests/test_mha_lowp_host.py too)
    Bt, Q, K, V = (torch.from_numpy(w.view(np.int16)).to(DEV).view(TDT[kind]) for w in words)
    A = _open(mat)
    got = _lowp(A, mat, Q, K, V, Bt, scale=scale).double()
    _close(A)
    wide = [t.float() for t in (Bt, Q, K, V)]
    dO = torch.zeros((mat.m, heads, d), dtype=torch.float32, device=DEV)
    want = EB.reference(mat, rows, cols, scale, wide[0], wide[1], wide[2], wide[3], dO)[0]
    rho, a_out = EB.allowances(mat, rows, cols, scale, wide[0], wide[1], wide[2], wide[3], dO, np.float32, STAGES)[:2]
    assert STAGES * rho <= FIRST_ORDER, (mat.name, rho)
    allowed = a_out + torch.from_numpy(L.round_allowance(want.cpu().numpy(), kind)).to(DEV)
    err = (got - want).abs()
    print(f"{mat.name} {kind}: rho {rho:.3e}, worst |error| / allowance {float((err / allowed.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= allowed).all())


# ---- 6. writes and reads ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", L.KINDS)
def test_only_the_declared_elements_are_read_and_written(kind):
    heads, k, d = 3, 16, 5
    for name in ("half-empty", "class-edges"):
        mat = _zoo()[name]
        A = _open(mat, val=np.full(mat.nnz, np.nan))  # (the handle holds NaN values: they are not read)
        Bt, Q, K, V = _operands(mat, heads, k, d, kind, seed=2500)
        want = _words(_lowp(A, mat, Q, K, V, Bt))
        info0, bytes0 = bytes(A.info()), A.info().device_bytes

        def padded(t, extra):
            w = int(np.prod(t.shape[1:]))
            buf = torch.full((t.shape[0], w + extra), float("nan"), dtype=t.dtype, device=DEV)
            buf[:, :w] = t.reshape(t.shape[0], w)
            return buf, (buf[:, :w] if t.dim() == 2 else buf[:, :w].unflatten(1, tuple(t.shape[1:])))
        (bw, Bv), (_, Qv), (_, Kv), (_, Vv) = padded(Bt, 3), padded(Q, 8), padded(K, 3), padded(V, 2)
        kept = bw.clone()
        guard, ldo = 64, heads * d + 3
        obuf = _poison((guard + mat.m * ldo + guard,), kind)
        Ov = obuf[guard:guard + mat.m * ldo].view(mat.m, ldo)[:, :heads * d].unflatten(1, (heads, d))
        assert A.mhaLowp(Qv, Kv, Vv, Ov, B=Bv, scale=SCALE) == 0, _capi.last_error()
        torch.cuda.synchronize()
        whole = _words(obuf)
        body = whole[guard:guard + mat.m * ldo].reshape(mat.m, ldo)
        assert (whole[:guard] == POISON_WORD).all() and (whole[-guard:] == POISON_WORD).all() and (body[:, heads * d:] == POISON_WORD).all()
        assert not (body[:, :heads * d] == POISON_WORD).any(), "an element of O was not written"
        assert not L.is_nan(body[:, :heads * d], kind).any(), "padding was read"
        assert np.array_equal(body[:, :heads * d].reshape(mat.m, heads, d), want), name
        assert np.array_equal(_words(bw), _words(kept))  # B is only read
        assert bytes(A.info()) == info0 and A.info().device_bytes == bytes0
        _close(A)


# ---- 7. degenerate shapes and the order of errors ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", L.KINDS)
def test_degenerate_shapes_and_the_error_order(kind):
    ot = _capi.BF16 if kind == "bf16" else _capi.F16
    mat = _zoo()["half-empty"]
    A = _open(mat)
    Bt, Q, K, V = _operands(mat, 3, 4, 6, kind, seed=2600)
    O = _poison((mat.m, 3, 6), kind)
    INV = _capi.INVALID_ARGUMENT
    assert A.mha_lowp_ptr(ot, 0, 1.0, Bt, 3, Q, 12, K, 12, 4, V, 18, 6, O, 18) == 0, _capi.last_error()  # heads = 0
    assert A.mha_lowp_ptr(ot, 3, 1.0, Bt, 3, Q, 12, K, 12, 4, V, 18, 0, O, 18) == 0, _capi.last_error()  # d = 0
    for bad in (_capi.F64, _capi.F32, 4, -1):
        assert A.mha_lowp_ptr(bad, 3, 1.0, Bt, 3, Q, 12, K, 12, 4, V, 18, 6, O, 18) == _capi.UNSUPPORTED_VALUE_TYPE
    assert A.mha_lowp_ptr(7, -1, float("nan"), Bt, 3, Q, 12, K, 12, 4, V, 18, 6, O, 18) == _capi.UNSUPPORTED_VALUE_TYPE  # the type comes first
    assert A.mha_lowp_ptr(ot, 3, float("nan"), Bt, 3, None, 0, K, 12, 4, V, 18, 6, O, 18) == INV
    assert A.mha_lowp_ptr(ot, 3, float("inf"), Bt, 3, Q, 12, K, 12, 4, V, 18, 6, O, 18) == INV
    assert A.mha_lowp_ptr(ot, 3, 1.0, Bt, 2, Q, 12, K, 12, 4, V, 18, 6, O, 18) == INV  # ldb < heads
    torch.cuda.synchronize()
    assert (_words(O) == POISON_WORD).all()
    # k = 0: every score is the bias alone -- the words of Q = +0 at k = 4 (qk = +0 either way)
    Q0, K0 = (torch.zeros((r, 3, 0), dtype=TDT[kind], device=DEV) for r in (mat.m, mat.n))
    assert np.array_equal(_words(_lowp(A, mat, Q0, K0, V, Bt, scale=0.7)), _words(_lowp(A, mat, torch.zeros_like(Q), K, V, Bt, scale=0.7)))
    _close(A)
    none = zoo.empty_matrix()  # nnz = 0 with m > 0: the word 0x0000 everywhere
    assert none.m > 0 and none.nnz == 0
    A = _open(none)
    Bt, Q, K, V = _operands(none, 3, 4, 6, kind, seed=2601)
    assert not _words(_lowp(A, none, Q, K, V, Bt)).any()
    _close(A)
    nothing = type(none)(0, 5, np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0), "no-rows")  # m = 0: a no-op
    A = _open(nothing)
    K, V = _draw(np.random.default_rng(1), (5, 3, 4), kind), _draw(np.random.default_rng(2), (5, 3, 6), kind)
    Q, O = (torch.zeros((0, 3, w), dtype=TDT[kind], device=DEV) for w in (4, 6))
    assert A.mhaLowp(Q, K, V, O) == 0, _capi.last_error()
    _close(A)


# ---- 8. graph capture on the first use ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", L.KINDS)
def test_the_call_is_captured_on_its_first_use_and_replays(kind):
    mat = _zoo()["half-empty"]
    A = _open(mat)  # (a fresh handle: the captured call is the first mhaLowp it sees)
    Bt, Q, K, V = _operands(mat, 3, 16, 6, kind, seed=2700)
    O = _poison((mat.m, 3, 6), kind)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert A.setStream(side) == 0
    held = A.info().device_bytes
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        assert A.mhaLowp(Q, K, V, O, B=Bt, scale=SCALE) == 0, _capi.last_error()
    assert A.info().device_bytes == held
    torch.cuda.synchronize()
    replays = []
    for _ in range(2):
        O.view(torch.int16).fill_(POISON_WORD)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        replays.append(_words(O).copy())
    del graph
    assert A.setStream(None) == 0
    eager = _words(_lowp(A, mat, Q, K, V, Bt))
    assert not (eager == POISON_WORD).any()
    for r in replays:
        assert np.array_equal(r, eager)
    _close(A)


# ---- 9. autograd ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", L.KINDS)
def test_autograd_takes_the_16_bit_route_and_its_backward_is_the_fp32_routes(kind):
    mat = _zoo()["class-edges"]
    A = _open(mat)
    heads, k, d = 3, 8, 16
    Bt, Q, K, V = _operands(mat, heads, k, d, kind, seed=2800)
    dO = _draw(np.random.default_rng(2801), (mat.m, heads, d), kind)
    q, k_, v, b = (t.clone().requires_grad_(True) for t in (Q, K, V, Bt))
    out = autograd.multihead_attention(A, q, k_, v, scale=SCALE, bias=b)
    assert out.dtype == TDT[kind]
    out.backward(dO)
    torch.cuda.synchronize()
    assert np.array_equal(_words(out), _words(_lowp(A, mat, Q, K, V, Bt)))
    q32, k32, v32, b32 = (t.float().requires_grad_(True) for t in (Q, K, V, Bt))
    out32 = autograd.multihead_attention(A, q32, k32, v32, scale=SCALE, bias=b32)  # the fp32 route on the widened leaves
    out32.backward(dO.float())
    torch.cuda.synchronize()
    for g, g32, what in zip((q.grad, k_.grad, v.grad, b.grad), (q32.grad, k32.grad, v32.grad, b32.grad), ("dQ", "dK", "dV", "dB")):
        assert g.dtype == TDT[kind] and g.shape == g32.shape
        assert _same(g, g32.to(TDT[kind]), kind), (kind, what)
    # no bias, and only Q wanting a gradient
    q2 = Q.clone().requires_grad_(True)
    out2 = autograd.multihead_attention(A, q2, K, V, scale=SCALE)
    out2.backward(dO)
    q3 = Q.float().requires_grad_(True)
    torch.cuda.synchronize()
    dQ3 = torch.full(q3.shape, float("nan"), dtype=torch.float32, device=DEV)
    assert A.mhaEdgeBiasBackward(q3.detach(), K.float(), V.float(), dO.float(), dQ=dQ3, scale=SCALE) == 0, _capi.last_error()
    torch.cuda.synchronize()
    assert np.array_equal(_words(out2), _words(_lowp(A, mat, Q, K, V, None))) and _same(q2.grad, dQ3.to(TDT[kind]), kind)
    # a 1-D bias or slopes live in the handle's values, which have another type
    with pytest.raises(ValueError, match="1-D bias and slopes"):
        autograd.multihead_attention(A, Q, K, V, bias=Bt[:, 0].contiguous())
    with pytest.raises(ValueError, match="1-D bias and slopes"):
        autograd.multihead_attention(A, Q, K, V, bias=Bt, slopes=torch.ones(heads, dtype=TDT[kind], device=DEV))
    # nothing runs in backward when no input needs a gradient
    calls = []
    real = A.mhaEdgeBiasBackward
    A.mhaEdgeBiasBackward = lambda *a, **kw: calls.append(1) or real(*a, **kw)
    assert not autograd.multihead_attention(A, Q, K, V, scale=SCALE, bias=Bt).requires_grad
    other = torch.ones((), dtype=TDT[kind], device=DEV, requires_grad=True)
    (autograd.multihead_attention(A, Q, K, V, scale=SCALE, bias=Bt).float().sum() * other.float()).backward()
    torch.cuda.synchronize()
    assert calls == []
    del A.mhaEdgeBiasBackward
    _close(A)
