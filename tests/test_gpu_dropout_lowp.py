"""csr5hip_dropout_mha_lowp / csr5hip_dropout_mha_lowp_backward (``A.dropoutMhaLowp``, ``A.dropoutMhaLowpBackward``) and the 16-bit
route of ``autograd.dropout_attention`` on the GPU: dropped multi-head attention on the pattern with Q, K, V, B (and dO) STORED in
bf16 or fp16, O, dQ, dK, dV and dB written in that type, and everything computed in fp32 (cd and the workspace included).

THE DEFINITION, and test 1: the kernels run the fp32 dropped calls' statements in their order on the widened operands and round each
output once where they store it, so on an fp32 handle of the same pattern, as 16-bit words (a NaN wherever a NaN is expected):

    dropoutMhaLowp(Q, K, V, B, scale, p, seed, offset, head0)
        == dropoutMha(Q.float(), K.float(), V.float(), B.float(), scale, p, seed, offset, head0).to(type)
    dropoutMhaLowpBackward(Q, K, V, dO, B, ...)  ==  dropoutMhaBackward(Q.float(), ..., dO.float(), B.float(), ...).to(type)   per output

and the row kernel's workspace values M, 1 / Z and D are the fp32 call's bits.  Tests 2 to 6, 8 and 9 are further identities of
words; 7 goes to the numpy float64 reference with the reference mask under tests/dropout_reference.py's fp32 allowance plus ONE
rounding to the operand type (tests/lowp_reference.round_allowance): both derived, no new number.

WHY 6 HOLDS.  Q = +0 makes every score +0, every weight 1 and Z = L exactly; on ``dealt`` L = 16 in every row, so rinv = 2^-4, and
p = 1/2 gives cd = 2: the row's factor is 2^-3.  V holds integers of magnitude at most 7, so the accumulator over the kept entries
is an integer of magnitude at most 112 in EVERY summation order, exact in fp32, and O = acc / 8 has at most 7 significant bits: a
bf16 (8) and an fp16 (11) hold it exactly.  One wrong mask bit in a row changes that row.

Operands are drawn as in tests/test_gpu_mha_lowp_backward.py (B and Q in [-2, 2), K, V and dO in [-1, 1), rounded once to the type);
every output is pre-filled with the word 0x5A5A and must have been overwritten everywhere."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from benchmark_spmv_using_csr5_amd import _capi  # noqa: E402
from benchmark_spmv_using_csr5_amd import autograd  # noqa: E402
from tests import attention_edges as E  # noqa: E402
from tests import dropout_reference as DR  # noqa: E402
from tests import edge_bias_reference as EB  # noqa: E402
from tests import handle_history as HH  # noqa: E402
from tests import lowp_backward_reference as LB  # noqa: E402
from tests import lowp_reference as L  # noqa: E402
from tests import zoo  # noqa: E402
from tests.test_gpu_attention_autograd import FIRST_ORDER, STAGES  # noqa: E402
from tests.test_gpu_exact_reference import DEV, _close  # noqa: E402
from tests.test_gpu_mha_lowp_backward import (MATRICES, POISON_WORD, SCALE, SHAPES, TDT, _counted, _draw, _guard_intact, _guarded,  # noqa: E402
                                              _odd_ld, _of_words, _open, _operands, _padded, _poison, _same_work, _shifted, _words,
                                              _work, _zoo)
from tests.test_gpu_mha_lowp_backward import _lowp as _undropped_backward  # noqa: E402

NAMES = DR.NAMES  # O, dQ, dK, dV, dB
SEED, OFFSET = 2 ** 63 + 5, 2 ** 32 + 1
DROPS = ((0.1, 0), (0.6, 2), (0.1, 2), (0.6, 0))  # (p, head0); with three heads head0 = 2 straddles a Philox block


def _lowp(A, mat, Q, K, V, dO, p, head0=0, Bt=None, scale=SCALE, want="OQKVB", seed=SEED, offset=OFFSET):
    """[O, dQ, dK, dV, dB, work] of one dropoutMhaLowp and one dropoutMhaLowpBackward; ``want``: the outputs asked for (B only with a
    bias), None for the others"""
    kind, heads = ("bf16" if Q.dtype == torch.bfloat16 else "f16"), Q.shape[1]
    O = _poison((mat.m,) + tuple(V.shape[1:]), kind) if "O" in want else None
    dQ = _poison(Q.shape, kind) if "Q" in want else None
    dK = _poison(K.shape, kind) if "K" in want else None
    dV = _poison(V.shape, kind) if "V" in want else None
    dB = _poison(Bt.shape, kind) if "B" in want and Bt is not None else None
    work = _work(mat, heads) if dK is not None or dV is not None else None
    if O is not None:
        assert A.dropoutMhaLowp(Q, K, V, O, p, seed, offset, head0, B=Bt, scale=scale) == 0, _capi.last_error()
    if any(t is not None for t in (dQ, dK, dV, dB)):
        assert A.dropoutMhaLowpBackward(Q, K, V, dO, p, seed, offset, head0, dQ=dQ, dK=dK, dV=dV, work=work, B=Bt, scale=scale,
                                        dB=dB) == 0, _capi.last_error()
    torch.cuda.synchronize()
    for t, what in zip((O, dQ, dK, dV, dB), NAMES):
        assert t is None or not (_words(t) == POISON_WORD).any(), f"an element of {what} was not written"
    return [O, dQ, dK, dV, dB, work]


def _rounded_fp32(A32, mat, Q, K, V, dO, p, head0=0, Bt=None, scale=SCALE):
    """the definition's right-hand side: the fp32 dropped calls on an fp32 handle on the widened operands, each output cast to the
    operand type; and the backward's workspace"""
    nan = lambda shape: torch.full(tuple(shape), float("nan"), dtype=torch.float32, device=DEV)  # noqa: E731
    O, outs = nan((mat.m,) + tuple(V.shape[1:])), [nan(t.shape) for t in (Q, K, V)]
    dB = nan(Bt.shape) if Bt is not None else None
    work = _work(mat, Q.shape[1])
    Bf = None if Bt is None else Bt.float()
    assert A32.dropoutMha(Q.float(), K.float(), V.float(), O, p, SEED, OFFSET, head0, B=Bf, scale=scale) == 0, _capi.last_error()
    assert A32.dropoutMhaBackward(Q.float(), K.float(), V.float(), dO.float(), p, SEED, OFFSET, head0, dQ=outs[0], dK=outs[1], dV=outs[2],
                                  work=work, B=Bf, scale=scale, dB=dB) == 0, _capi.last_error()
    torch.cuda.synchronize()
    return [O.to(Q.dtype)] + [o.to(Q.dtype) for o in outs] + [dB.to(Q.dtype) if dB is not None else None, work]


def _all_same(got, want, kind, where):
    for g, w, what in zip(got[:5], want[:5], NAMES):
        assert (g is None) == (w is None), where + (what,)
        if g is not None:
            assert L.same_words(_words(g), _words(w), kind), where + (what,)


def _all_equal(got, want, where):
    for g, w, what in zip(got[:5], want[:5], NAMES):
        assert (g is None) == (w is None), where + (what,)
        if g is not None:
            assert np.array_equal(_words(g), _words(w)), where + (what,)


# ---- 1 and 3. the definition, as words, on an fp32 and on an fp64 handle -----------------------------------------------------------
@pytest.mark.parametrize("kind", L.KINDS)
@pytest.mark.parametrize("name", MATRICES)
def test_every_output_is_the_rounding_of_the_fp32_dropped_calls_on_either_handle(name, kind):
    mat = _zoo()[name]
    A32 = _open(mat, np.float32)
    A64 = _open(mat, np.float64, val=np.full(mat.nnz, np.nan))  # (NaN in the values, the parent's and the companion's: they are not read)
    for si, (heads, k, d) in enumerate(SHAPES):
        Bt, Q, K, V, dO = _operands(mat, heads, k, d, kind, seed=4000 + si)
        Bw, dead = LB.masked_bias(mat, _words(Bt), kind)
        Bt = _of_words(Bw, kind)
        for p, head0 in DROPS:
            where = (name, kind, heads, k, d, p, head0)
            want = _rounded_fp32(A32, mat, Q, K, V, dO, p, head0, Bt)
            got32, got64 = _lowp(A32, mat, Q, K, V, dO, p, head0, Bt), _lowp(A64, mat, Q, K, V, dO, p, head0, Bt)
            _all_same(got32, want, kind, where + ("against the rounded fp32 calls",))
            assert L.is_nan(_words(got32[0])[dead, 0], kind).all() and not L.is_nan(_words(got32[0])[:, 1:], kind).any()  # one head only
            assert _same_work(got32[5], want[5], mat, heads), where + ("the workspace",)
            _all_equal(got64, got32, where + ("the fp64 handle",))
            assert np.array_equal(got64[5].cpu().numpy().view(np.uint32), got32[5].cpu().numpy().view(np.uint32)), where + ("fp64: work",)
        none = _lowp(A32, mat, Q, K, V, dO, 0.6, 2, None)  # a null B is scaled attention and has no dB
        _all_same(none, _rounded_fp32(A32, mat, Q, K, V, dO, 0.6, 2, None), kind, (name, kind, heads, k, d, "B = None"))
        assert none[4] is None and not np.array_equal(_words(none[0]), _words(got32[0]))
    _close(A32)
    _close(A64)


# ---- 2. p = 0 is the undropped 16-bit call --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", L.KINDS)
@pytest.mark.parametrize("name", ("half-empty", "two-hubs", "class-edges", "class-edges^T", "dealt"))
def test_p_zero_has_the_words_of_the_undropped_16_bit_calls(name, kind):
    mat = _zoo()[name]
    A = _open(mat)
    for si, (heads, k, d) in enumerate(SHAPES):
        Bt, Q, K, V, dO = _operands(mat, heads, k, d, kind, seed=4100 + si)
        for bias in (Bt, None):
            got = _lowp(A, mat, Q, K, V, dO, 0.0, 2, bias)
            O = _poison(got[0].shape, kind)
            assert A.mhaLowp(Q, K, V, O, B=bias, scale=SCALE) == 0, _capi.last_error()
            grads = _undropped_backward(A, mat, Q, K, V, dO, bias)
            _all_equal(got, [O] + list(grads[:4]), (name, kind, heads, k, d, bias is None))
            assert _same_work(got[5], grads[4], mat, heads)
    _close(A)


# ---- 4. the load width decides no bit -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", L.KINDS)
@pytest.mark.parametrize("heads, k, d", ((2, 24, 8), (2, 16, 16), (2, 40, 16)))
@pytest.mark.parametrize("name", ("class-edges", "class-edges^T"))
def test_the_load_width_decides_no_bit(name, heads, k, d, kind):
    mat = _zoo()[name]
    A = _open(mat)
    Bt, Q, K, V, dO = _operands(mat, heads, k, d, kind, seed=4200 + k)
    for t, w in ((Q, k), (K, k), (V, d), (dO, d)):  # the 16-byte path: attention_vec's and attention_bwd_vec's rule in 2-byte elements
        assert t.data_ptr() % 16 == 0 and t.is_contiguous() and (heads * w * 2) % 16 == 0 and (w * 2) % 16 == 0
    vec = _lowp(A, mat, Q, K, V, dO, 0.6, 2, Bt)
    _all_same(vec, _rounded_fp32(A, mat, Q, K, V, dO, 0.6, 2, Bt), kind, (name, k, kind, "16-byte loads"))
    shifted = tuple(_shifted(t) for t in (Q, K, V, dO, Bt))
    assert all(t.data_ptr() % 16 == 2 for t in shifted[:4])
    odd = tuple(_odd_ld(t) for t in (Q, K, V, dO, Bt))
    for what, (q, k_, v, do, b) in (("one element into a buffer", shifted), ("odd leading dimensions", odd),
                                    ("only dO off the boundary", (Q, K, V, shifted[3], Bt)), ("only K off the boundary", (Q, shifted[1], V, dO, Bt))):
        _all_equal(_lowp(A, mat, q, k_, v, do, 0.6, 2, b), vec, (name, k, kind, what))
    _close(A)


# ---- 5. a head of the packed call is the one-head call with its absolute head ------------------------------------------------------
def _head_by_head(A, mat, heads, k, d, kind, seed, p, head0):
    Bt, Q, K, V, dO = _operands(mat, heads, k, d, kind, seed)
    packed = [_words(t) for t in _lowp(A, mat, Q, K, V, dO, p, head0, Bt)[:5]]
    for h in range(heads):
        s = slice(h, h + 1)
        one = _lowp(A, mat, Q[:, s], K[:, s], V[:, s], dO[:, s], p, head0 + h, Bt[:, s])
        for o, pk, what in zip(one[:5], packed, NAMES):
            assert np.array_equal(_words(o)[:, 0], pk[:, h]), (mat.name, kind, heads, "head", h, what)


@pytest.mark.parametrize("kind", L.KINDS)
@pytest.mark.parametrize("name", ("class-edges", "class-edges^T"))
def test_three_heads_on_the_class_edges_are_three_one_head_calls(name, kind):
    mat = _zoo()[name]
    A = _open(mat)
    _head_by_head(A, mat, 3, 16, 8, kind, 4300, 0.6, 2)
    _head_by_head(A, mat, 3, 12, 65, kind, 4301, 0.1, 0)
    _close(A)


@pytest.mark.parametrize("kind", L.KINDS)
@pytest.mark.parametrize("lines, per_group", ((90113, 3), (262145, 8)), ids=("groups-3-3-2", "one-group"))
def test_eight_heads_in_head_groups_are_eight_one_head_calls(lines, per_group, kind):
    """tests/test_gpu_attention_edges.py's two line counts; the matrices are square, so both kernels see these head groups"""
    assert E.heads_per_group(lines, 8) == per_group
    mat = E.many_lines(lines)
    assert mat.n == lines
    A = _open(mat)
    _head_by_head(A, mat, 8, 16, 1, kind, 4310, 0.6, 2)
    _close(A)


# ---- 6. the mask is the public one ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", L.KINDS)
@pytest.mark.parametrize("heads, k, d, head0", ((3, 3, 5, 2), (2, 16, 16, 0)))
def test_the_mask_is_the_one_dropout_mask_writes(heads, k, d, head0, kind):
    mat = _zoo()["dealt"]
    lens = np.diff(mat.row_ptr)
    assert (lens == 16).all()
    rows, cols = DR.rows_cols(mat)
    rng = np.random.default_rng([4400, heads, k])
    Vn = rng.integers(1, 8, size=(mat.n, heads, d)) * rng.choice((-1, 1), size=(mat.n, heads, d))
    A = _open(mat)
    Q = torch.zeros((mat.m, heads, k), dtype=TDT[kind], device=DEV)
    K = _draw(rng, (mat.n, heads, k), kind)
    V = torch.from_numpy(Vn.astype(np.float32)).to(DEV).to(TDT[kind])
    assert np.array_equal(V.float().cpu().numpy(), Vn)
    O = _poison((mat.m, heads, d), kind)
    assert A.dropoutMhaLowp(Q, K, V, O, 0.5, SEED, OFFSET, head0) == 0, _capi.last_error()
    mask = torch.full((mat.nnz, heads), 0xAB, dtype=torch.uint8, device=DEV)
    assert A.dropoutMask(mask, 0.5, SEED, OFFSET, head0) == 0, _capi.last_error()
    torch.cuda.synchronize()
    _close(A)
    keep = mask.cpu().numpy().astype(np.int64)
    assert set(np.unique(keep)) == {0, 1} and np.array_equal(keep, DR.mask(mat.nnz, heads, 0.5, SEED, OFFSET, head0))
    acc = np.zeros((mat.m, heads, d), dtype=np.int64)
    np.add.at(acc, rows, keep[:, :, None] * Vn[cols])
    assert np.abs(acc).max() <= 112
    want = (acc.astype(np.float32) * np.float32(0.125)).astype(np.float32)      # exact: an integer of 7 bits times 2^-3
    assert np.array_equal(L.widen(L.to_words(want, kind), kind), want)          # ... which the operand type holds
    got = L.widen(_words(O), kind)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (kind, heads, k, d, int((got != want).sum()))
    flipped = keep.copy()
    flipped[0, 0] ^= 1                                                          # (one wrong bit shows: |V| >= 1)
    acc2 = np.zeros_like(acc)
    np.add.at(acc2, rows, flipped[:, :, None] * Vn[cols])
    assert not np.array_equal(acc2, acc)


# ---- 7. the float64 reference ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", L.KINDS)
@pytest.mark.parametrize("p", (0.1, 0.6))
@pytest.mark.parametrize("which", ("class-edges", "random"))
def test_the_float64_reference_forward_and_every_gradient(which, p, kind):
    """|got - ref| <= tests/dropout_reference.py's fp32 allowance (on the widened operands: what the kernels compute before they
    store) + one rounding to the operand type.  The worst |error| / allowance of every output is printed"""
    mat = _zoo()["class-edges"] if which == "class-edges" else EB.random_matrix()
    heads, k, d = EB.F_HEADS, EB.F_K, EB.F_D
    words, scale = LB.f64_case(mat, kind, heads, k, d)
    Bt, Q, K, V, dO = (_of_words(w, kind) for w in words)
    A = _open(mat)
    got = _lowp(A, mat, Q, K, V, dO, p, 2, Bt, scale=scale, seed=4500, offset=7)
    _close(A)
    Bf, Qf, Kf, Vf, dOf = (L.widen(w, kind) for w in words)
    keep, cd = DR.mask(mat.nnz, heads, p, 4500, 7, 2), DR.cd_of(p, np.float32)
    rho, want, allow = DR.allowances(mat, scale, Bf, Qf, Kf, Vf, dOf, keep, cd, np.float32, STAGES)
    assert STAGES * rho <= FIRST_ORDER, (mat.name, rho)
    worst = {}
    for g, w, al, n in zip(got[:5], want, allow, NAMES):
        worst[n] = DR.compare(L.widen(_words(g), kind), w, al + L.round_allowance(w, kind), n)
        print(f"{mat.name} {kind} p={p} {n}: rho {rho:.3e}, worst |error| / allowance {worst[n]:.3f}")
    assert all(v <= 1.0 for v in worst.values()), worst


# ---- 8. contract edges ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", L.KINDS)
def test_a_subset_of_the_outputs_has_the_words_of_the_whole_call(kind):
    mat = _zoo()["class-edges"]
    heads, k, d = 3, 12, 5
    Bt, Q, K, V, dO = _operands(mat, heads, k, d, kind, seed=4600)
    bare = _open(mat, transpose=False)  # O, dQ and dB need neither the companion nor the workspace
    alone = {w: _lowp(bare, mat, Q, K, V, dO, 0.6, 2, Bt, want=w) for w in ("O", "Q", "B")}
    assert bare.info().transpose_built == 0
    _close(bare)
    A = _open(mat)
    full = _lowp(A, mat, Q, K, V, dO, 0.6, 2, Bt)
    again, other = _lowp(A, mat, Q, K, V, dO, 0.6, 2, Bt), _lowp(A, mat, Q, K, V, dO, 0.6, 2, Bt, offset=OFFSET + 1)
    alone.update({w: _lowp(A, mat, Q, K, V, dO, 0.6, 2, Bt, want=w) for w in ("K", "V")})
    _close(A)
    for i, w in enumerate("OQKVB"):
        assert [t is not None for t in alone[w][:5]] == [j == i for j in range(5)]
        assert np.array_equal(_words(alone[w][i]), _words(full[i])), (kind, NAMES[i], "alone")
        assert np.array_equal(_words(again[i]), _words(full[i])) and not np.array_equal(_words(other[i]), _words(full[i])), NAMES[i]


@pytest.mark.parametrize("kind", L.KINDS)
def test_only_the_declared_elements_are_read_and_written(kind):
    heads, k, d = 3, 16, 5
    for name in ("half-empty", "class-edges"):
        mat = _zoo()[name]
        A = _open(mat, val=np.full(mat.nnz, np.nan))
        Bt, Q, K, V, dO = _operands(mat, heads, k, d, kind, seed=4700)
        want = _lowp(A, mat, Q, K, V, dO, 0.6, 2, Bt)
        assert not any(L.is_nan(_words(t), kind).any() for t in want[:5])
        info0, bytes0 = bytes(A.info()), A.info().device_bytes
        (bw, Bv), (_, Qv), (_, Kv), (_, Vv), (_, dOv) = _padded(Bt, 3), _padded(Q, 8), _padded(K, 3), _padded(V, 2), _padded(dO, 5)
        kept = bw.clone()
        sizes = ((mat.m, d), (mat.m, k), (mat.n, k), (mat.n, d))
        bufs = [_guarded(r, heads * w, kind) for r, w in sizes] + [_guarded(mat.nnz, heads, kind)]
        views = [b[1].unflatten(1, (heads, w)) for b, (_, w) in zip(bufs[:4], sizes)] + [bufs[4][1]]  # dB: a slice of a wider tensor
        assert A.dropoutMhaLowp(Qv, Kv, Vv, views[0], 0.6, SEED, OFFSET, 2, B=Bv, scale=SCALE) == 0, _capi.last_error()
        assert A.dropoutMhaLowpBackward(Qv, Kv, Vv, dOv, 0.6, SEED, OFFSET, 2, dQ=views[1], dK=views[2], dV=views[3], work=_work(mat, heads),
                                        B=Bv, scale=SCALE, dB=views[4]) == 0, _capi.last_error()
        torch.cuda.synchronize()
        rws = (mat.m, mat.m, mat.n, mat.n, mat.nnz)
        for (b, _, ld), w, width, r, what in zip(bufs, want, (heads * d, heads * k, heads * k, heads * d, heads), rws, NAMES):
            body = _guard_intact(b, r, width, ld, what)
            assert not L.is_nan(body, kind).any(), "padding was read"
            assert np.array_equal(body, _words(w).reshape(r, -1)), (name, kind, what)
        assert np.array_equal(_words(bw), _words(kept))  # B is only read
        assert bytes(A.info()) == info0 and A.info().device_bytes == bytes0
        _close(A)


@pytest.mark.parametrize("kind", L.KINDS)
def test_degenerate_shapes_and_the_error_order(kind):
    ot = _capi.BF16 if kind == "bf16" else _capi.F16
    mat = _zoo()["half-empty"]
    A = _open(mat, transpose=False)
    Bt, Q, K, V, dO = _operands(mat, 3, 4, 6, kind, seed=4800)
    O, dQ, dK, dB = _poison((mat.m, 3, 6), kind), _poison(Q.shape, kind), _poison(K.shape, kind), _poison(Bt.shape, kind)
    work = _work(mat, 3)
    INV, TYPE = _capi.INVALID_ARGUMENT, _capi.UNSUPPORTED_VALUE_TYPE

    def fwd(t=ot, heads=3, scale=1.0, ldb=3, q=Q, d=6, p=0.5, head0=0):
        return A.dropout_mha_lowp_ptr(t, heads, scale, Bt, ldb, q, 12, K, 12, 4, V, 18, d, O, 18, p, 1, 2, head0)

    def bwd(t=ot, heads=3, scale=1.0, ldb=3, q=Q, dq=dQ, dk=None, lddb=3, wk=None, p=0.5, head0=0):
        return A.dropout_mha_lowp_backward_ptr(t, heads, scale, Bt, ldb, q, 12, K, 12, 4, V, 18, 6, dO, 18, dq, 12, dk, 12, None, 18, wk, dB,
                                               lddb, p, 1, 2, head0)
    for call in (fwd, bwd):
        assert call(heads=0) == 0, _capi.last_error()
        for bad in (_capi.F64, _capi.F32, 4, -1):
            assert call(t=bad) == TYPE and call(t=bad, p=1.0) == TYPE and call(t=bad, heads=-1, scale=float("nan")) == TYPE
        for bad in (dict(p=float("nan")), dict(p=-0.5), dict(p=1.0), dict(head0=-1), dict(head0=2 ** 31 - 2), dict(heads=-1),
                    dict(scale=float("inf")), dict(ldb=2), dict(q=None), dict(p=1.0, ldb=2), dict(p=1.0, q=None)):
            assert call(**bad) == INV, bad
    assert fwd(d=0) == 0 and bwd(lddb=2) == INV and bwd(dq=None, dk=dK, wk=None) == INV  # dK without the workspace
    assert A.dropoutMhaLowpBackward(Q, K, V, dO, 0.5, 1, dK=dK, work=work, B=Bt) == INV  # dK without a companion, under this call's name
    assert "transposed companion" in _capi.last_error() and "csr5hip_dropout_mha_lowp_backward:" in _capi.last_error()
    torch.cuda.synchronize()
    assert all((_words(t) == POISON_WORD).all() for t in (O, dQ, dK, dB)) and bool(torch.isnan(work).all())
    assert A.buildTranspose() == 0, _capi.last_error()
    # k = 0: every score is the bias alone -- the words of Q = +0 at k = 4 (qk = +0 either way); dQ and dK have no element
    Q0, K0 = (torch.zeros((r, 3, 0), dtype=TDT[kind], device=DEV) for r in (mat.m, mat.n))
    zeroed = _lowp(A, mat, torch.zeros_like(Q), K, V, dO, 0.5, 2, Bt, scale=0.7, want="OVB")
    O0, dV0, dB0 = _poison(O.shape, kind), _poison(V.shape, kind), _poison(Bt.shape, kind)
    assert A.dropoutMhaLowp(Q0, K0, V, O0, 0.5, SEED, OFFSET, 2, B=Bt, scale=0.7) == 0, _capi.last_error()
    assert A.dropoutMhaLowpBackward(Q0, K0, V, dO, 0.5, SEED, OFFSET, 2, dV=dV0, work=work, B=Bt, scale=0.7, dB=dB0) == 0, _capi.last_error()
    torch.cuda.synchronize()
    for g, w in ((O0, zeroed[0]), (dV0, zeroed[3]), (dB0, zeroed[4])):
        assert np.array_equal(_words(g), _words(w))
    # d = 0: dB is the score gradient of an empty product, a zero wherever p is finite
    V0, dO0 = (torch.zeros((r, 3, 0), dtype=TDT[kind], device=DEV) for r in (mat.n, mat.m))
    dB0 = _poison(Bt.shape, kind)
    assert A.dropoutMhaLowpBackward(Q, K, V0, dO0, 0.5, 1, B=Bt, dB=dB0) == 0, _capi.last_error()
    torch.cuda.synchronize()
    assert not (_words(dB0) & 0x7FFF).any()
    assert A.dropoutMhaLowpBackward(Q, K, V, dO, 0.5, 1, B=Bt) == 0, _capi.last_error()  # nothing wanted: a successful no-op
    _close(A)
    none = zoo.empty_matrix()  # nnz = 0 with m > 0: the word 0x0000 in every wanted output, no element of dB
    assert none.m > 0 and none.nnz == 0
    A = _open(none)
    Bt, Q, K, V, dO = _operands(none, 3, 4, 6, kind, seed=4801)
    for t in _lowp(A, none, Q, K, V, dO, 0.5, 0, Bt)[:5]:
        assert not _words(t).any()
    _close(A)
    one = type(none)(1, 5, np.array([0, 3], dtype=np.int32), np.array([0, 2, 4], dtype=np.int32), np.ones(3), "one-row")
    A32, A = _open(one), _open(one, np.float64)
    Bt, Q, K, V, dO = _operands(one, 3, 4, 6, kind, seed=4802)
    _all_same(_lowp(A, one, Q, K, V, dO, 0.6, 2, Bt), _rounded_fp32(A32, one, Q, K, V, dO, 0.6, 2, Bt), kind, ("one row", kind))
    _close(A32)
    _close(A)


@pytest.mark.parametrize("kind", L.KINDS)
def test_the_calls_are_captured_on_their_first_use_and_a_replay_repeats_the_mask(kind):
    mat = _zoo()["half-empty"]
    A = _open(mat)  # (a fresh handle with its companion: the captured calls are the first of their kind it sees)
    Bt, Q, K, V, dO = _operands(mat, 3, 16, 6, kind, seed=4900)
    outs = [_poison(s, kind) for s in ((mat.m, 3, 6), Q.shape, K.shape, V.shape, Bt.shape)]
    work = _work(mat, 3)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert A.setStream(side) == 0
    held = A.info().device_bytes
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        assert A.dropoutMhaLowp(Q, K, V, outs[0], 0.6, SEED, OFFSET, 2, B=Bt, scale=SCALE) == 0, _capi.last_error()
        assert A.dropoutMhaLowpBackward(Q, K, V, dO, 0.6, SEED, OFFSET, 2, dQ=outs[1], dK=outs[2], dV=outs[3], work=work, B=Bt, scale=SCALE,
                                        dB=outs[4]) == 0, _capi.last_error()
    assert A.info().device_bytes == held
    torch.cuda.synchronize()
    new = _operands(mat, 3, 16, 6, kind, seed=4901)
    for t, n in zip((Bt, Q, K, V, dO), new):
        assert not torch.equal(t, n)
        t.copy_(n)  # changed in place: the graph reads the same addresses
    replays = []
    for _ in range(2):
        for o in outs:
            o.view(torch.int16).fill_(POISON_WORD)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        replays.append([_words(o).copy() for o in outs])
    del graph
    assert A.setStream(None) == 0
    eager = _lowp(A, mat, new[1], new[2], new[3], new[4], 0.6, 2, new[0])
    for r in replays:  # (seed and offset are by-value arguments: a replay repeats the mask)
        for g, e, what in zip(r, eager[:5], NAMES):
            assert not (g == POISON_WORD).any() and np.array_equal(g, _words(e)), (kind, what)
    _close(A)


@pytest.mark.parametrize("kind", L.KINDS)
@pytest.mark.parametrize("history", ("loaded", "reconverted"))
def test_a_loaded_and_a_reconverted_handle_give_the_fresh_handles_words(history, kind, tmp_path):
    mat = _zoo()["class-edges"]
    val = HH.values(mat, 4950, np.float32)
    fresh = _open(mat, np.float32, val=val)
    old, _ = (HH._loaded if history == "loaded" else HH._reconverted)(mat, val, np.float32, tmp_path)
    Bt, Q, K, V, dO = _operands(mat, 3, 3, 5, kind, seed=4951)
    res = []
    for A in (fresh, old):
        if not A.info().transpose_built:
            assert A.buildTranspose() == 0, _capi.last_error()
        res.append(_lowp(A, mat, Q, K, V, dO, 0.6, 2, Bt))
    _all_equal(res[1], res[0], (history, kind))
    _close(fresh)
    _close(old)


# ---- 9. autograd --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", L.KINDS)
@pytest.mark.parametrize("handle_dtype", (np.float32, np.float64), ids=("fp32-handle", "fp64-handle"))
def test_autograd_is_one_call_each_way_on_both_handle_dtypes(handle_dtype, kind):
    mat = _zoo()["class-edges"]
    A = _open(mat, handle_dtype, transpose=False)
    heads, k, d = 3, 8, 16
    Bt, Q, K, V, dO = _operands(mat, heads, k, d, kind, seed=5000)
    drop = dict(p=0.6, seed=SEED, offset=OFFSET)
    calls = []
    for name in ("dropoutMhaLowp", "dropoutMhaLowpBackward", "dropoutMha", "dropoutMhaBackward", "mhaEdgeBiasBackward", "mhaLowp", "buildTranspose"):
        _counted(A, name, calls)
    # only Q needs a gradient, the bias none: no companion, no workspace, no dB
    q = Q.clone().requires_grad_(True)
    seen = []
    real = A.dropoutMhaLowpBackward
    A.dropoutMhaLowpBackward = lambda *a, **kw: seen.append(kw) or real(*a, **kw)
    autograd.dropout_attention(A, q, K, V, scale=SCALE, bias=Bt, **drop).backward(dO)
    torch.cuda.synchronize()
    assert calls == ["dropoutMhaLowp", "dropoutMhaLowpBackward"] and A.info().transpose_built == 0
    assert seen[0]["dB"] is None and seen[0]["work"] is None and seen[0]["dK"] is None and seen[0]["dV"] is None
    A.dropoutMhaLowpBackward = real
    q_, k_, v, b_ = (t.clone().requires_grad_(True) for t in (Q, K, V, Bt))
    del calls[:]
    out = autograd.dropout_attention(A, q_, k_, v, scale=SCALE, bias=b_, **drop)
    out.backward(dO)
    torch.cuda.synchronize()
    assert calls == ["dropoutMhaLowp", "buildTranspose", "dropoutMhaLowpBackward"]
    direct = _lowp(A, mat, Q, K, V, dO, 0.6, 0, Bt)
    for g, w, what in zip((out, q_.grad, k_.grad, v.grad, b_.grad), direct[:5], NAMES):
        assert g.dtype == TDT[kind] and g.shape == w.shape and np.array_equal(_words(g), _words(w)), (kind, what)
    assert np.array_equal(_words(q.grad), _words(direct[1]))
    # K and V as one tensor: autograd adds the two gradients
    kv = K.clone().requires_grad_(True)
    dOk = dO[:, :, :k].contiguous()
    Kd = _lowp(A, mat, Q, K, K, dOk, 0.6, 0, Bt)
    autograd.dropout_attention(A, Q, kv, kv, scale=SCALE, bias=Bt, **drop).backward(dOk)
    torch.cuda.synchronize()
    assert np.array_equal(_words(kv.grad), _words(Kd[2] + Kd[3]))
    # evaluation is the undropped 16-bit call; nothing runs in backward when nothing needs a gradient
    del calls[:]
    ev = autograd.dropout_attention(A, Q, K, V, scale=SCALE, bias=Bt, training=False, **drop)
    O = _poison(ev.shape, kind)
    assert A.mhaLowp(Q, K, V, O, B=Bt, scale=SCALE) == 0
    torch.cuda.synchronize()
    assert calls == ["mhaLowp", "mhaLowp"] and np.array_equal(_words(ev), _words(O))
    del calls[:]
    assert not autograd.dropout_attention(A, Q, K, V, scale=SCALE, bias=Bt, **drop).requires_grad
    other = torch.ones((), dtype=TDT[kind], device=DEV, requires_grad=True)
    (autograd.dropout_attention(A, Q, K, V, scale=SCALE, bias=Bt, **drop).float().sum() * other.float()).backward()
    torch.cuda.synchronize()
    assert calls == ["dropoutMhaLowp", "dropoutMhaLowp"]
    _close(A)
