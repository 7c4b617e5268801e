"""``attention`` / ``attentionBackward`` / ``mha`` / ``mhaBackward`` on the GPU where the kernels decide things, on the patterns of
tests/attention_edges.py.  The other attention tests run on the matrix zoo of the SpMV work, whose line lengths (at most 14, 16,
40, 64, 1 024, 3 000 and beyond) sit on no class edge, whose hubs all lie in workgroup 0, and whose line counts give head groups
of one or two heads only.

``class_edges()``: 769 x 4 608, row i has (0, 1, 15, 16, 17, 63, 64, 65, 511, 512)[i % 10] entries, so every wavefront of every
workgroup holds lines on both sides of 16 | 17 (lanes -> wavefront), 63 | 64 | 65 (the slot wrap-around j mod 64) and the
wavefront class' last lengths 511 and 512 (a full share of LDS), except

    row   entries  why
    3       513    a hub just above the wavefront class (workgroup 0, wavefront 0)
    60    2 048    staged = rl <= AT_STAGE at equality; the staged columns reused by the later heads at exactly 2 048
    61    2 049    its neighbour in the same wavefront: the chunk loop with a last chunk of ONE entry
    130   4 096    a whole number of chunks, in another wavefront
    256   4 097    the first row of workgroup 1: two full chunks and one entry
    511     513    the last row of workgroup 1
    700   2 049    a hub in workgroup 2
    768     600    the only row of the last workgroup

so hr = blockIdx.x * AT_BLOCK + hub_row[i] runs with blockIdx.x = 0 .. 3, every workgroup holds wavefront-class rows and hubs
together (the barrier that hands the wavefronts' shares of LDS to the hub rows), and hubs lie at j mod 256 = 1, 0 and in between.
Its transpose gives the column kernel the same line lengths; ``dealt()`` does so with 16 entries in every row.

A  the derived bounds of tests/test_gpu_attention_autograd.py and tests/test_gpu_attention_backward.py against the float64 torch
   reference, at widths whose second column block has width 1 (17, 65, 257; 257 opens a second group of four blocks) and with
   fp32 k = 7 | 9 on either side of the 16-byte loads; ``mha`` / ``mhaBackward`` per head against that reference too.  The
   preconditions rho <= 2**-6 and STAGES_B rho_b <= 2**-6 were evaluated beforehand in numpy: the largest STAGES_B rho_b of the
   cases below is 4.1e-3 (fp32, class_edges(), (3, 257)), of D 5.3e-4, so no width had to be reduced.
B  the forward bit for bit, any summation order: integer V, every unmasked weight exactly 1 (tests/attention_edges.py).  In fp32
   the bound of A cannot see ONE lost entry of a row of 4 097 (it carries 2.4e-4 of the row, the allowance is as large); this can.
C  the backward bit for bit on ``dealt()``: p = 1/16 exactly, integer operands.
D  head groups of 3 + 3 + 2 heads (90 113 lines) and of all heads (262 145 lines) on ``many_lines(m)``, whose only hub is the one
   line of the last of 353 (1 025) workgroups: every head bit for bit the single-head call, two heads against the reference.
E  rows 61, 256, 511 and 768 alone in a one-row matrix at another sigma: the bits they have inside the matrix.

No tolerance is introduced here: A and D use the allowances derived in those two files, B, C and E compare bits under conditions
that the tests assert on their own data."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from benchmark_spmv_using_csr5_amd import _capi  # noqa: E402
from benchmark_spmv_using_csr5_amd import handle as H  # noqa: E402
from benchmark_spmv_using_csr5_amd import matrices as M  # noqa: E402
from tests import attention_edges as E  # noqa: E402
from tests import sddmm_reference as S  # noqa: E402
from tests.test_gpu_attention_autograd import _within  # noqa: E402
from tests.test_gpu_attention_backward import _backward, _check, _open, _operands, transpose  # noqa: E402
from tests.test_gpu_exact_reference import DEV, Path, _bits, _close  # noqa: E402
from tests.test_gpu_fused_attention import RHO_MAX, _attend, _bound  # noqa: E402
from tests.test_gpu_mha import _mha, _mha_backward, _per_head, _per_head_backward, _same  # noqa: E402
from tests.test_gpu_mha import _operands as _packed_operands  # noqa: E402

AUTO = H.ANONYMOUSLIB_AUTO_TUNED_SIGMA
KD_A = ((8, 16), (7, 17), (9, 65), (3, 257))
HKD_A = ((3, 8, 16), (3, 3, 5))
# (name, sigma, padded leading dimensions)
CONFIGS = (("default", AUTO, False), ("sigma7-padded", 7, True), ("sigma32", 32, False))
ALONE = (61, 256, 511, 768)


def _tdt(dtype):
    return torch.float64 if dtype == np.float64 else torch.float32


def _dt(dtype):
    return "fp64" if dtype == np.float64 else "fp32"


@functools.lru_cache(maxsize=None)
def _mat(name):
    if name.endswith("^T"):
        return transpose(_mat(name[:-2]))
    if name.startswith("many-lines-"):
        return E.many_lines(int(name[len("many-lines-"):]))
    return {"class-edges": E.class_edges, "dealt": E.dealt}[name]()


def _path(sigma):
    return Path("edges" if sigma == AUTO else f"sigma{sigma}", sigma, H.SPMV_FUSED)


def _dev(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays)


def _padded(t, extra):
    """t as the leading columns of a wider allocation (the leading dimension grows by `extra`); packed tensors stay packed"""
    if t.shape[-1] == 0 or extra == 0:
        return t
    flat = t.reshape(t.shape[0], -1)
    wide = torch.full((flat.shape[0], flat.shape[1] + extra), -777.25, dtype=t.dtype, device=t.device)
    wide[:, :flat.shape[1]] = flat
    view = wide[:, :flat.shape[1]]
    return view if t.dim() == 2 else view.unflatten(1, tuple(t.shape[1:]))


def _empty_rows(mat):
    return torch.from_numpy(np.diff(mat.row_ptr) == 0).to(DEV)


# ---- A. the derived bounds at the edges ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
@pytest.mark.parametrize("kd", KD_A, ids=lambda kd: f"k{kd[0]}-d{kd[1]}")
@pytest.mark.parametrize("name", ("class-edges", "class-edges^T"))
def test_forward_and_backward_match_the_float64_reference_at_the_edges(name, kd, dtype):
    (k, d), mat = kd, _mat(name)
    Q, K, V, dO = _operands(mat, k, d, dtype, seed=500)
    A = _open(mat, dtype)
    O = _attend(A, Q, K, V)
    got = _backward(A, mat, Q, K, V, dO)
    _close(A)
    what = f"{name} {_dt(dtype)} k={k} d={d}"
    want, rho, a_out = _bound(mat, Q, K, V, dtype)
    print(f"{what}: rho {rho:.3e}")
    assert rho <= RHO_MAX, (what, rho)
    _within(O, want, a_out, what + " O")
    assert not _bits(O[_empty_rows(mat)].cpu().numpy()).any(), what  # rows without entries: exactly +0
    _check(mat, got, Q, K, V, dO, dtype, what)  # (asserts STAGES_B rho_b <= 2**-6 first)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
@pytest.mark.parametrize("hkd", HKD_A, ids=lambda s: f"h{s[0]}-k{s[1]}-d{s[2]}")
@pytest.mark.parametrize("name", ("class-edges", "class-edges^T"))
def test_every_head_matches_the_float64_reference_at_the_edges(name, hkd, dtype):
    """``mhaBackward``'s dQ, dK and dV against a reference that shares nothing with the single-head backward"""
    (heads, k, d), mat = hkd, _mat(name)
    Q, K, V, dO = _packed_operands(mat, heads, k, d, dtype, seed=510)
    Q = Q / (k ** 0.5)  # the usual scaling of attention, as tests/test_gpu_attention_backward.py
    A = _open(mat, dtype)
    O = _mha(A, Q, K, V)
    got = _mha_backward(A, mat, Q, K, V, dO)
    _close(A)
    assert not any(bool(torch.isnan(t).any()) for t in [O] + got), "an element was not written"
    for h in range(heads):
        q, k_, v, do = (t[:, h].contiguous() for t in (Q, K, V, dO))
        what = f"{name} {_dt(dtype)} heads={heads} k={k} d={d} head {h}"
        want, rho, a_out = _bound(mat, q, k_, v, dtype)
        assert rho <= RHO_MAX, (what, rho)
        _within(O[:, h], want, a_out, what + " O")
        _check(mat, [g[:, h] for g in got], q, k_, v, do, dtype, what)


# ---- B. the forward, bit for bit -----------------------------------------------------------------------------------------------
FORWARD_CASES = (("k0", 0, 17, 1), ("q0", 8, 5, 1), ("masked", 5, 65, 2), ("masked", 8, 16, 2))


def _forward_conditions(mat, variant, unmasked, worst, what):
    """the conditions of tests/attention_edges.py on this test's own data"""
    assert worst < E.EXACT_LIMIT, (what, worst)  # every partial sum in every order is an integer below 2**24
    if variant == "masked":
        mixed, all_masked = E.mask_conditions(mat, unmasked)
        assert mixed, what + ": a row of 17 or more entries is all masked or all unmasked"
        assert 0 < all_masked < 0.1, (what, all_masked)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
@pytest.mark.parametrize("case", FORWARD_CASES, ids=lambda c: f"{c[0]}-k{c[1]}-d{c[2]}")
def test_forward_has_exactly_the_bits_of_the_definition(case, dtype):
    (variant, k, d, seed), mat = case, _mat("class-edges")
    Q, K, V, unmasked = E.forward_operands(mat, variant, k, d, dtype, seed)
    want, worst = E.exact_forward(mat, V, unmasked, dtype)
    _forward_conditions(mat, variant, unmasked, worst, f"{variant} {_dt(dtype)}")
    for cname, sigma, pad in CONFIGS:
        q, k_, v = (_padded(t, e if pad else 0) for t, e in zip(_dev(Q, K, V), (3, 1, 2)))
        O = _padded(torch.full((mat.m, d), float("nan"), dtype=_tdt(dtype), device=DEV), 3 if pad else 0)
        A = _open(mat, dtype, _path(sigma), companion=False)
        assert A.attention(q, k_, v, O) == 0, _capi.last_error()
        torch.cuda.synchronize()
        _close(A)
        got = O.cpu().numpy()
        wrong = np.flatnonzero(~np.array([E.same_bits(g, w) for g, w in zip(got, want)]))
        assert wrong.size == 0, (variant, _dt(dtype), cname, "rows", wrong[:8].tolist(), np.diff(mat.row_ptr)[wrong[:8]].tolist())


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
@pytest.mark.parametrize("case", FORWARD_CASES[1:], ids=lambda c: f"{c[0]}-k{c[1]}-d{c[2]}")
def test_every_head_of_mha_has_exactly_the_bits_of_the_definition(case, dtype):
    """heads = 3 with values and a mask of their own each"""
    (variant, k, d, seed), mat, heads = case, _mat("class-edges"), 3
    Q, K, V, unmasked = E.forward_operands(mat, variant, k, d, dtype, seed, heads=heads)
    want = []
    for h in range(heads):
        o, worst = E.exact_forward(mat, V[:, h], unmasked[h], dtype)
        _forward_conditions(mat, variant, unmasked[h], worst, f"{variant} {_dt(dtype)} head {h}")
        want.append(o)
    if variant == "masked":
        assert not np.array_equal(unmasked[0], unmasked[1]) and not np.array_equal(unmasked[1], unmasked[2])
    for cname, sigma, pad in CONFIGS:
        q, k_, v = (_padded(t, e if pad else 0) for t, e in zip(_dev(Q, K, V), (3, 1, 2)))
        O = _padded(torch.full((mat.m, heads, d), float("nan"), dtype=_tdt(dtype), device=DEV), 3 if pad else 0)
        A = _open(mat, dtype, _path(sigma), companion=False)
        assert A.mha(q, k_, v, O) == 0, _capi.last_error()
        torch.cuda.synchronize()
        _close(A)
        got = O.cpu().numpy()
        for h in range(heads):
            wrong = np.flatnonzero(~np.array([E.same_bits(g, w) for g, w in zip(got[:, h], want[h])]))
            assert wrong.size == 0, (variant, _dt(dtype), cname, "head", h, "rows", wrong[:8].tolist())


# ---- C. the backward, bit for bit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
@pytest.mark.parametrize("kd", ((8, 5), (3, 17)), ids=lambda kd: f"k{kd[0]}-d{kd[1]}")
@pytest.mark.parametrize("zero", ("Q", "K"), ids=lambda z: f"{z}-zero")
def test_backward_has_exactly_the_bits_of_the_definition(zero, kd, dtype):
    """Q = 0 makes dQ the non-trivial output (dK = +0), K = 0 makes dK (dQ = +0); dV is non-trivial in both.  The columns of
    ``dealt()`` have the edge lengths: the column kernel's classes; ``mhaBackward`` with three heads of their own values too."""
    (k, d), mat = kd, _mat("dealt")
    assert (np.diff(mat.row_ptr) == 16).all()
    A = _open(mat, dtype)
    ops = E.backward_operands(mat, zero, k, d, dtype, seed=3)
    want = E.exact_backward(mat, *ops, dtype)
    assert want.worst < E.EXACT_LIMIT, want.worst
    assert (want.dK if zero == "K" else want.dQ).any() and want.dV.any()
    Q, K, V, dO = _dev(*ops)
    for g, w, what in zip(_backward(A, mat, Q, K, V, dO), (want.dQ, want.dK, want.dV), ("dQ", "dK", "dV")):
        wrong = np.flatnonzero((_bits(g.cpu().numpy()) != _bits(w)).any(axis=1))
        assert wrong.size == 0, (zero, k, d, _dt(dtype), what, "lines", wrong[:8].tolist())
    heads = 3
    ops = E.backward_operands(mat, zero, k, d, dtype, seed=4, heads=heads)
    Q, K, V, dO = _dev(*ops)
    got = _mha_backward(A, mat, Q, K, V, dO)
    _close(A)
    for h in range(heads):
        want = E.exact_backward(mat, *(t[:, h] for t in ops), dtype)
        assert want.worst < E.EXACT_LIMIT, want.worst
        for g, w, what in zip(got, (want.dQ, want.dK, want.dV), ("dQ", "dK", "dV")):
            wrong = np.flatnonzero((_bits(g[:, h].cpu().numpy()) != _bits(w)).any(axis=1))
            assert wrong.size == 0, (zero, k, d, _dt(dtype), "head", h, what, "lines", wrong[:8].tolist())


# ---- D. head groups wider than two ---------------------------------------------------------------------------------------------
# (lines, heads, heads per group by the rule, k, d, dtype): both types at 90 113 lines, one per head count at 262 145
GROUP_CASES = ((90113, 8, 3, 8, 4, np.float32), (90113, 8, 3, 8, 4, np.float64), (262145, 8, 8, 8, 4, np.float32),
               (262145, 5, 5, 3, 5, np.float64), (262145, 3, 3, 8, 4, np.float64))


@pytest.mark.parametrize("side", ("", "^T"), ids=("rows", "transposed"))
@pytest.mark.parametrize("case", GROUP_CASES, ids=lambda c: f"m{c[0]}-h{c[1]}-k{c[3]}-d{c[4]}-{_dt(c[5])}")
def test_head_groups_of_three_and_of_all_heads(case, side):
    """the rule gives 3 + 3 + 2 heads at 90 113 lines and one group of all heads at 262 145; the transposed pattern puts the
    hub of the last workgroup and the wavefront-class line before the column kernel"""
    m, heads, hper, k, d, dtype = case
    mat = _mat(f"many-lines-{m}{side}")
    lens = np.diff(_mat(f"many-lines-{m}").row_ptr)
    assert (m - 1) % E.AT_BLOCK == 0 and lens[m - 1] == 513 and lens[E.middle_row(m)] == 40 and lens.max() == 513
    assert np.sort(lens)[-3] <= 3 and E.middle_row(m) % E.AT_BLOCK == 63
    assert mat.m == mat.n == m and E.heads_per_group(m, heads) == hper  # (both kernels walk m lines)
    Q, K, V, dO = _packed_operands(mat, heads, k, d, dtype, seed=520)
    Q = Q / (k ** 0.5)
    A = _open(mat, dtype)
    O = _mha(A, Q, K, V)
    got = _mha_backward(A, mat, Q, K, V, dO)
    assert not any(bool(torch.isnan(t).any()) for t in [O] + got), "an element was not written"
    assert _same(O, _per_head(A, Q, K, V)), "O"
    for g, w, what in zip(got, _per_head_backward(A, mat, Q, K, V, dO), ("dQ", "dK", "dV")):
        assert _same(g, w), what
    _close(A)
    for h in sorted({hper % heads, heads - 1}):  # the first head of the second group (head 0 where there is one group), the last
        q, k_, v, do = (t[:, h].contiguous() for t in (Q, K, V, dO))
        what = f"{mat.name} {_dt(dtype)} heads={heads} head {h}"
        want, rho, a_out = _bound(mat, q, k_, v, dtype)
        assert rho <= RHO_MAX, (what, rho)
        _within(O[:, h], want, a_out, what + " O")
        _check(mat, [g[:, h] for g in got], q, k_, v, do, dtype, what)


# ---- E. position independence at the edges -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_an_edge_row_alone_gives_the_bits_it_has_inside_the_matrix(dtype):
    """rows 61 (2 049 entries, beside a hub of 2 048), 256 (4 097, first of workgroup 1), 511 (513, last of workgroup 1) and 768
    (600, alone in workgroup 3), each as the one row of a matrix at sigma = 7: the same O and dQ"""
    mat = _mat("class-edges")
    assert [int(np.diff(mat.row_ptr)[r]) for r in ALONE] == [2049, 4097, 513, 600]
    Q, K, V, dO = _operands(mat, 8, 16, dtype, seed=530)
    A = _open(mat, dtype, companion=False)
    O = _attend(A, Q, K, V).cpu().numpy()
    dQ = _backward(A, mat, Q, K, V, dO, want=(True, False, False))[0].cpu().numpy()
    _close(A)
    for r in ALONE:
        a, b = int(mat.row_ptr[r]), int(mat.row_ptr[r + 1])
        one = M.CsrMatrix(1, mat.n, np.array([0, b - a], dtype=np.int32), mat.col[a:b].copy(), np.ones(b - a), f"row{r}")
        A1 = _open(one, dtype, _path(7), companion=False)
        O1 = _attend(A1, Q[r:r + 1].clone(), K, V).cpu().numpy()
        dQ1 = _backward(A1, one, Q[r:r + 1].clone(), K, V, dO[r:r + 1].clone(), want=(True, False, False))[0].cpu().numpy()
        _close(A1)
        assert np.array_equal(_bits(O1[0]), _bits(O[r])), (r, "O")
        assert np.array_equal(_bits(dQ1[0]), _bits(dQ[r])), (r, "dQ")
