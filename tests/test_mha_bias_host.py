"""csr5hip_mha_biased / csr5hip_mha_biased_backward on the host side (no GPU): the C ABI symbols and their declarations, the C++
class members, the return codes and their order, the Python argument checks of scale, slopes and dS,
``autograd.multihead_attention``'s new arguments, the host emulation of the kernel sources under the address and
undefined-behaviour sanitizers (stand-alone programs), and the augmented operands of tests/mha_bias_reference.py.

For tests/test_gpu_mha_bias_edges.py: the padded augmentation step by step in exact rationals (the sign of zero included), the
wrong scores its expectations must reject, the transcription of the 16-byte-load rules against the headers' functions, the
structure its path test asserts, and the first-order condition of its float64 comparison."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from benchmark_spmv_using_csr5_amd import _capi
from benchmark_spmv_using_csr5_amd import handle as H
from benchmark_spmv_using_csr5_amd import matrices as M
from tests import attention_edges as E
from tests import mha_bias_reference as B
from tests import sddmm_reference as S
from tests import zoo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
DECLS = {
    "csr5hip_mha_biased": ("int csr5hip_mha_biased(csr5hip_handle h, int heads, double scale, const void *d_slopes, const void *d_Q, "
                           "int ldq, const void *d_K, int ldk, int k, const void *d_V, int ldv, int d, void *d_O, int ldo);"),
    "csr5hip_mha_biased_backward": ("int csr5hip_mha_biased_backward(csr5hip_handle h, int heads, double scale, const void *d_slopes, "
                                    "const void *d_Q, int ldq, const void *d_K, int ldk, int k, const void *d_V, int ldv, int d, "
                                    "const void *d_dO, int lddo, void *d_dQ, int lddq, void *d_dK, int lddk, void *d_dV, int lddv, "
                                    "void *d_work, void *d_dS, int ldds);"),
}


def test_library_exports_both_symbols_with_the_declared_signatures():
    import torch  # noqa: F401  (one HIP runtime per process: see _capi.load)
    lib = C.CDLL(_capi.LIB_PATH)
    with open(os.path.join(INC, "csr5hip.h")) as f:
        assert '#include "csr5hip_bias.h"' in f.read()  # (csr5hip.h brings the declarations in: users include that header)
    with open(os.path.join(INC, "csr5hip_bias.h")) as f:
        text = re.sub(r"\s+", " ", f.read())
    for name, decl in DECLS.items():
        assert hasattr(lib, name)
        assert decl in text
    bound = {name: (res, args) for name, res, args in _capi.SYMBOLS_BIASED}
    p, i, dbl = C.c_void_p, C.c_int, C.c_double
    assert bound == {"csr5hip_mha_biased": (i, [p, i, dbl, p, p, i, p, i, i, p, i, i, p, i]),
                     "csr5hip_mha_biased_backward": (i, [p, i, dbl, p, p, i, p, i, i, p, i, i, p, i, p, i, p, i, p, i, p, p, i])}
    loaded = _capi.load()
    assert loaded.csr5hip_mha_biased.argtypes == bound["csr5hip_mha_biased"][1]          # load() binds them
    assert loaded.csr5hip_mha_biased_backward.argtypes == bound["csr5hip_mha_biased_backward"][1]


def test_cpp_class_has_the_biased_members(tmp_path):
    src = tmp_path / "use_mha_biased.cpp"
    src.write_text(
        '#include "anonymouslib_hip.h"\n'
        "int use(anonymouslibHandle<int, unsigned, double> &A, const double *sl, const double *Q, const double *K, const double *V,\n"
        "        const double *dO, double *O, double *dQ, double *dK, double *dV, double *work, double *dS)\n"
        "{ return A.mhaBiased(4, 0.25, sl, Q, 32, K, 32, 8, V, 64, 16, O, 64)\n"
        "       + A.mhaBiasedBackward(4, 0.25, sl, Q, 32, K, 32, 8, V, 64, 16, dO, 64, dQ, 32, dK, 32, dV, 64, work, dS, 4); }\n"
        "int use32(anonymouslibHandle<int, unsigned, float> &A, const float *Q, const float *K, const float *V, const float *dO,\n"
        "          float *O, float *dQ)\n"
        "{ return A.mhaBiased(4, 1.0, nullptr, Q, 32, K, 32, 8, V, 64, 16, O, 64)\n"
        "       + A.mhaBiasedBackward(4, 1.0, nullptr, Q, 32, K, 32, 8, V, 64, 16, dO, 64, dQ, 32, nullptr, 32, nullptr, 64, nullptr,\n"
        "                             nullptr, 4); }\n")
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", f"-I{INC}", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _info_bytes(lib, h):
    info = _capi.Csr5Info()
    assert lib.csr5hip_get_info(h, C.byref(info)) == 0
    return bytes(info)


def test_return_codes_in_order_without_a_gpu():
    """Decided on the host, with fake non-null pointers, in csr5hip_mha's / csr5hip_mha_backward's order, to which a non-finite
    scale (with the first arguments) and ldds < heads with dS given (with the leading dimensions) are added; dS counts as a wanted
    output; get_info unchanged throughout."""
    lib = _capi.load()
    h = C.c_void_p()
    assert lib.csr5hip_create(C.byref(h), 10, 12, _capi.F64) == 0
    f = C.c_void_p(64)
    INV, CSR, UNK = _capi.INVALID_ARGUMENT, _capi.UNSUPPORTED_CSR_SPMV, _capi.UNKOWN_FORMAT

    def fwd(heads=3, scale=0.5, sl=f, Q=f, ldq=12, K=f, ldk=12, k=4, V=f, ldv=15, d=5, O=f, ldo=15, handle=h):
        return lib.csr5hip_mha_biased(handle, heads, scale, sl, Q, ldq, K, ldk, k, V, ldv, d, O, ldo)

    def bwd(heads=3, scale=0.5, sl=f, Q=f, ldq=12, K=f, ldk=12, k=4, V=f, ldv=15, d=5, dO=f, lddo=15, dQ=f, lddq=12, dK=None, lddk=12,
            dV=None, lddv=15, work=None, dS=None, ldds=3, handle=h):
        return lib.csr5hip_mha_biased_backward(handle, heads, scale, sl, Q, ldq, K, ldk, k, V, ldv, d, dO, lddo, dQ, lddq, dK, lddk, dV,
                                               lddv, work, dS, ldds)

    def no_companion(**kw):
        return bwd(**kw) == INV and "csr5hip_build_transpose" in _capi.last_error()
    before = _info_bytes(lib, h)
    for call in (fwd, bwd):
        assert call(handle=None) == INV
        assert call() == UNK and call(sl=None) == UNK                  # before inputCSR; slopes may be null
        assert call(Q=None, K=None, V=None) == UNK
        assert call(heads=0) == UNK
        assert call(heads=-1) == INV and call(k=-1) == INV and call(d=-1) == INV
        for bad in (float("nan"), float("inf"), -float("inf")):
            assert call(scale=bad) == INV                              # the scale comes before the format
        assert call(scale=0.0) == UNK and call(scale=-3.0) == UNK      # any finite scale is legal
    assert bwd(dS=f, ldds=2) == INV and bwd(dS=f, ldds=3) == UNK and bwd(dS=None, ldds=0) == UNK
    assert no_companion(dK=f, work=f) and no_companion(dV=f, work=f) and no_companion(heads=0, dK=f)
    assert lib.csr5hip_input_csr(h, 100, None, None, None) == 0       # CSR format, nnz > 0
    before = _info_bytes(lib, h)
    assert fwd() == CSR and bwd() == CSR and fwd(heads=0) == CSR and bwd(heads=0) == CSR
    for bad in (dict(heads=-1), dict(k=-1), dict(d=-1), dict(scale=float("nan")), dict(ldq=11), dict(ldk=11), dict(ldv=14), dict(ldo=14),
                dict(Q=None), dict(K=None), dict(V=None), dict(O=None)):
        assert fwd(**bad) == INV, bad
    for bad in (dict(heads=-1), dict(k=-1), dict(d=-1), dict(scale=float("inf")), dict(ldq=11), dict(ldk=11), dict(lddq=11), dict(lddk=11),
                dict(ldv=14), dict(lddo=14), dict(lddv=14), dict(dS=f, ldds=2), dict(Q=None), dict(K=None), dict(V=None), dict(dO=None),
                dict(dK=f), dict(dV=f)):
        assert bwd(**bad) == INV, bad
    assert bwd(dQ=None, dS=f, Q=None) == INV                           # dS alone is a wanted output: the operands are judged
    assert bwd(dQ=None, dS=f) == CSR and bwd(dQ=f, dS=f, ldds=7) == CSR
    assert no_companion(dQ=None, dS=f, dV=f, work=f)                   # the companion is judged before the format
    assert bwd(Q=None, K=None, V=None, dO=None, dQ=None) == CSR        # nothing wanted: nothing judged but the format
    assert _info_bytes(lib, h) == before
    assert lib.csr5hip_free(h) == 0


def test_python_methods_reject_bad_tensors_before_the_library():
    torch = pytest.importorskip("torch")
    A = H.anonymouslibHandle(6, 4)
    calls = []
    A.mha_biased_ptr = lambda *a: calls.append(a) or 0  # nothing may reach the library
    A.mha_biased_backward_ptr = lambda *a: calls.append(a) or 0
    f64 = torch.float64
    z = lambda *s: torch.zeros(*s, dtype=f64)  # noqa: E731
    fwd = dict(Q=z(6, 2, 3), K=z(4, 2, 3), V=z(4, 2, 5), O=z(6, 2, 5))
    bwd = dict(Q=z(6, 2, 3), K=z(4, 2, 3), V=z(4, 2, 5), dO=z(6, 2, 5), dQ=z(6, 2, 3), dK=z(4, 2, 3), dV=z(4, 2, 5), work=z(48))
    with pytest.raises(ValueError, match="inputCSR"):
        A.mhaBiased(**fwd)
    with pytest.raises(ValueError, match="inputCSR"):
        A.mhaBiasedBackward(**bwd)
    assert A.inputCSR(7, None, None, None) == 0
    with pytest.raises(ValueError, match="GPU"):
        A.mhaBiased(**fwd)                                             # host tensors: everything else is in order
    with pytest.raises(ValueError, match="GPU"):
        A.mhaBiasedBackward(**bwd, scale=0.5)
    # the operand checks are mha's: one of each kind suffices here
    with pytest.raises(ValueError, match="Q has 2 heads, K 3"):
        A.mhaBiased(**dict(fwd, K=z(4, 3, 3)))
    with pytest.raises(ValueError, match="K .*dtype"):
        A.mhaBiasedBackward(**dict(bwd, K=bwd["K"].float()))
    with pytest.raises(ValueError, match="work .*shape"):
        A.mhaBiasedBackward(**dict(bwd, work=z(47)))
    for method, good in ((A.mhaBiased, fwd), (A.mhaBiasedBackward, bwd)):
        for bad in (float("nan"), float("inf"), None, "1", True, z(1)):
            with pytest.raises(ValueError, match="scale"):
                method(**good, scale=bad)
        for bad, word in ((np.zeros(2), "tensor"), (torch.zeros(2), "dtype"), (z(3), "shape"), (z(2, 1), "shape"), (z(4)[::2], "contiguous"),
                          (z(2), "GPU")):
            with pytest.raises(ValueError, match=f"slopes .*{word}"):
                method(**good, slopes=bad)
    for bad, word in ((np.zeros((7, 2)), "tensor"), (torch.zeros(7, 2), "dtype"), (z(7, 3), "shape"), (z(6, 2), "shape"), (z(14), "shape"),
                      (z(7, 4)[:, ::2], "stride\\(1\\)"), (z(1, 2).expand(7, 2), "overlap"), (z(7, 2), "GPU")):
        with pytest.raises(ValueError, match=f"dS .*{word}"):
            A.mhaBiasedBackward(**bwd, dS=bad)
    pool = z(7 + 6, 6)
    with pytest.raises(ValueError, match="dS shares a storage with dQ"):
        A.mhaBiasedBackward(**dict(bwd, dQ=pool[7:].view(6, 2, 3)), dS=pool[:7, :2])
    assert calls == []
    A.close()


def test_multihead_attention_takes_scale_bias_and_slopes_without_a_gpu():
    import inspect

    from benchmark_spmv_using_csr5_amd import autograd
    sig = inspect.signature(autograd.multihead_attention)
    assert list(sig.parameters) == ["A", "Q", "K", "V", "scale", "bias", "slopes"]
    assert all(sig.parameters[n].default is None for n in ("scale", "bias", "slopes"))
    torch = pytest.importorskip("torch")
    sl = torch.ones(2, dtype=torch.float64, requires_grad=True)
    with pytest.raises(ValueError, match="slopes needs a gradient"):
        autograd.multihead_attention(None, None, None, None, slopes=sl)


def test_augmented_operands_reproduce_the_biased_scores():
    """in integers, where every sum is exact: (Q|u) . (K|slope v) = Q . K + slope u v per entry and head, and the bias values are
    u[i] v[j] per entry in CSR order, distinct across the repeated pairs' neighbours"""
    for mat in (S.duplicates_matrix(), {m.name: m for m in zoo.small_zoo()}["half-empty"]):
        u, v, a = B.rank_one(mat, seed=5)
        rows, cols = B.rows_of(mat), mat.col[:mat.nnz].astype(np.int64)
        assert a.shape == (mat.nnz,) and np.array_equal(a, u[rows] * v[cols]) and np.abs(a).max() <= 16 and len(np.unique(a)) > 8
        assert np.array_equal(a.astype(np.float32).astype(np.float64), a)
        rng = np.random.default_rng(6)
        for dtype in (np.float32, np.float64):
            Q = rng.integers(-8, 9, size=(mat.m, 3, 2)).astype(dtype)
            K = rng.integers(-8, 9, size=(mat.n, 3, 2)).astype(dtype)
            for slopes in (None, (2.0, 0.5, -1.0)):
                Qw, Kw = B.augment(Q, K, u, v, slopes)
                assert Qw.shape == (mat.m, 3, 3) and Kw.shape == (mat.n, 3, 3) and Qw.dtype == dtype and Kw.dtype == dtype
                assert Qw.flags.c_contiguous and Kw.flags.c_contiguous
                assert np.array_equal(Qw[:, :, :2], Q) and np.array_equal(Kw[:, :, :2], K)
                sl = np.ones(3) if slopes is None else np.array(slopes)
                want = (Q[rows].astype(np.float64) * K[cols]).sum(2) + sl[None, :] * a[:, None]
                assert np.array_equal((Qw[rows].astype(np.float64) * Kw[cols]).sum(2), want)
    with pytest.raises(AssertionError):
        B.augment(np.zeros((2, 1, 1)), np.zeros((2, 1, 1)), np.zeros(2), np.zeros(2), (0.3,))


def _sanitizers_link(cxx, tmp_path):
    src = tmp_path / "probe.cpp"
    src.write_text("int main() { return 0; }\n")
    r = subprocess.run([cxx, "-fsanitize=address,undefined", str(src), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    return r.returncode == 0 and subprocess.run([str(tmp_path / "probe")]).returncode == 0


def test_host_emulation_under_the_sanitizers(tmp_path):
    """scripts/host_emulation/run_mha_bias.py: stand-alone programs built from the kernel sources with
    -fsanitize=address,undefined; three heads (head groups of two and one), both precisions.  (k, d) = (3, 5), element loads, on
    kat0 and duplicates; (12, 8), every head's slice of every row 16-byte aligned, so that the sigma = 4 and sigma = 16
    configurations run the 16-byte-load instantiations of the biased kernels on exact-size heap blocks, on duplicates ALONE (rows
    of at most 16 entries and a wavefront's row; kat0 has only the former).  Measured on one machine: 63 s before the new shape,
    104 s with it on both matrices -- more than half as much again, so one matrix was kept -- and 98 to 106 s as it is (20 s of
    each figure build the two programs)."""
    cxx = "/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else "clang++"
    try:
        linked = _sanitizers_link(cxx, tmp_path)
    except OSError:
        linked = False
    if not linked:
        pytest.skip(f"{cxx} cannot link a program with -fsanitize=address,undefined (no sanitizer runtime)")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "host_emulation", "run_mha_bias.py"), "--matrices", "kat0,duplicates",
                        "--heads", "3", "--kd", "3x5,12x8", "--skip", "kat0:12x8", "--cxx", cxx], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.count(": ok") == 6 and r.stdout.count("duplicates") == 4 and r.stdout.count("k=12 d=8: ok") == 2, r.stdout


# ---- for tests/test_gpu_mha_bias_edges.py ------------------------------------------------------------------------------------------
def _round(fr, dtype):
    """a non-zero Fraction rounded ONCE to `dtype`, ties to even"""
    x = float(fr)  # (correctly rounded to float64)
    if dtype == np.float64:
        return np.float64(x)
    best = None
    f = np.float32(x)
    for cand in (np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))):
        if not np.isfinite(cand):
            continue
        dist = abs(Fraction(float(cand)) - fr)
        even = int(np.array(cand).view(np.uint32)) & 1 == 0
        if best is None or dist < best[0] or (dist == best[0] and even):
            best = (dist, cand)
    return best[1]


def _fma(x, y, z, dtype):
    """fma(x, y, z) of finite numpy scalars by exact rationals, one rounding, IEEE's sign of an exact zero (round to nearest)"""
    exact = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
    if exact != 0:
        return _round(exact, dtype)
    if x == 0 or y == 0:  # a zero product onto a zero: -0 only from two negative zeros
        neg = (bool(np.signbit(x)) != bool(np.signbit(y))) and bool(np.signbit(z))
        return dtype(-0.0) if neg and z == 0 else dtype(0.0)
    return dtype(0.0)     # an exact cancellation of non-zero terms


def _chain(q, k, dtype):
    acc = dtype(0.0)
    for a, b in zip(q, k):
        acc = _fma(a, b, acc, dtype)
    return acc


def _same_scalar(a, b):
    return a == b and bool(np.signbit(a)) == bool(np.signbit(b))


def test_padded_augmentation_reproduces_the_biased_scores_step_by_step():
    """k = 12 widened to 16: the biased score fma(chain(Q, K), c, slope u v) and the plain chain over c Q | u | 0 and
    K | slope v | 0, both in exact rationals rounded once per step, agree in every bit, the sign of zero included; with one entry
    whose c qk + b cancels exactly and one whose product and bias are zeros of opposite sign"""
    mats = {m.name: m for m in zoo.small_zoo()}
    for mat in (mats["kat0"], mats["dense16"]):
        rows, cols = B.rows_of(mat), mat.col[:mat.nnz].astype(np.int64)
        u, v, _ = B.rank_one(mat, seed=5)
        e0 = int(np.flatnonzero(u[rows] * v[cols] != 0)[0])       # this entry will cancel in head 0
        i1 = int([i for i in range(mat.m) if i != rows[e0] and mat.row_ptr[i + 1] > mat.row_ptr[i]][0])
        u[i1] = 0.0                                                 # this row's bias is +-0
        a = u[rows] * v[cols]
        assert np.signbit(a[rows == i1]).any() or (v[cols[rows == i1]] >= 0).all()
        for dtype in (np.float32, np.float64):
            for c in B.A_SCALES:
                for slopes in ((None, B.A_SLOPES) if mat.nnz < 100 else (B.A_SLOPES,)):
                    sl = np.ones(3) if slopes is None else np.array(slopes)
                    rng = np.random.default_rng(12)
                    Q = rng.uniform(-2, 2, size=(mat.m, 3, 12)).astype(dtype)
                    K = rng.uniform(-1, 1, size=(mat.n, 3, 12)).astype(dtype)
                    i0, j0 = int(rows[e0]), int(cols[e0])
                    Q[i0, 0], K[j0, 0] = 0, 0
                    Q[i0, 0, 3], K[j0, 0, 3] = -sl[0] * a[e0] / c, 1   # qk = -b / c exactly (integers over a power of two)
                    Q[i1, 1] = 0                                       # qk = +0 against b = +-0
                    Qw, Kw = B.augment(Q * dtype(B.scaled_identity(c)), K, u, v, slopes, pad=B.A_PAD)
                    assert Qw.shape == (mat.m, 3, 16) and Kw.shape == (mat.n, 3, 16) and Qw.dtype == dtype
                    assert not Qw[:, :, 13:].any() and not Kw[:, :, 13:].any() and not np.signbit(Qw[:, :, 13:]).any()
                    zeros = 0
                    for e in range(mat.nnz):
                        i, j = int(rows[e]), int(cols[e])
                        for h in range(3):
                            b = dtype(a[e]) if slopes is None else dtype(sl[h]) * dtype(a[e])  # (exact: small integers)
                            biased = _fma(_chain(Q[i, h], K[j, h], dtype), dtype(c), b, dtype)
                            plain = _chain(Qw[i, h], Kw[j, h], dtype)
                            assert _same_scalar(biased, plain), (mat.name, dtype, c, slopes, e, h, biased, plain)
                            if biased == 0:
                                zeros += 1
                                assert not np.signbit(biased)
                    assert zeros >= 2  # (the cancellation and the zeros of opposite sign were met)


@functools.lru_cache(maxsize=1)
def _class_edges():
    return E.class_edges()


def _classes(mat):
    """the rows of each class: <= 16, <= 512, <= 2 048, beyond"""
    lens = np.diff(mat.row_ptr)
    return [np.flatnonzero((lens > lo) & (lens <= hi)) for lo, hi in ((1, 16), (16, 512), (512, 2048), (2048, 1 << 30))]


def test_the_expectations_reject_wrong_kernels():
    """on the operands of tests/test_gpu_mha_bias_edges.py (A), class-edges, fp32, scale 0.25 and slopes (2, 0.5, -1): the score
    of the definition against four scores a wrong kernel could compute -- (qk + b) c; the slope ignored; the first head's slope
    for every head; the value of the row's next entry -- each differs in bits in a row of every class, so a bit-exact comparison
    of O (a function of the row's scores) cannot pass with any of them.  Rows of one entry have no neighbour and are left out."""
    mat = _class_edges()
    rows, cols = B.rows_of(mat), mat.col[:mat.nnz].astype(np.int64)
    _, _, a = B.rank_one(mat, seed=7)
    Q, K, _, _ = B.operands_a(mat, np.float32)
    qk = B.chain(Q[rows], K[cols])
    want = B.scores("definition", qk, 0.25, a, B.A_SLOPES, mat.row_ptr)
    # the emulation is the definition's: against exact rationals on a sample
    for e in np.random.default_rng(3).choice(mat.nnz, size=40, replace=False):
        for h in range(3):
            b = np.float32(B.A_SLOPES[h]) * np.float32(a[e])
            ref = _fma(_chain(Q[rows[e], h], K[cols[e], h], np.float32), np.float32(0.25), b, np.float32)
            assert _same_scalar(ref, want[e, h]), (e, h)
    for kind in B.SCORES[1:]:
        wrong = B.scores(kind, qk, 0.25, a, B.A_SLOPES, mat.row_ptr)
        differs = np.zeros(mat.m, dtype=bool)
        differs[rows[(wrong.view(np.uint32) != want.view(np.uint32)).any(axis=1)]] = True
        for cls, members in zip(("<= 16", "<= 512", "<= 2 048", "> 2 048"), _classes(mat)):
            assert members.size and differs[members].any(), (kind, cls)
            print(f"{kind}: rows {cls}: {int(differs[members].sum())} of {members.size} differ")


def _function_text(header, name):
    with open(os.path.join(ROOT, "benchmark_spmv_using_csr5_amd", "csrc", header)) as f:
        text = f.read()
    start = text.index("template <typename VT>\nstatic bool " + name + "(")
    return text[start:text.index("\n}\n", start) + 3]


def test_the_vec_rule_transcriptions_are_the_headers_functions(tmp_path):
    """attention_vec and attention_bwd_vec, cut out of the headers and compiled for the host, against ``B.vec_forward`` and
    ``B.vec_backward`` on a grid of types, heads, widths, leading dimensions and addresses"""
    src = tmp_path / "vec.cpp"
    src.write_text(
        "#include <cstddef>\n#include <cstdint>\n#include <cstdio>\n"
        + _function_text("csr5_attention_kern.h", "attention_vec") + _function_text("csr5_attention_bwd_kern.h", "attention_bwd_vec") +
        "static const void *at(int a) { return reinterpret_cast<const void *>((uintptr_t)4096 + a); }\n"
        "template <typename VT> static void grid(int sz) {\n"
        "  const int ks[] = {0, 1, 3, 4, 7, 8, 9, 12, 13, 16}, ds[] = {5, 8, 16}, ex[] = {0, 1, 2, 4}, ad[] = {0, 4, 8, 16};\n"
        "  for (int h = 1; h <= 3; h++) for (int k : ks) for (int e1 : ex) for (int e2 : ex) for (int a1 : ad) for (int a2 : ad)\n"
        "    std::printf(\"0 %d %d %d 0 %d %d 0 0 %d %d 0 0 %d\\n\", sz, h, k, h * k + e1, h * k + e2, a1, a2,\n"
        "                (int)attention_vec<VT>(h, at(a1), h * k + e1, at(a2), h * k + e2, k));\n"
        "  for (int h = 1; h <= 3; h++) for (int k : ks) for (int d : ds) for (int w = 0; w < 4; w++) for (int e : ex) for (int a : ad) {\n"
        "    int ld[4] = {h * k, h * k, h * d, h * d}, ads[4] = {0, 0, 0, 0};\n"
        "    ld[w] += e; ads[(w + 1) % 4] = a;\n"
        "    std::printf(\"1 %d %d %d %d %d %d %d %d %d %d %d %d %d\\n\", sz, h, k, d, ld[0], ld[1], ld[2], ld[3], ads[0], ads[1], ads[2], ads[3],\n"
        "                (int)attention_bwd_vec<VT>(h, k, d, at(ads[0]), ld[0], at(ads[1]), ld[1], at(ads[2]), ld[2], at(ads[3]), ld[3])); }\n"
        "}\n"
        "int main() { grid<float>(4); grid<double>(8); }\n")
    exe = tmp_path / "vec"
    r = subprocess.run(["g++", "-std=c++14", "-O0", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = np.array(subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split(), dtype=np.int64).reshape(-1, 14)
    seen = set()
    for back, sz, h, k, d, l0, l1, l2, l3, a0, a1, a2, a3, got in out.tolist():
        if back:
            want = B.vec_backward(h, k, d, sz, (l0, l1, l2, l3), (a0, a1, a2, a3))
        else:
            want = B.vec_forward(h, k, sz, l0, l1, a0, a1)
        assert want == bool(got), (back, sz, h, k, d, (l0, l1, l2, l3), (a0, a1, a2, a3), got)
        seen.add((back, got))
    assert seen == {(0, 0), (0, 1), (1, 0), (1, 1)} and out.shape[0] > 5000
    # the shapes of (A): 16-byte loads at 12 and at 16, in both types; of today's widened test (k = 5, 6): none
    for sz in (4, 8):
        for k in (B.A_K, B.A_K + 1 + B.A_PAD):
            assert B.vec_forward(3, k, sz, 3 * k, 3 * k) and B.vec_backward(3, k, B.A_D, sz, (3 * k, 3 * k, 3 * B.A_D, 3 * B.A_D))
        assert not B.vec_forward(3, 5, sz, 17, 17) and not B.vec_backward(3, 5, 5, sz, (17, 17, 15, 15))


def test_the_structure_the_path_test_relies_on():
    """``distinct_values`` is a permutation of the equidistant values; class-edges at sigma = 4 holds fast-track tiles (no row
    starts inside: CSR order), tiles in tile order and a non-empty tail, by the oracle's conversion"""
    from oracle.csr5_oracle import Oracle
    mat = _class_edges()
    val = B.distinct_values(mat, 1200)
    assert np.array_equal(np.sort(val), np.arange(mat.nnz) / mat.nnz * 4 - 2) and not np.array_equal(val, np.sort(val))
    assert not np.array_equal(val, B.distinct_values(mat, 1201))
    assert np.unique(val.astype(np.float32)).size == mat.nnz and val.min() == -2 and val.max() < 2
    fmt = Oracle().convert(64, 4, mat.m, mat.row_ptr, mat.col, val)
    fast, tail = B.tile_structure(fmt, mat.nnz)
    tiles = fmt.p - 1
    assert 0 < fast < tiles and 0 < tail <= 256 and tiles * 256 + tail == mat.nnz
    # the values travel with their columns: position by position the converted pair is a pair of the matrix
    pairs = set(zip(mat.col[:mat.nnz].tolist(), val.tolist()))
    assert all(pc in pairs for pc in zip(fmt.col[:mat.nnz].tolist(), fmt.val[:mat.nnz].tolist()))


def _transposed(mat):
    rows, cols = B.rows_of(mat), mat.col[:mat.nnz].astype(np.int64)
    order = np.argsort(cols, kind="stable")
    rp = np.zeros(mat.n + 1, dtype=np.int32)
    rp[1:] = np.cumsum(np.bincount(cols, minlength=mat.n))
    return M.CsrMatrix(mat.n, mat.m, rp, rows[order].astype(np.int32), np.ones(mat.nnz), mat.name + "^T")


def test_the_first_order_condition_of_the_float64_comparison_at_the_edges():
    """STAGES rho <= FIRST_ORDER (8 and 2**-6, tests/test_gpu_attention_autograd.py) for every case of (F): rho is a function of
    the inputs, so it is judged here, in numpy.  With values in [-2, 2) and Q in [-2, 2) nothing had to be shrunk: the largest
    STAGES rho is 3.95e-3 (fp32, class-edges, the row of 4 097 entries; (k, d) = (8, 16))."""
    worst = 0.0
    for mi, mat in enumerate((_class_edges(), _transposed(_class_edges()))):
        for ki, (k, d) in enumerate(B.F_KD):
            for dtype in (np.float64, np.float32):
                val, slopes, c, (Q, K, _, _) = B.case_f(mat, k, d, dtype, 1300 + 10 * mi + 2 * ki)
                assert val.min() >= -2 and val.max() < 2 and np.abs(slopes).max() < 1.5 and c == float(dtype(1 / np.sqrt(k)))
                rho = B.first_order_rho(mat, c, val, slopes, Q, K, dtype)
                print(f"{mat.name} {np.dtype(dtype).name} k={k} d={d}: rho {rho:.3e}")
                assert 8 * rho <= 2.0 ** -6, (mat.name, k, d, rho)
                worst = max(worst, 8 * rho)
    assert 1e-3 < worst < 2.0 ** -6
