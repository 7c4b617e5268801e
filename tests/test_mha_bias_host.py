"""csr5hip_mha_biased / csr5hip_mha_biased_backward on the host side (no GPU): the C ABI symbols and their declarations, the C++
class members, the return codes and their order, the Python argument checks of scale, slopes and dS,
``autograd.multihead_attention``'s new arguments, the host emulation of the kernel sources under the address and
undefined-behaviour sanitizers (stand-alone programs), and the augmented operands of tests/mha_bias_reference.py."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from benchmark_spmv_using_csr5_amd import _capi
from benchmark_spmv_using_csr5_amd import handle as H
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
    """scripts/host_emulation/run_mha_bias.py on kat0 and duplicates: stand-alone programs built from the kernel sources with
    -fsanitize=address,undefined; three heads (head groups of two and one), (k, d) = (3, 5), both precisions"""
    cxx = "/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else "clang++"
    try:
        linked = _sanitizers_link(cxx, tmp_path)
    except OSError:
        linked = False
    if not linked:
        pytest.skip(f"{cxx} cannot link a program with -fsanitize=address,undefined (no sanitizer runtime)")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "host_emulation", "run_mha_bias.py"), "--matrices", "kat0,duplicates",
                        "--heads", "3", "--kd", "3x5", "--cxx", cxx], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.count(": ok") == 4, r.stdout
