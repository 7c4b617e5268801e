"""csr5hip_gat / csr5hip_gat_backward on the host side (no GPU): the score chain restated in numpy against an operation-by-operation
restatement, the first-order condition of tests/test_gpu_gat.py's float64 comparison, the C ABI symbols and their declarations,
the C++ class members, the return codes and their order, the Python argument checks, that ``autograd.gat_attention`` imports, the
host emulation of the kernel sources under the address and undefined-behaviour sanitizers (a stand-alone program), and that the
numpy reference rejects two wrong kernels: g taken from the sign of l a instead of u's, and the a of head 0 used for every head."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from benchmark_spmv_using_csr5_amd import _capi
from benchmark_spmv_using_csr5_amd import handle as H
from tests import attention_edges as E
from tests import gat_reference as G
from tests import sddmm_reference as S
from tests import zoo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
DECLS = {
    "csr5hip_gat": ("int csr5hip_gat(csr5hip_handle h, int heads, double negative_slope, const void *d_a, double scale, const void *d_B, "
                    "int ldb, const void *d_Q, int ldq, const void *d_K, int ldk, int k, const void *d_V, int ldv, int d, void *d_O, "
                    "int ldo);"),
    "csr5hip_gat_backward": ("int csr5hip_gat_backward(csr5hip_handle h, int heads, double negative_slope, const void *d_a, double scale, "
                             "const void *d_B, int ldb, const void *d_Q, int ldq, const void *d_K, int ldk, int k, const void *d_V, "
                             "int ldv, int d, const void *d_dO, int lddo, void *d_dQ, int lddq, void *d_dK, int lddk, void *d_dV, "
                             "int lddv, void *d_work, void *d_dB, int lddb, void *d_dAr, int lddar);"),
}


def _small():
    return {m.name: m for m in zoo.small_zoo()}["kat0"], S.duplicates_matrix()


# ---- the chain in numpy ---------------------------------------------------------------------------------------------------------------
def test_the_numpy_chain_is_the_definition_operation_by_operation():
    """fp32, every operation carried out in float64 -- where the sum or product of two fp32 numbers of this range is exact -- and
    rounded ONCE to fp32: u, ns u, fma(a, l, z) as round(a l + z), fma(z, c, b) as round(z c + b), entry by entry in plain Python"""
    f32 = np.float32
    for mat in _small():
        rows, cols = G.rows_cols(mat)
        rng = np.random.default_rng([31, mat.nnz])
        heads, k = 2, 3
        Q = (rng.uniform(-1, 1, (mat.m, heads, k)) * 2).astype(f32)
        K = rng.uniform(-1, 1, (mat.n, heads, k)).astype(f32)
        bias = rng.uniform(-2, 2, (mat.nnz, heads)).astype(f32)
        a = G.exact_a(heads, k, f32)
        assert len(np.unique(a)) == 4
        for an, ns, scale, bn in ((a, 0.2, 0.25, bias), (None, 0.2, 1.0, None), (a, 0.0, 2.0, bias), (None, 1.0, 0.25, bias)):
            got = G.scores(mat, Q, K, an, ns, scale, bn, f32)
            assert got.dtype == f32 and got.shape == (mat.nnz, heads)
            nst = float(f32(ns))
            for e in range(mat.nnz):
                for h in range(heads):
                    z = 0.0
                    for c in range(k):
                        u = float(f32(float(Q[rows[e], h, c]) + float(K[cols[e], h, c])))
                        l = u if u > 0 else float(f32(nst * u))
                        z = float(f32((float(an[h, c]) if an is not None else 1.0) * l + z))
                    s = f32(z * scale + (float(bn[e, h]) if bn is not None else 0.0))
                    assert s.tobytes() == got[e, h].tobytes(), (mat.name, e, h, ns, scale)
    with pytest.raises(AssertionError):
        G.scores(mat, Q, K, a * f32(0.3), 0.2, 0.25, bias, f32)   # an a whose products round
    with pytest.raises(AssertionError):
        G.scores(mat, Q, K, a, 0.2, 0.3, bias, f32)               # a scale that is no power of two


def test_the_float64_references_agree_and_the_first_order_condition_holds():
    """the torch-autograd reference against the numpy one on the CPU; STAGES rho <= FIRST_ORDER (8 and 2**-6,
    tests/test_gpu_attention_autograd.py) for the cases of tests/test_gpu_gat.py's float64 comparisons: rho is a function of the
    inputs, so it is judged here"""
    torch = pytest.importorskip("torch")
    for mat, seed in ((E.class_edges(), G.F_SEEDS["class-edges"]), (G.random_matrix(), G.F_SEEDS["random"])):
        for dtype in (np.float64, np.float32):
            for sd, (heads, k, d) in ((seed, (G.F_HEADS, G.F_K, G.F_D)), (seed + 5, (G.F_HEADS, G.F_K, G.F_D))):
                a, ns, bias, c, (Q, K, _, _) = G.case(mat, heads, k, d, dtype, sd)
                rho = G.first_order_rho(mat, c, a, ns, bias, Q, K, dtype)
                print(f"{mat.name} {np.dtype(dtype).name}: rho {rho:.3e}")
                assert 8 * rho <= 2.0 ** -6, (mat.name, rho)
    mat = G.random_matrix()
    a, ns, _, c, (Q, X, _, dO) = G.case(mat, 3, 8, 8, np.float32, 2950)  # (the K-and-V-one-tensor case)
    assert 8 * G.first_order_rho(mat, c, a, ns, np.zeros((mat.nnz, 3)), Q, X, np.float32) <= 2.0 ** -6
    a, ns, bias, c, (Q, K, V, dO) = G.case(mat, 3, 8, 16, np.float64, 1)
    rows, cols = (torch.from_numpy(t) for t in G.rows_cols(mat))
    tt = [torch.from_numpy(t) for t in (a, bias, Q, K, V, dO)]
    want = G.reference(mat, rows, cols, c, tt[0], ns, tt[1], *tt[2:])
    got, mag, _ = G.numpy_reference(mat, a, ns, c, bias, Q, K, V, dO)
    for g, w, m_, n in zip(got, want[:6], mag, G.NAMES):
        assert np.abs(g - w.numpy()).max() <= 1e-12 * max(float(m_.max()), 1e-30), n
    assert np.abs(got[5].sum(0) - want[6].numpy()).max() <= 1e-10  # the gradient of a is dAr summed over the rows
    allow = G.allowances(mat, rows, cols, c, tt[0], ns, tt[1], *tt[2:], np.float64, 8)
    assert len(allow) == 8 and all(bool((al >= 0).all()) for al in allow[1:])


# ---- rejection ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("fp64", "fp32"))
def test_the_reference_rejects_two_wrong_kernels(dtype):
    """on the inputs of the host emulation (three heads, k = 3): what two wrong kernels would compute, judged by the emulation's own
    bound.  g from the sign of l a instead of u's: wherever a is negative the derivative is the other branch's, in dQ and dK (O, dV,
    dB and dAr do not see g).  The a of head 0 for every head: everything misses."""
    from scripts.host_emulation import emulation as EMU
    from scripts.host_emulation import run_gat
    for mat in _small():
        heads, k, d = 3, 3, 5
        a = EMU.distinct_a(heads, k, dtype)
        assert (a < 0).any() and (a > 0).any()
        bias = EMU.distinct_bias(mat.nnz, heads).astype(dtype)
        Q, K, V, dO = EMU.operands(mat, heads, k, d, dtype)
        u = float(np.finfo(dtype).eps) / 2
        ns, c = float(dtype(run_gat.SLOPE)), float(dtype(EMU.SCALE))
        ref, mag, smag = G.numpy_reference(mat, a, ns, c, bias, Q, K, V, dO)
        for r, al in zip(ref, mag):  # the reference passes its own bound when rounded to the type: the bound is not empty
            assert G.within(r.astype(dtype).astype(np.float64), r, al, smag, u).all()

        def misses(wrong):
            return [n for g, r, al, n in zip(wrong, ref, mag, G.NAMES) if not G.within(g, r, al, smag, u).all()]
        assert misses(G.numpy_reference(mat, a, ns, c, bias, Q, K, V, dO, wrong="g-from-la")[0]) == ["dQ", "dK"]
        assert misses(G.numpy_reference(mat, a, ns, c, bias, Q, K, V, dO, wrong="a-of-head-0")[0]) == list(G.NAMES)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_library_exports_both_symbols_with_the_declared_signatures():
    import torch  # noqa: F401  (one HIP runtime per process: see _capi.load)
    lib = C.CDLL(_capi.LIB_PATH)
    with open(os.path.join(INC, "csr5hip.h")) as f:
        assert '#include "csr5hip_gat.h"' in f.read()  # (csr5hip.h brings the declarations in: users include that header)
    with open(os.path.join(INC, "csr5hip_gat.h")) as f:
        text = re.sub(r"\s+", " ", f.read())
    for name, decl in DECLS.items():
        assert hasattr(lib, name)
        assert decl in text
    bound = {name: (res, args) for name, res, args in _capi.SYMBOLS_GAT}
    p, i, dbl = C.c_void_p, C.c_int, C.c_double
    assert bound == {"csr5hip_gat": (i, [p, i, dbl, p, dbl, p, i, p, i, p, i, i, p, i, i, p, i]),
                     "csr5hip_gat_backward": (i, [p, i, dbl, p, dbl, p, i, p, i, p, i, i, p, i, i, p, i, p, i, p, i, p, i, p, p, i, p, i])}
    loaded = _capi.load()
    assert loaded.csr5hip_gat.argtypes == bound["csr5hip_gat"][1]          # load() binds them
    assert loaded.csr5hip_gat_backward.argtypes == bound["csr5hip_gat_backward"][1]
    others = _capi.SYMBOLS + _capi.SYMBOLS_BIASED + _capi.SYMBOLS_EDGE_BIAS + _capi.SYMBOLS_LOWP + _capi.SYMBOLS_LOWP_BACKWARD
    assert not {n for n, _, _ in others} & set(bound)                      # (the other lists are as they were)


def test_cpp_class_has_the_gat_members(tmp_path):
    src = tmp_path / "use_gat.cpp"
    src.write_text(
        '#include "anonymouslib_hip.h"\n'
        "int use(anonymouslibHandle<int, unsigned, double> &A, const double *a, const double *B, const double *Q, const double *K,\n"
        "        const double *V, const double *dO, double *O, double *dQ, double *dK, double *dV, double *work, double *dB, double *dAr)\n"
        "{ return A.gat(4, 0.2, a, 0.25, B, 6, Q, 32, K, 32, 8, V, 64, 16, O, 64)\n"
        "       + A.gatBackward(4, 0.2, a, 0.25, B, 6, Q, 32, K, 32, 8, V, 64, 16, dO, 64, dQ, 32, dK, 32, dV, 64, work, dB, 4, dAr, 32); }\n"
        "int use32(anonymouslibHandle<int, unsigned, float> &A, const float *Q, const float *K, const float *V, const float *dO,\n"
        "          float *O, float *dQ)\n"
        "{ return A.gat(4, 0.2, nullptr, 1.0, nullptr, 4, Q, 4, K, 4, 1, V, 64, 16, O, 64)\n"
        "       + A.gatBackward(4, 0.2, nullptr, 1.0, nullptr, 4, Q, 4, K, 4, 1, V, 64, 16, dO, 64, dQ, 4, nullptr, 4, nullptr, 64, nullptr,\n"
        "                       nullptr, 4, nullptr, 4); }\n")
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", f"-I{INC}", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _info_bytes(lib, h):
    info = _capi.Csr5Info()
    assert lib.csr5hip_get_info(h, C.byref(info)) == 0
    return bytes(info)


def test_return_codes_in_order_without_a_gpu():
    """Decided on the host, with fake non-null pointers, on a handle with null arrays: the first arguments, the scale and the slope;
    then the leading dimensions, to which ldb, lddb and lddar (judged only with d_B, d_dB, d_dAr given) belong; then the shared
    path's order (null operands, the companion, the format), dB and dAr counting as wanted outputs; get_info unchanged throughout."""
    lib = _capi.load()
    h = C.c_void_p()
    assert lib.csr5hip_create(C.byref(h), 10, 12, _capi.F64) == 0
    f = C.c_void_p(64)
    INV, CSR, UNK = _capi.INVALID_ARGUMENT, _capi.UNSUPPORTED_CSR_SPMV, _capi.UNKOWN_FORMAT

    def fwd(heads=3, ns=0.2, a=f, scale=0.5, B=f, ldb=3, Q=f, ldq=12, K=f, ldk=12, k=4, V=f, ldv=15, d=5, O=f, ldo=15, handle=h):
        return lib.csr5hip_gat(handle, heads, ns, a, scale, B, ldb, Q, ldq, K, ldk, k, V, ldv, d, O, ldo)

    def bwd(heads=3, ns=0.2, a=f, scale=0.5, B=f, ldb=3, Q=f, ldq=12, K=f, ldk=12, k=4, V=f, ldv=15, d=5, dO=f, lddo=15, dQ=f, lddq=12,
            dK=None, lddk=12, dV=None, lddv=15, work=None, dB=None, lddb=3, dAr=None, lddar=12, handle=h):
        return lib.csr5hip_gat_backward(handle, heads, ns, a, scale, B, ldb, Q, ldq, K, ldk, k, V, ldv, d, dO, lddo, dQ, lddq, dK, lddk,
                                        dV, lddv, work, dB, lddb, dAr, lddar)

    def no_companion(**kw):
        return bwd(**kw) == INV and "csr5hip_build_transpose" in _capi.last_error() and "csr5hip_gat_backward" in _capi.last_error()
    before = _info_bytes(lib, h)
    for call in (fwd, bwd):
        assert call(handle=None) == INV
        assert call() == UNK and call(B=None) == UNK and call(a=None) == UNK   # before inputCSR; a and B may be null
        assert call(Q=None, K=None, V=None) == UNK
        assert call(heads=0) == UNK
        assert call(heads=-1) == INV and call(k=-1) == INV and call(d=-1) == INV
        for bad in (float("nan"), float("inf"), -float("inf")):
            assert call(scale=bad) == INV and call(ns=bad) == INV             # the scale and the slope come before the format
        assert call(ns=0.0) == UNK and call(ns=-3.0) == UNK and call(ns=1.0) == UNK  # any finite slope is legal
        assert call(ldb=2) == INV and call(ldb=3) == UNK and call(B=None, ldb=0) == UNK
        assert call(k=0, ldq=0, ldk=0) == UNK                                  # k = 0 is legal
    assert bwd(dB=f, lddb=2) == INV and bwd(dB=f, lddb=3) == UNK and bwd(dB=None, lddb=0) == UNK
    assert bwd(dAr=f, lddar=11) == INV and bwd(dAr=f, lddar=12) == UNK and bwd(dAr=None, lddar=0) == UNK  # lddar: only with dAr
    assert no_companion(dK=f, work=f) and no_companion(dV=f, work=f) and no_companion(heads=0, dK=f)
    assert lib.csr5hip_input_csr(h, 100, None, None, None) == 0               # CSR format, nnz > 0
    before = _info_bytes(lib, h)
    assert fwd() == CSR and bwd() == CSR and fwd(heads=0) == CSR and bwd(heads=0) == CSR and fwd(a=None, B=None) == CSR
    for bad in (dict(heads=-1), dict(k=-1), dict(d=-1), dict(scale=float("nan")), dict(ns=float("nan")), dict(ldq=11), dict(ldk=11),
                dict(ldv=14), dict(ldo=14), dict(ldb=2), dict(Q=None), dict(K=None), dict(V=None), dict(O=None)):
        assert fwd(**bad) == INV, bad
    for bad in (dict(heads=-1), dict(k=-1), dict(d=-1), dict(scale=float("inf")), dict(ns=float("inf")), dict(ldq=11), dict(ldk=11),
                dict(lddq=11), dict(lddk=11), dict(ldv=14), dict(lddo=14), dict(lddv=14), dict(ldb=2), dict(dB=f, lddb=2),
                dict(dAr=f, lddar=11), dict(Q=None), dict(K=None), dict(V=None), dict(dO=None), dict(dK=f), dict(dV=f)):
        assert bwd(**bad) == INV, bad
    # the leading dimensions come before the null operands and before the companion
    assert bwd(dK=f, work=f, dAr=f, lddar=11) == INV and bwd(Q=None, dAr=f, lddar=11) == INV and bwd(Q=None, dB=f, lddb=2) == INV
    assert bwd(dQ=None, dAr=f, Q=None) == INV                                  # dAr alone is a wanted output: the operands are judged
    assert bwd(dQ=None, dAr=f) == CSR and bwd(dQ=None, dB=f) == CSR and bwd(dQ=f, dAr=f, lddar=40) == CSR
    assert bwd(dQ=None, dAr=f, work=None) == CSR                               # dAr is a row-side output: no workspace, no companion
    assert no_companion(dQ=None, dAr=f, dV=f, work=f)                          # the companion is judged before the format
    assert bwd(Q=None, K=None, V=None, dO=None, dQ=None) == CSR                # nothing wanted: nothing judged but the format
    assert _info_bytes(lib, h) == before
    assert lib.csr5hip_free(h) == 0


# ---- the Python layers ------------------------------------------------------------------------------------------------------------------
def test_python_methods_reject_bad_tensors_before_the_library():
    torch = pytest.importorskip("torch")
    A = H.anonymouslibHandle(6, 4)
    calls = []
    A.gat_ptr = lambda *a: calls.append(a) or 0  # nothing may reach the library
    A.gat_backward_ptr = lambda *a: calls.append(a) or 0
    f64 = torch.float64
    z = lambda *s: torch.zeros(*s, dtype=f64)  # noqa: E731
    fwd = dict(Q=z(6, 2, 3), K=z(4, 2, 3), V=z(4, 2, 5), O=z(6, 2, 5))
    bwd = dict(Q=z(6, 2, 3), K=z(4, 2, 3), V=z(4, 2, 5), dO=z(6, 2, 5), dQ=z(6, 2, 3), dK=z(4, 2, 3), dV=z(4, 2, 5), work=z(48))
    with pytest.raises(ValueError, match="inputCSR"):
        A.gat(**fwd)
    with pytest.raises(ValueError, match="inputCSR"):
        A.gatBackward(**bwd)
    assert A.inputCSR(7, None, None, None) == 0
    with pytest.raises(ValueError, match="GPU"):
        A.gat(**fwd)                                                   # host tensors: everything else is in order
    with pytest.raises(ValueError, match="GPU"):
        A.gatBackward(**bwd, scale=0.5, B=z(7, 2), dB=z(7, 2), dAr=z(6, 2, 3))
    with pytest.raises(ValueError, match="Q has 2 heads, K 3"):
        A.gat(**dict(fwd, K=z(4, 3, 3)))
    with pytest.raises(ValueError, match="work .*shape"):
        A.gatBackward(**dict(bwd, work=z(47)))
    for method, good in ((A.gat, fwd), (A.gatBackward, bwd)):
        for bad in (float("nan"), float("inf"), None, "1", True, z(1)):
            with pytest.raises(ValueError, match="scale"):
                method(**good, scale=bad)
            with pytest.raises(ValueError, match="negative_slope"):
                method(**good, negative_slope=bad)
        for bad, word in ((np.zeros((2, 3)), "tensor"), (z(6), "shape"), (torch.zeros(2, 3), "dtype"), (z(3, 2), "shape"),
                          (z(2, 4), "shape"), (z(2, 6)[:, ::2], "contiguous"), (z(4, 3)[::2], "contiguous"), (z(2, 3), "GPU")):
            with pytest.raises(ValueError, match=f" a .*{word}"):
                method(**good, a=bad)
        with pytest.raises(ValueError, match=" B .*shape"):
            method(**good, B=z(7, 3))
    # dAr is judged as dQ is, and shares storage with no other argument
    for bad, text in ((z(6, 2, 4), "width 3, dAr 4"), (z(4, 2, 3), "dAr must have shape"), (z(6, 3, 3), "2 heads, dAr 3"),
                      (torch.zeros(6, 2, 3), "dAr has dtype"), (z(6, 2, 6)[:, :, ::2], "dAr must have stride")):
        with pytest.raises(ValueError, match=text):
            A.gatBackward(**bwd, dAr=bad)
    pool = z(2, 6, 2, 3)
    with pytest.raises(ValueError, match="dAr shares storage with dQ"):
        A.gatBackward(**dict(bwd, dQ=pool[0]), dAr=pool[1])
    with pytest.raises(ValueError, match="dAr shares storage with Q"):
        A.gatBackward(**dict(bwd, Q=pool[0]), dAr=pool[1])
    ab = z(8, 3)
    with pytest.raises(ValueError, match="dB shares a storage with a"):
        A.gatBackward(**bwd, a=ab[:2], dB=ab[1:8, :2])
    assert calls == []
    A.close()


def test_gat_attention_imports_and_is_documented_without_a_gpu():
    pytest.importorskip("torch")
    from benchmark_spmv_using_csr5_amd import autograd
    assert "gat_attention" in autograd.__all__ and callable(autograd.gat_attention)
    for word in ("GATv2", "dAr.sum(0)", "gatBackward", "(nnz, H)"):
        assert word in autograd.gat_attention.__doc__
    with pytest.raises(ValueError, match="2-D"):
        autograd.gat_attention(None, None, None, None, bias=np.zeros(3))


# ---- the host emulation -----------------------------------------------------------------------------------------------------------------
def _sanitizers_link(cxx, tmp_path):
    src = tmp_path / "probe.cpp"
    src.write_text("int main() { return 0; }\n")
    r = subprocess.run([cxx, "-fsanitize=address,undefined", str(src), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    return r.returncode == 0 and subprocess.run([str(tmp_path / "probe")]).returncode == 0


def test_host_emulation_under_the_sanitizers(tmp_path):
    """scripts/host_emulation/run_gat.py: a stand-alone program built from the kernel sources with -fsanitize=address,undefined;
    kat0 and duplicates, one head and three (head groups of two and one), (k, d) = (1, 5) and (3, 5), both precisions, forward and
    backward; the padded configuration has NaN in all padding.  Every operand, a, B, dB, dAr, the workspace and the map is a heap
    block of exactly its declared size, the patterns carry no value array."""
    cxx = "/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else "clang++"
    try:
        linked = _sanitizers_link(cxx, tmp_path)
    except OSError:
        linked = False
    if not linked:
        pytest.skip(f"{cxx} cannot link a program with -fsanitize=address,undefined (no sanitizer runtime)")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "host_emulation", "run_gat.py"), "--matrices", "kat0,duplicates",
                        "--heads", "1,3", "--kd", "1x5,3x5", "--cxx", cxx], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.count(": ok") == 16 and r.stdout.count("duplicates") == 8 and r.stdout.count("heads=3 k=3 d=5: ok") == 4, r.stdout
