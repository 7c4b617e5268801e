"""csr5hip_mha_edge_bias / csr5hip_mha_edge_bias_backward on the host side (no GPU): the C ABI symbols and their declarations,
the C++ class members, the return codes and their order, the Python argument checks of B and dB, the routing of
``autograd.multihead_attention`` by the bias's dimension, the host emulation of the kernel sources under the address and
undefined-behaviour sanitizers (stand-alone programs), and that the emulation's expectations reject the wrong kernels a new
indexing could be: the bias of head 0 for every head, the bias at the A^T-CSR position instead of through the map, ldb taken as
heads.  The first-order condition of tests/test_gpu_mha_edge_bias.py's float64 comparison is judged here too."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from benchmark_spmv_using_csr5_amd import _capi
from benchmark_spmv_using_csr5_amd import handle as H
from scripts.host_emulation import emulation as EMU
from tests import attention_edges as E
from tests import edge_bias_reference as EB
from tests import sddmm_reference as S
from tests import zoo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
DECLS = {
    "csr5hip_mha_edge_bias": ("int csr5hip_mha_edge_bias(csr5hip_handle h, int heads, double scale, const void *d_B, int ldb, "
                              "const void *d_Q, int ldq, const void *d_K, int ldk, int k, const void *d_V, int ldv, int d, void *d_O, "
                              "int ldo);"),
    "csr5hip_mha_edge_bias_backward": ("int csr5hip_mha_edge_bias_backward(csr5hip_handle h, int heads, double scale, const void *d_B, "
                                       "int ldb, const void *d_Q, int ldq, const void *d_K, int ldk, int k, const void *d_V, int ldv, "
                                       "int d, const void *d_dO, int lddo, void *d_dQ, int lddq, void *d_dK, int lddk, void *d_dV, "
                                       "int lddv, void *d_work, void *d_dB, int lddb);"),
}


def test_library_exports_both_symbols_with_the_declared_signatures():
    import torch  # noqa: F401  (one HIP runtime per process: see _capi.load)
    lib = C.CDLL(_capi.LIB_PATH)
    with open(os.path.join(INC, "csr5hip.h")) as f:
        assert '#include "csr5hip_edge_bias.h"' in f.read()  # (csr5hip.h brings the declarations in: users include that header)
    with open(os.path.join(INC, "csr5hip_edge_bias.h")) as f:
        text = re.sub(r"\s+", " ", f.read())
    for name, decl in DECLS.items():
        assert hasattr(lib, name)
        assert decl in text
    bound = {name: (res, args) for name, res, args in _capi.SYMBOLS_EDGE_BIAS}
    p, i, dbl = C.c_void_p, C.c_int, C.c_double
    assert bound == {"csr5hip_mha_edge_bias": (i, [p, i, dbl, p, i, p, i, p, i, i, p, i, i, p, i]),
                     "csr5hip_mha_edge_bias_backward": (i, [p, i, dbl, p, i, p, i, p, i, i, p, i, i, p, i, p, i, p, i, p, i, p, p, i])}
    loaded = _capi.load()
    assert loaded.csr5hip_mha_edge_bias.argtypes == bound["csr5hip_mha_edge_bias"][1]          # load() binds them
    assert loaded.csr5hip_mha_edge_bias_backward.argtypes == bound["csr5hip_mha_edge_bias_backward"][1]
    assert not {n for n, _, _ in _capi.SYMBOLS + _capi.SYMBOLS_BIASED} & set(bound)          # (the other lists are as they were)


def test_cpp_class_has_the_edge_bias_members(tmp_path):
    src = tmp_path / "use_mha_edge_bias.cpp"
    src.write_text(
        '#include "anonymouslib_hip.h"\n'
        "int use(anonymouslibHandle<int, unsigned, double> &A, const double *B, const double *Q, const double *K, const double *V,\n"
        "        const double *dO, double *O, double *dQ, double *dK, double *dV, double *work, double *dB)\n"
        "{ return A.mhaEdgeBias(4, 0.25, B, 6, Q, 32, K, 32, 8, V, 64, 16, O, 64)\n"
        "       + A.mhaEdgeBiasBackward(4, 0.25, B, 6, Q, 32, K, 32, 8, V, 64, 16, dO, 64, dQ, 32, dK, 32, dV, 64, work, dB, 4); }\n"
        "int use32(anonymouslibHandle<int, unsigned, float> &A, const float *Q, const float *K, const float *V, const float *dO,\n"
        "          float *O, float *dQ)\n"
        "{ return A.mhaEdgeBias(4, 1.0, nullptr, 4, Q, 32, K, 32, 8, V, 64, 16, O, 64)\n"
        "       + A.mhaEdgeBiasBackward(4, 1.0, nullptr, 4, Q, 32, K, 32, 8, V, 64, 16, dO, 64, dQ, 32, nullptr, 32, nullptr, 64, nullptr,\n"
        "                               nullptr, 4); }\n")
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", f"-I{INC}", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _info_bytes(lib, h):
    info = _capi.Csr5Info()
    assert lib.csr5hip_get_info(h, C.byref(info)) == 0
    return bytes(info)


def test_return_codes_in_order_without_a_gpu():
    """Decided on the host, with fake non-null pointers: the first arguments and the scale; then the leading dimensions, to which
    ldb < heads with B given and lddb < heads with dB given belong; then csr5hip_mha's / csr5hip_mha_backward's order (null
    operands, the companion, the format), dB counting as a wanted output; get_info unchanged throughout."""
    lib = _capi.load()
    h = C.c_void_p()
    assert lib.csr5hip_create(C.byref(h), 10, 12, _capi.F64) == 0
    f = C.c_void_p(64)
    INV, CSR, UNK = _capi.INVALID_ARGUMENT, _capi.UNSUPPORTED_CSR_SPMV, _capi.UNKOWN_FORMAT

    def fwd(heads=3, scale=0.5, B=f, ldb=3, Q=f, ldq=12, K=f, ldk=12, k=4, V=f, ldv=15, d=5, O=f, ldo=15, handle=h):
        return lib.csr5hip_mha_edge_bias(handle, heads, scale, B, ldb, Q, ldq, K, ldk, k, V, ldv, d, O, ldo)

    def bwd(heads=3, scale=0.5, B=f, ldb=3, Q=f, ldq=12, K=f, ldk=12, k=4, V=f, ldv=15, d=5, dO=f, lddo=15, dQ=f, lddq=12, dK=None,
            lddk=12, dV=None, lddv=15, work=None, dB=None, lddb=3, handle=h):
        return lib.csr5hip_mha_edge_bias_backward(handle, heads, scale, B, ldb, Q, ldq, K, ldk, k, V, ldv, d, dO, lddo, dQ, lddq, dK,
                                                  lddk, dV, lddv, work, dB, lddb)

    def no_companion(**kw):
        return bwd(**kw) == INV and "csr5hip_build_transpose" in _capi.last_error() and "edge_bias" in _capi.last_error()
    before = _info_bytes(lib, h)
    for call in (fwd, bwd):
        assert call(handle=None) == INV
        assert call() == UNK and call(B=None) == UNK                   # before inputCSR; B may be null
        assert call(Q=None, K=None, V=None) == UNK
        assert call(heads=0) == UNK
        assert call(heads=-1) == INV and call(k=-1) == INV and call(d=-1) == INV
        for bad in (float("nan"), float("inf"), -float("inf")):
            assert call(scale=bad) == INV                              # the scale comes before the format
        assert call(scale=0.0) == UNK and call(scale=-3.0) == UNK      # any finite scale is legal
        assert call(ldb=2) == INV and call(ldb=3) == UNK and call(ldb=7) == UNK
        assert call(B=None, ldb=0) == UNK                              # ldb is judged only with B given
    assert bwd(dB=f, lddb=2) == INV and bwd(dB=f, lddb=3) == UNK and bwd(dB=None, lddb=0) == UNK
    assert no_companion(dK=f, work=f) and no_companion(dV=f, work=f) and no_companion(heads=0, dK=f)
    assert lib.csr5hip_input_csr(h, 100, None, None, None) == 0       # CSR format, nnz > 0
    before = _info_bytes(lib, h)
    assert fwd() == CSR and bwd() == CSR and fwd(heads=0) == CSR and bwd(heads=0) == CSR and fwd(B=None) == CSR and bwd(B=None) == CSR
    for bad in (dict(heads=-1), dict(k=-1), dict(d=-1), dict(scale=float("nan")), dict(ldq=11), dict(ldk=11), dict(ldv=14), dict(ldo=14),
                dict(ldb=2), dict(Q=None), dict(K=None), dict(V=None), dict(O=None)):
        assert fwd(**bad) == INV, bad
    for bad in (dict(heads=-1), dict(k=-1), dict(d=-1), dict(scale=float("inf")), dict(ldq=11), dict(ldk=11), dict(lddq=11), dict(lddk=11),
                dict(ldv=14), dict(lddo=14), dict(lddv=14), dict(ldb=2), dict(dB=f, lddb=2), dict(Q=None), dict(K=None), dict(V=None),
                dict(dO=None), dict(dK=f), dict(dV=f)):
        assert bwd(**bad) == INV, bad
    # the leading dimensions come before the null operands and before the companion: no companion text is left by them
    assert bwd(dK=f, work=f, ldb=2) == INV and bwd(Q=None, dB=f, lddb=2) == INV
    assert bwd(dQ=None, dB=f, Q=None) == INV                           # dB alone is a wanted output: the operands are judged
    assert bwd(dQ=None, dB=f) == CSR and bwd(dQ=f, dB=f, lddb=7) == CSR
    assert no_companion(dQ=None, dB=f, dV=f, work=f)                   # the companion is judged before the format
    assert bwd(Q=None, K=None, V=None, dO=None, dQ=None) == CSR        # nothing wanted: nothing judged but the format
    assert _info_bytes(lib, h) == before
    assert lib.csr5hip_free(h) == 0


def test_python_methods_reject_bad_tensors_before_the_library():
    torch = pytest.importorskip("torch")
    A = H.anonymouslibHandle(6, 4)
    calls = []
    A.mha_edge_bias_ptr = lambda *a: calls.append(a) or 0  # nothing may reach the library
    A.mha_edge_bias_backward_ptr = lambda *a: calls.append(a) or 0
    f64 = torch.float64
    z = lambda *s: torch.zeros(*s, dtype=f64)  # noqa: E731
    fwd = dict(Q=z(6, 2, 3), K=z(4, 2, 3), V=z(4, 2, 5), O=z(6, 2, 5))
    bwd = dict(Q=z(6, 2, 3), K=z(4, 2, 3), V=z(4, 2, 5), dO=z(6, 2, 5), dQ=z(6, 2, 3), dK=z(4, 2, 3), dV=z(4, 2, 5), work=z(48))
    with pytest.raises(ValueError, match="inputCSR"):
        A.mhaEdgeBias(**fwd)
    with pytest.raises(ValueError, match="inputCSR"):
        A.mhaEdgeBiasBackward(**bwd)
    assert A.inputCSR(7, None, None, None) == 0
    with pytest.raises(ValueError, match="GPU"):
        A.mhaEdgeBias(**fwd)                                           # host tensors: everything else is in order
    with pytest.raises(ValueError, match="GPU"):
        A.mhaEdgeBiasBackward(**bwd, scale=0.5, B=z(7, 2), dB=z(7, 2))
    # the operand checks are mha's: one of each kind suffices here
    with pytest.raises(ValueError, match="Q has 2 heads, K 3"):
        A.mhaEdgeBias(**dict(fwd, K=z(4, 3, 3)))
    with pytest.raises(ValueError, match="K .*dtype"):
        A.mhaEdgeBiasBackward(**dict(bwd, K=bwd["K"].float()))
    with pytest.raises(ValueError, match="work .*shape"):
        A.mhaEdgeBiasBackward(**dict(bwd, work=z(47)))
    bad_tensors = ((np.zeros((7, 2)), "tensor"), (z(7), "shape"),      # no tensor; a 1-D B
                   (torch.zeros(7, 2), "dtype"),                        # a wrong dtype
                   (z(6, 2), "shape"), (z(14), "shape"),                # a wrong first dimension
                   (z(7, 4)[:, ::2], "stride\\(1\\)"),                  # a non-unit last stride
                   (z(7, 1), "shape"), (z(7, 3), "shape"),              # fewer than H columns; more
                   (z(1, 2).expand(7, 2), "overlap"), (z(7, 2), "GPU"))
    for method, good in ((A.mhaEdgeBias, fwd), (A.mhaEdgeBiasBackward, bwd)):
        for bad in (float("nan"), float("inf"), None, "1", True, z(1)):
            with pytest.raises(ValueError, match="scale"):
                method(**good, scale=bad)
        for bad, word in bad_tensors:
            with pytest.raises(ValueError, match=f" B .*{word}"):
                method(**good, B=bad)
    for bad, word in bad_tensors:
        with pytest.raises(ValueError, match=f"dB .*{word}"):
            A.mhaEdgeBiasBackward(**bwd, dB=bad)
    pool = z(7 + 6, 6)
    with pytest.raises(ValueError, match="dB shares a storage with dQ"):
        A.mhaEdgeBiasBackward(**dict(bwd, dQ=pool[7:].view(6, 2, 3)), dB=pool[:7, :2])
    both = z(7, 4)
    with pytest.raises(ValueError, match="dB shares a storage with B"):
        A.mhaEdgeBiasBackward(**bwd, B=both[:, :2], dB=both[:, 2:])
    assert calls == []
    # a slice of a wider tensor is legal: the shape and stride checks pass and only the device is left to object to
    with pytest.raises(ValueError, match="B must live on the GPU"):
        A._mha_edge_args("probe", 2, 1.0, z(7, 5)[:, :2], z(7, 6)[:, 1:3], ())
    A.close()


def test_multihead_attention_routes_by_the_dimension_of_the_bias(monkeypatch):
    torch = pytest.importorskip("torch")
    from benchmark_spmv_using_csr5_amd import autograd
    seen = []
    monkeypatch.setattr(autograd._MultiheadAttention, "apply", staticmethod(lambda *a: seen.append(("plain", len(a)))))
    monkeypatch.setattr(autograd._BiasedMultiheadAttention, "apply", staticmethod(lambda *a: seen.append(("values", a[5].dim(), a[4]))))
    monkeypatch.setattr(autograd._EdgeBiasMultiheadAttention, "apply", staticmethod(lambda *a: seen.append(("edge", a[5].dim(), a[4]))))
    one, two = torch.zeros(7), torch.zeros(7, 2)
    sl = torch.ones(2)
    autograd.multihead_attention(None, None, None, None)
    autograd.multihead_attention(None, None, None, None, bias=one)
    autograd.multihead_attention(None, None, None, None, scale=0.5, bias=one, slopes=sl)
    autograd.multihead_attention(None, None, None, None, bias=two)
    autograd.multihead_attention(None, None, None, None, scale=0.25, bias=two)
    assert seen == [("plain", 4), ("values", 1, 1.0), ("values", 1, 0.5), ("edge", 2, 1.0), ("edge", 2, 0.25)]
    with pytest.raises(ValueError, match="slopes cannot be combined with a 2-D"):
        autograd.multihead_attention(None, None, None, None, bias=two, slopes=sl)
    assert len(seen) == 5
    for text in (autograd.__doc__, autograd.multihead_attention.__doc__):
        assert "mhaEdgeBias" in text and "(nnz, H)" in text


def _sanitizers_link(cxx, tmp_path):
    src = tmp_path / "probe.cpp"
    src.write_text("int main() { return 0; }\n")
    r = subprocess.run([cxx, "-fsanitize=address,undefined", str(src), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    return r.returncode == 0 and subprocess.run([str(tmp_path / "probe")]).returncode == 0


def test_host_emulation_under_the_sanitizers(tmp_path):
    """scripts/host_emulation/run_mha_edge_bias.py: stand-alone programs built from the kernel sources with
    -fsanitize=address,undefined; kat0 and duplicates, one head and three (head groups of two and one), (k, d) = (3, 5), both
    precisions, forward and backward; the padded configuration has ldb = heads + 2.  B, dB and the map are heap blocks of exactly
    nnz ldb, nnz lddb and nnz elements, the patterns carry no value array.  Measured on one machine: 83 s, of which about 20 s
    build the two programs."""
    cxx = "/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else "clang++"
    try:
        linked = _sanitizers_link(cxx, tmp_path)
    except OSError:
        linked = False
    if not linked:
        pytest.skip(f"{cxx} cannot link a program with -fsanitize=address,undefined (no sanitizer runtime)")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "host_emulation", "run_mha_edge_bias.py"), "--matrices", "kat0,duplicates",
                        "--heads", "1,3", "--kd", "3x5", "--cxx", cxx], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.count(": ok") == 8 and r.stdout.count("duplicates") == 4 and r.stdout.count("heads=3 k=3 d=5: ok") == 4, r.stdout


def _emulation_case(name, dtype):
    mat = {"kat0": {m.name: m for m in zoo.small_zoo()}["kat0"], "duplicates": S.duplicates_matrix()}[name]
    H_, k, d = 3, 3, 5
    bias = EMU.distinct_bias(mat.nnz, H_).astype(dtype)
    return mat, bias, EMU.operands(mat, H_, k, d, dtype)


@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("fp64", "fp32"))
@pytest.mark.parametrize("name", ("kat0", "duplicates"))
def test_the_emulations_expectations_reject_wrong_kernels(name, dtype):
    """on the very inputs of the emulation (three heads): the reference against what three wrong kernels would compute, judged by
    the emulation's own bound (``within``).  Each must miss it in O, dQ and dB (the row side) or in dK and dV (the column side):
    a test that a wrong kernel would pass shows nothing."""
    mat, bias, (Q, K, V, dO) = _emulation_case(name, dtype)
    u = float(np.finfo(dtype).eps) / 2
    ref, mag, smag = EMU.edge_reference(mat, bias, Q, K, V, dO)
    # the reference passes its own bound when rounded to the type: the bound is not empty
    for r, a in zip(ref, mag):
        assert EMU.within(r.astype(dtype).astype(np.float64), r, a, smag, u).all()
    _, amap = EMU.transpose_with_map(mat)
    amap = amap.astype(np.int64)
    assert not np.array_equal(amap, np.arange(mat.nnz))

    def misses(wrong, which):
        return [what for g, r, a, what in zip(wrong, ref, mag, EMU.EDGE_NAMES) if what in which and not EMU.within(g, r, a, smag, u).all()]
    # 1. the bias of head 0 used for every head
    head0 = np.repeat(bias[:, :1], bias.shape[1], axis=1)
    assert misses(EMU.edge_reference(mat, head0, Q, K, V, dO)[0], EMU.EDGE_NAMES) == list(EMU.EDGE_NAMES)
    # 2. the column kernel reads B at the A^T-CSR position q instead of at map[q]: the entry of rank e = map[q] gets B[q]
    at_position = np.empty_like(bias)
    at_position[amap] = bias
    assert misses(EMU.edge_reference(mat, bias, Q, K, V, dO, B_col=at_position)[0], ("dK", "dV")) == ["dK", "dV"]
    # 3. ldb taken as heads: element (e, h) read at e heads + h of the block of nnz (heads + 2) values (finite padding here, so
    #    that the miss is one of the bound and not of a NaN)
    flat = EMU.wide_bias(bias, bias.shape[1] + 2, fill=7.5).reshape(-1)
    packed = flat[:bias.size].reshape(bias.shape)
    assert misses(EMU.edge_reference(mat, packed, Q, K, V, dO)[0], EMU.EDGE_NAMES) == list(EMU.EDGE_NAMES)
    # and the NaN padding the emulation really uses poisons what such a kernel writes
    poisoned = EMU.wide_bias(bias, bias.shape[1] + 2).reshape(-1)[:bias.size].reshape(bias.shape)
    assert np.isnan(EMU.edge_reference(mat, poisoned, Q, K, V, dO)[0][0]).any()


def test_the_first_order_condition_of_the_float64_comparison():
    """STAGES rho <= FIRST_ORDER (8 and 2**-6, tests/test_gpu_attention_autograd.py) for the cases of
    tests/test_gpu_mha_edge_bias.py's float64 comparison: rho is a function of the inputs, so it is judged here, in numpy; and it
    is not above the biased call's rho for the same scores (one rounding fewer: the module docstring of edge_bias_reference)."""
    from tests import mha_bias_reference as B
    F_HEADS = EB.F_HEADS
    for mat, seed in ((E.class_edges(), EB.F_SEEDS["class-edges"]), (EB.random_matrix(), EB.F_SEEDS["random"])):
        for dtype in (np.float64, np.float32):
            bias, c, (Q, K, _, _) = EB.case(mat, F_HEADS, EB.F_K, EB.F_D, dtype, seed)
            rho = EB.first_order_rho(mat, c, bias, Q, K, dtype)
            print(f"{mat.name} {np.dtype(dtype).name}: rho {rho:.3e}")
            assert 8 * rho <= 2.0 ** -6, (mat.name, rho)
            for h in range(F_HEADS):  # (head by head: the biased rho of that head's column as values with slope 1)
                one = B.first_order_rho(mat, c, bias[:, h], np.ones(1), Q[:, h:h + 1], K[:, h:h + 1], dtype)
                assert EB.first_order_rho(mat, c, bias[:, h:h + 1], Q[:, h:h + 1], K[:, h:h + 1], dtype) <= one
