"""csr5hip_mha_lowp on the host side (no GPU): the C ABI symbol and its declaration, the C++ class member, the return codes and
their order, the Python argument checks of ``mhaLowp``, the routing of ``autograd.multihead_attention`` by Q's dtype, the bf16
conversion of tests/lowp_reference.py against torch's, the host emulation of the kernel source under the address and
undefined-behaviour sanitizers (a stand-alone program), and the conditions of tests/test_gpu_mha_lowp.py's float64 comparison that
are functions of the inputs alone."""
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
from tests import edge_bias_reference as EB
from tests import lowp_reference as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
DECL = ("int csr5hip_mha_lowp(csr5hip_handle h, int operand_type, int heads, double scale, const void *d_B, int ldb, "
        "const void *d_Q, int ldq, const void *d_K, int ldk, int k, const void *d_V, int ldv, int d, void *d_O, int ldo);")


def test_library_exports_the_symbol_with_the_declared_signature():
    import torch  # noqa: F401  (one HIP runtime per process: see _capi.load)
    lib = C.CDLL(_capi.LIB_PATH)
    with open(os.path.join(INC, "csr5hip.h")) as f:
        assert '#include "csr5hip_lowp.h"' in f.read()  # (csr5hip.h brings the declaration in: users include that header)
    with open(os.path.join(INC, "csr5hip_lowp.h")) as f:
        text = re.sub(r"\s+", " ", f.read())
    assert hasattr(lib, "csr5hip_mha_lowp") and DECL in text
    assert "#define CSR5HIP_BF16 2" in text and "#define CSR5HIP_F16 3" in text
    assert (_capi.BF16, _capi.F16) == (2, 3) and not {_capi.BF16, _capi.F16} & {_capi.F64, _capi.F32}
    p, i, dbl = C.c_void_p, C.c_int, C.c_double
    assert _capi.SYMBOLS_LOWP == [("csr5hip_mha_lowp", i, [p, i, i, dbl, p, i, p, i, p, i, i, p, i, i, p, i])]
    assert _capi.load().csr5hip_mha_lowp.argtypes == _capi.SYMBOLS_LOWP[0][2]  # load() binds it
    others = _capi.SYMBOLS + _capi.SYMBOLS_BIASED + _capi.SYMBOLS_EDGE_BIAS
    assert "csr5hip_mha_lowp" not in {n for n, _, _ in others}  # (the other lists are as they were)


def test_cpp_class_has_the_member(tmp_path):
    src = tmp_path / "use_mha_lowp.cpp"
    src.write_text(
        '#include "anonymouslib_hip.h"\n'
        "int use(anonymouslibHandle<int, unsigned, double> &A, anonymouslibHandle<int, unsigned, float> &A32, const void *B, const void *Q,\n"
        "        const void *K, const void *V, void *O)\n"
        "{ return A.mhaLowp(CSR5HIP_BF16, 4, 0.25, B, 6, Q, 64, K, 64, 16, V, 64, 16, O, 64)\n"
        "       + A32.mhaLowp(CSR5HIP_F16, 4, 1.0, nullptr, 4, Q, 64, K, 64, 16, V, 64, 16, O, 64); }\n")
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", f"-I{INC}", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _info_bytes(lib, h):
    info = _capi.Csr5Info()
    assert lib.csr5hip_get_info(h, C.byref(info)) == 0
    return bytes(info)


@pytest.mark.parametrize("value_type", (_capi.F64, _capi.F32), ids=("fp64-handle", "fp32-handle"))
def test_return_codes_in_order_without_a_gpu(value_type):
    """Decided on the host, with fake non-null pointers: the handle; the operand type; then csr5hip_mha_edge_bias's list (the first
    arguments and the scale, the leading dimensions with ldb < heads when B is given, the null operands, the format); get_info
    unchanged throughout.  The handle's value type plays no part."""
    lib = _capi.load()
    h = C.c_void_p()
    assert lib.csr5hip_create(C.byref(h), 10, 12, value_type) == 0
    f = C.c_void_p(64)
    INV, CSR, UNK, TYP = _capi.INVALID_ARGUMENT, _capi.UNSUPPORTED_CSR_SPMV, _capi.UNKOWN_FORMAT, _capi.UNSUPPORTED_VALUE_TYPE

    def call(ot=_capi.BF16, heads=3, scale=0.5, B=f, ldb=3, Q=f, ldq=12, K=f, ldk=12, k=4, V=f, ldv=15, d=5, O=f, ldo=15, handle=h):
        return lib.csr5hip_mha_lowp(handle, ot, heads, scale, B, ldb, Q, ldq, K, ldk, k, V, ldv, d, O, ldo)
    before = _info_bytes(lib, h)
    assert call(handle=None) == INV and call(handle=None, ot=9) == INV            # the handle comes before the operand type
    for bad in (_capi.F64, _capi.F32, 4, -1, 1 << 20):
        assert call(ot=bad) == TYP
        assert call(ot=bad, heads=-1) == TYP and call(ot=bad, scale=float("nan")) == TYP and call(ot=bad, ldq=0) == TYP  # ... before all else
    for ot in (_capi.BF16, _capi.F16):
        assert call(ot=ot) == UNK and call(ot=ot, B=None) == UNK                  # before inputCSR; B may be null
        assert call(ot=ot, Q=None, K=None, V=None) == UNK and call(ot=ot, heads=0) == UNK
        assert call(ot=ot, heads=-1) == INV and call(ot=ot, k=-1) == INV and call(ot=ot, d=-1) == INV
        for bad in (float("nan"), float("inf"), -float("inf")):
            assert call(ot=ot, scale=bad) == INV                                  # the scale comes before the format
        assert call(ot=ot, scale=0.0) == UNK and call(ot=ot, scale=-3.0) == UNK
        assert call(ot=ot, ldb=2) == INV and call(ot=ot, ldb=7) == UNK and call(ot=ot, B=None, ldb=0) == UNK
    assert lib.csr5hip_input_csr(h, 100, None, None, None) == 0                   # CSR format, nnz > 0
    before = _info_bytes(lib, h)
    assert call() == CSR and call(heads=0) == CSR and call(B=None) == CSR and call(ot=_capi.F16) == CSR
    for bad in (dict(heads=-1), dict(k=-1), dict(d=-1), dict(scale=float("nan")), dict(ldq=11), dict(ldk=11), dict(ldv=14), dict(ldo=14),
                dict(ldb=2), dict(Q=None), dict(K=None), dict(V=None), dict(O=None)):
        assert call(**bad) == INV, bad
        assert call(ot=0, **bad) == TYP, bad
    assert call(Q=None, ldb=2) == INV and call(Q=None, K=None, k=0) == CSR        # k = 0 needs neither Q nor K
    assert _info_bytes(lib, h) == before
    assert lib.csr5hip_free(h) == 0


def test_python_method_rejects_bad_tensors_before_the_library():
    torch = pytest.importorskip("torch")
    for handle_dtype in ("float64", "float32"):
        A = H.anonymouslibHandle(6, 4, dtype=handle_dtype)
        calls = []
        A.mha_lowp_ptr = lambda *a: calls.append(a) or 0  # nothing may reach the library
        for dt, other in ((torch.bfloat16, torch.float16), (torch.float16, torch.bfloat16)):
            z = lambda *s: torch.zeros(*s, dtype=dt)  # noqa: E731
            good = dict(Q=z(6, 2, 3), K=z(4, 2, 3), V=z(4, 2, 5), O=z(6, 2, 5))
            if A._nnz is None:
                with pytest.raises(ValueError, match="inputCSR"):
                    A.mhaLowp(**good)
                assert A.inputCSR(7, None, None, None) == 0
            with pytest.raises(ValueError, match="GPU"):
                A.mhaLowp(**good)                                          # host tensors: everything else is in order
            with pytest.raises(ValueError, match="GPU"):
                A.mhaLowp(**good, B=z(7, 2), scale=0.5)
            for bad in (torch.zeros(6, 2, 3), torch.zeros(6, 2, 3, dtype=torch.float64), np.zeros((6, 2, 3)), None):
                with pytest.raises(ValueError, match="Q must be a torch.bfloat16 or torch.float16 tensor"):
                    A.mhaLowp(**dict(good, Q=bad))
            for name in ("K", "V", "O"):                                   # all of one 16-bit type: neither the other one nor fp32
                for wrong in (other, torch.float32):
                    with pytest.raises(ValueError, match=f"{name} has dtype .*Q has {dt}"):
                        A.mhaLowp(**dict(good, **{name: good[name].to(wrong)}))
            with pytest.raises(ValueError, match="Q has 2 heads, K 3"):
                A.mhaLowp(**dict(good, K=z(4, 3, 3)))
            with pytest.raises(ValueError, match="V .*stride"):
                A.mhaLowp(**dict(good, V=z(4, 2, 10)[:, :, ::2]))
            with pytest.raises(ValueError, match="O shares storage with Q"):
                pool = z(6 * 2 * 8)
                A.mhaLowp(**dict(good, Q=pool[:36].view(6, 2, 3), O=pool[36:96].view(6, 2, 5)))
            for bad in (float("nan"), float("inf"), None, "1", True, z(1)):
                with pytest.raises(ValueError, match="scale"):
                    A.mhaLowp(**good, scale=bad)
            for bad, word in ((np.zeros((7, 2)), "tensor"), (z(7), "shape"), (torch.zeros(7, 2), "dtype"), (z(7, 2).to(other), "dtype"),
                              (z(6, 2), "shape"), (z(7, 4)[:, ::2], "stride\\(1\\)"), (z(7, 1), "shape"), (z(7, 3), "shape"),
                              (z(1, 2).expand(7, 2), "overlap"), (z(7, 2), "GPU")):
                with pytest.raises(ValueError, match=f" B .*{word}"):
                    A.mhaLowp(**good, B=bad)
        assert calls == []
        # the existing methods keep rejecting 16-bit tensors
        h16 = lambda *s: torch.zeros(*s, dtype=torch.bfloat16)  # noqa: E731
        for method in (A.mha, A.mhaEdgeBias, A.mhaBiased):
            with pytest.raises(ValueError, match="Q has dtype torch.bfloat16, the handle holds"):
                method(h16(6, 2, 3), h16(4, 2, 3), h16(4, 2, 5), h16(6, 2, 5))
        A.close()


def test_multihead_attention_routes_16_bit_operands(monkeypatch):
    torch = pytest.importorskip("torch")
    from benchmark_spmv_using_csr5_amd import autograd
    seen = []
    monkeypatch.setattr(autograd._LowpMultiheadAttention, "apply", staticmethod(lambda *a: seen.append(("lowp", a[4], a[5] is None))))
    monkeypatch.setattr(autograd._EdgeBiasMultiheadAttention, "apply", staticmethod(lambda *a: seen.append(("edge",))))
    monkeypatch.setattr(autograd._MultiheadAttention, "apply", staticmethod(lambda *a: seen.append(("plain",))))
    for dt in (torch.bfloat16, torch.float16):
        Q, two = torch.zeros(6, 2, 3, dtype=dt), torch.zeros(7, 2, dtype=dt)
        autograd.multihead_attention(None, Q, None, None)
        autograd.multihead_attention(None, Q, None, None, scale=0.5, bias=two)
        for kw in (dict(bias=torch.zeros(7, dtype=dt)), dict(slopes=torch.ones(2, dtype=dt)), dict(bias=two, slopes=torch.ones(2, dtype=dt))):
            with pytest.raises(ValueError, match="1-D bias and slopes"):
                autograd.multihead_attention(None, Q, None, None, **kw)
    autograd.multihead_attention(None, torch.zeros(6, 2, 3), None, None)                           # fp32: the routes that were
    autograd.multihead_attention(None, torch.zeros(6, 2, 3), None, None, bias=torch.zeros(7, 2))
    assert seen == [("lowp", 1.0, True), ("lowp", 0.5, False)] * 2 + [("plain",), ("edge",)]
    for text in (autograd.__doc__, autograd.multihead_attention.__doc__):
        assert "mhaLowp" in text and "stopgap" in text.lower()


def test_the_bf16_conversion_agrees_with_torch():
    """finite values only: every rounding case (ties to even, both ways; the carry into the exponent; overflow to Inf; subnormals) and
    a random sweep, against ``torch.Tensor.to(torch.bfloat16)`` on the CPU; ``widen`` is the exact inverse"""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(3)
    special = np.array([0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x3FFF8000, 0x7F7F8000, 0x7F7FFFFF, 0x00008000, 0x00018000,
                        0x00000001, 0x80000000, 0x00000000, 0xBF808000, 0x7F7F7FFF], dtype=np.uint32).view(np.float32)
    bits = rng.integers(0, 1 << 32, size=200000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    x = np.concatenate([special, bits[np.isfinite(bits)], rng.uniform(-2, 2, 50000).astype(np.float32)])
    want = torch.from_numpy(x).to(torch.bfloat16)
    assert np.array_equal(L.to_words(x, "bf16"), want.view(torch.int16).numpy().view(np.uint16))
    assert np.array_equal(L.widen(L.to_words(x, "bf16"), "bf16").view(np.uint32), want.float().numpy().view(np.uint32))
    half = torch.from_numpy(x).to(torch.float16)
    assert np.array_equal(L.to_words(x, "f16"), half.view(torch.int16).numpy().view(np.uint16))
    # NaN: one quiet NaN, compared positionally
    nan = np.array([np.nan, 1.0], dtype=np.float32)
    for kind in L.KINDS:
        w = L.to_words(nan, kind)
        assert w[0] == L.NAN_WORD[kind] and L.is_nan(w, kind).tolist() == [True, False]
        assert L.same_words(w, np.array([0xFFFF, w[1]], dtype=np.uint16), kind) and not L.same_words(w, np.array([w[0], w[1] ^ 1], dtype=np.uint16), kind)


def _sanitizers_link(cxx, tmp_path):
    src = tmp_path / "probe.cpp"
    src.write_text("int main() { return 0; }\n")
    r = subprocess.run([cxx, "-fsanitize=address,undefined", str(src), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    return r.returncode == 0 and subprocess.run([str(tmp_path / "probe")]).returncode == 0


def test_host_emulation_under_the_sanitizers(tmp_path):
    """scripts/host_emulation/run_mha_lowp.py: a stand-alone program built from the kernel source with -fsanitize=address,undefined;
    kat0 and duplicates, one head and three, (k, d) = (3, 5) and (16, 16) (element loads; 16-byte loads in the unpadded
    configurations), both operand types, padded leading dimensions in one configuration of three.  Every operand is a heap block of
    exactly rows * ld 2-byte elements.  Measured on one machine: 90 s, of which about 25 s build the program."""
    cxx = "/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else "clang++"
    try:
        linked = _sanitizers_link(cxx, tmp_path)
    except OSError:
        linked = False
    if not linked:
        pytest.skip(f"{cxx} cannot link a program with -fsanitize=address,undefined (no sanitizer runtime)")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "host_emulation", "run_mha_lowp.py"), "--matrices", "kat0,duplicates",
                        "--heads", "1,3", "--kd", "3x5,16x16", "--types", "bf16,f16", "--cxx", cxx], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.count(": ok") == 16 and r.stdout.count(" bf16 ") == 8 and r.stdout.count("heads=3 k=16 d=16: ok") == 4, r.stdout


@pytest.mark.parametrize("kind", L.KINDS)
def test_the_conditions_of_the_float64_comparison(kind):
    """for the inputs of tests/test_gpu_mha_lowp.py's float64 comparison, in numpy: STAGES rho <= FIRST_ORDER (8 and 2**-6,
    tests/test_gpu_attention_autograd.py) with rho the fp32 rho of tests/edge_bias_reference.py on the widened operands; the operands
    lie in [-1, 1); and the rounding term admits the rounding of any fp32 value in the output's range but not two of them"""
    for mat in (E.class_edges(), EB.random_matrix()):
        (B, Q, K, V), c = L.f64_case(mat, kind, EB.F_HEADS, EB.F_K, EB.F_D)
        Bf, Qf, Kf, Vf = (L.widen(t, kind) for t in (B, Q, K, V))
        for t in (Bf, Qf, Kf, Vf):
            assert np.isfinite(t).all() and np.abs(t).max() <= 1.0
        rho = EB.first_order_rho(mat, c, Bf, Qf, Kf, np.float32)
        print(f"{mat.name} {kind}: rho {rho:.3e}")
        assert 8 * rho <= 2.0 ** -6, (mat.name, rho)
    x = np.random.default_rng(9).uniform(-1, 1, 100000).astype(np.float32)
    err = np.abs(L.widen(L.to_words(x, kind), kind).astype(np.float64) - x.astype(np.float64))
    assert (err <= L.round_allowance(x, kind)).all()          # one rounding fits ...
    ulp = np.abs(L.widen(L.to_words(x, kind) + np.uint16(1), kind).astype(np.float64) - L.widen(L.to_words(x, kind), kind).astype(np.float64))
    big = np.abs(x) >= 2.0 ** -10
    assert (2 * ulp[big] > L.round_allowance(x, kind)[big]).all()  # ... an error of two units in the last place does not
