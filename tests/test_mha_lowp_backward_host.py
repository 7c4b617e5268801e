"""csr5hip_mha_lowp_backward on the host side (no GPU): the C ABI symbol and its declaration, the C++ class member, the return codes
and their order -- tests/test_attention_entry_points_host.py's mistakes, made in this call with the same codes --, the Python
argument checks of ``mhaLowpBackward``, the routing of the 16-bit autograd backward by the handle's dtype, the host emulation of the
kernel source under the address and undefined-behaviour sanitizers (a stand-alone program), and the conditions of
tests/test_gpu_mha_lowp_backward.py's float64 comparison that are functions of the inputs alone."""
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
from tests import lowp_backward_reference as LB
from tests import lowp_reference as L
from tests import test_attention_entry_points_host as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
NAME = "csr5hip_mha_lowp_backward"
DECL = ("int csr5hip_mha_lowp_backward(csr5hip_handle h, int operand_type, int heads, double scale, const void *d_B, int ldb, "
        "const void *d_Q, int ldq, const void *d_K, int ldk, int k, const void *d_V, int ldv, int d, "
        "const void *d_dO, int lddo, void *d_dQ, int lddq, void *d_dK, int lddk, void *d_dV, int lddv, "
        "void *d_work, void *d_dB, int lddb);")
ROW = ("handle", "type", "heads", "scale", "B", "ldb") + T._BWD + ("dS", "ldds")  # the row this call would have in T.ENTRIES


def test_library_exports_the_symbol_with_the_declared_signature():
    import torch  # noqa: F401  (one HIP runtime per process: see _capi.load)
    lib = C.CDLL(_capi.LIB_PATH)
    with open(os.path.join(INC, "csr5hip_lowp.h")) as f:
        text = re.sub(r"\s+", " ", f.read())
    assert hasattr(lib, NAME) and DECL in text
    p, i, dbl = C.c_void_p, C.c_int, C.c_double
    assert _capi.SYMBOLS_LOWP_BACKWARD == [(NAME, i, [p, i, i, dbl, p, i, p, i, p, i, i, p, i, i, p, i, p, i, p, i, p, i, p, p, i])]
    assert _capi.load().csr5hip_mha_lowp_backward.argtypes == _capi.SYMBOLS_LOWP_BACKWARD[0][2]  # load() binds it
    others = _capi.SYMBOLS + _capi.SYMBOLS_BIASED + _capi.SYMBOLS_EDGE_BIAS + _capi.SYMBOLS_LOWP
    assert NAME not in {n for n, _, _ in others}  # (the other lists are as they were)
    argtypes = _capi.SYMBOLS_LOWP_BACKWARD[0][2]
    assert len(argtypes) == len(ROW)
    for arg, ctype in zip(ROW, argtypes):
        integer = arg in ("type", "heads", "k", "d") or arg.startswith("ld")
        assert ctype is (dbl if arg == "scale" else i if integer else p), arg


def test_cpp_class_has_the_member(tmp_path):
    src = tmp_path / "use_mha_lowp_backward.cpp"
    src.write_text(
        '#include "anonymouslib_hip.h"\n'
        "int use(anonymouslibHandle<int, unsigned, double> &A, anonymouslibHandle<int, unsigned, float> &A32, const void *B, const void *Q,\n"
        "        const void *K, const void *V, const void *dO, void *dQ, void *dK, void *dV, float *work, void *dB)\n"
        "{ return A.mhaLowpBackward(CSR5HIP_BF16, 4, 0.25, B, 6, Q, 64, K, 64, 16, V, 64, 16, dO, 64, dQ, 64, dK, 64, dV, 64, work, dB, 4)\n"
        "       + A32.mhaLowpBackward(CSR5HIP_F16, 4, 1.0, nullptr, 4, Q, 64, K, 64, 16, V, 64, 16, dO, 64, dQ, 64, nullptr, 64, nullptr, 64,\n"
        "                             nullptr, nullptr, 4); }\n")
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", f"-I{INC}", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


class _Entry(T.Entry):
    """T.Entry for the call that T.ENTRIES does not hold"""

    def __init__(self, lib, handle):
        self.fn, self.name, self.args = getattr(lib, NAME), NAME, ROW
        self.heads = T.HEADS
        self.good = dict(handle=handle, type=_capi.BF16, heads=self.heads, scale=0.5, B=T.FAKE, ldb=self.heads, Q=T.FAKE, K=T.FAKE,
                         V=T.FAKE, dO=T.FAKE, k=T.K, d=T.D, dQ=T.FAKE, dK=None, dV=None, work=None, dS=None, ldds=self.heads)
        for ld, (width, _) in T.LEADING.items():
            if width and ld in ROW:
                self.good[ld] = self.heads * self.good[width]


@pytest.mark.parametrize("value_type", (_capi.F64, _capi.F32), ids=("fp64-handle", "fp32-handle"))
def test_return_codes_in_order_without_a_gpu(value_type):
    """tests/test_attention_entry_points_host.py's two tests on this call: every mistake made there, the same code; the handle, then
    the operand type, then csr5hip_mha_edge_bias_backward's list; the missing companion under this call's own name; get_info the same
    bytes throughout.  The handle's value type plays no part."""
    lib = _capi.load()
    h = C.c_void_p()
    assert lib.csr5hip_create(C.byref(h), T.M, T.N, value_type) == 0
    e, other = _Entry(lib, h), T.Entry(lib, h, "csr5hip_mha_edge_bias_backward")
    before = T._info_bytes(lib, h)
    T._argument_mistakes(e, T.UNK)                                  # before inputCSR: the unknown format
    assert e.call(Q=None, K=None, V=None) == T.UNK
    assert T._missing_companion(e, other, dK=T.FAKE, work=T.FAKE) and T._missing_companion(e, other, dV=T.FAKE, work=T.FAKE)
    assert e.call(dK=T.FAKE, dV=T.FAKE) == T.INV
    assert e.call(type=7, dK=T.FAKE, work=T.FAKE) == T.TYPE         # the type comes before the companion too
    assert T._info_bytes(lib, h) == before
    assert lib.csr5hip_input_csr(h, T.NNZ, None, None, None) == 0   # CSR format, nnz > 0
    before = T._info_bytes(lib, h)
    T._argument_mistakes(e, T.CSR)
    for operand in ("Q", "K", "V", "dO"):
        assert e.call(**{operand: None}) == T.INV, operand
        assert e.call(type=0, **{operand: None}) == T.TYPE, operand
    assert e.call(B=None) == T.CSR                                  # optional
    assert T._missing_companion(e, other, dK=T.FAKE, work=T.FAKE) and T._missing_companion(e, other, dV=T.FAKE, work=T.FAKE)
    assert T._missing_companion(e, other, dQ=None, dK=T.FAKE, dV=T.FAKE, work=T.FAKE)
    assert T._missing_companion(e, other, heads=0, dK=T.FAKE)
    for changes in (dict(dK=T.FAKE), dict(dV=T.FAKE), dict(dK=T.FAKE, work=T.FAKE, Q=None), dict(dV=T.FAKE, work=T.FAKE, dO=None)):
        assert other.call(dK=T.FAKE, work=T.FAKE) == T.INV
        text = _capi.last_error()
        assert e.call(**changes) == T.INV and _capi.last_error() == text and NAME + ":" not in text, changes
    assert e.call(dQ=None, Q=None, K=None, V=None, dO=None) == T.CSR
    assert e.call(dQ=None, k=-1) == T.INV and e.call(dQ=None, ldq=e.good["ldq"] - 1) == T.INV
    assert e.call(dQ=None, dS=T.FAKE) == T.CSR and e.call(dQ=None, dS=T.FAKE, Q=None) == T.INV
    assert T._info_bytes(lib, h) == before
    assert lib.csr5hip_free(h) == 0


def test_python_method_rejects_bad_tensors_before_the_library():
    torch = pytest.importorskip("torch")
    for handle_dtype in ("float64", "float32"):
        A = H.anonymouslibHandle(6, 4, dtype=handle_dtype)
        calls = []
        A.mha_lowp_backward_ptr = lambda *a: calls.append(a) or 0  # nothing may reach the library
        for dt, other in ((torch.bfloat16, torch.float16), (torch.float16, torch.bfloat16)):
            z = lambda *s: torch.zeros(*s, dtype=dt)  # noqa: E731
            good = dict(Q=z(6, 2, 3), K=z(4, 2, 3), V=z(4, 2, 5), dO=z(6, 2, 5), dQ=z(6, 2, 3))
            col = dict(good, dK=z(4, 2, 3), dV=z(4, 2, 5), work=torch.zeros(48))
            if A._nnz is None:
                with pytest.raises(ValueError, match="inputCSR"):
                    A.mhaLowpBackward(**good)
                assert A.inputCSR(7, None, None, None) == 0
            with pytest.raises(ValueError, match="GPU"):
                A.mhaLowpBackward(**good)                                  # host tensors: everything else is in order
            with pytest.raises(ValueError, match="GPU"):
                A.mhaLowpBackward(**col, B=z(7, 2), scale=0.5, dB=z(7, 2))
            for bad in (torch.zeros(6, 2, 3), torch.zeros(6, 2, 3, dtype=torch.float64), np.zeros((6, 2, 3)), None):
                with pytest.raises(ValueError, match="Q must be a torch.bfloat16 or torch.float16 tensor"):
                    A.mhaLowpBackward(**dict(good, Q=bad))
            for name in ("K", "V", "dO", "dQ"):                            # all of one 16-bit type: neither the other one nor fp32
                for wrong in (other, torch.float32):
                    with pytest.raises(ValueError, match=f"{name} has dtype .*Q has {dt}"):
                        A.mhaLowpBackward(**dict(good, **{name: good[name].to(wrong)}))
            for name in ("dK", "dV"):
                with pytest.raises(ValueError, match=f"{name} has dtype .*Q has {dt}"):
                    A.mhaLowpBackward(**dict(col, **{name: col[name].float()}))
            # the workspace: float32 whatever the operands and the handle hold, 4 m H values, contiguous, there when dK or dV is
            for bad, word in ((z(48), "float32"), (torch.zeros(48, dtype=torch.float64), "float32"), (torch.zeros(47), "shape"),
                              (torch.zeros(6, 8), "shape"), (torch.zeros(96)[::2], "contiguous"), (None, "work must be a torch tensor")):
                with pytest.raises(ValueError, match=word):
                    A.mhaLowpBackward(**dict(col, work=bad))
            with pytest.raises(ValueError, match="Q has 2 heads, dO 3"):
                A.mhaLowpBackward(**dict(good, dO=z(6, 3, 5)))
            with pytest.raises(ValueError, match="dQ shares storage with K"):
                pool = z(6 * 2 * 3 + 4 * 2 * 3)
                A.mhaLowpBackward(**dict(good, K=pool[:24].view(4, 2, 3), dQ=pool[24:].view(6, 2, 3)))
            for bad in (float("nan"), float("inf"), None, "1", True):
                with pytest.raises(ValueError, match="scale"):
                    A.mhaLowpBackward(**good, scale=bad)
            for which in ("B", "dB"):
                for bad, word in ((np.zeros((7, 2)), "tensor"), (z(7), "shape"), (torch.zeros(7, 2), "dtype"), (z(7, 2).to(other), "dtype"),
                                  (z(6, 2), "shape"), (z(7, 4)[:, ::2], "stride\\(1\\)"), (z(1, 2).expand(7, 2), "overlap"), (z(7, 2), "GPU")):
                    with pytest.raises(ValueError, match=f" {which} .*{word}"):
                        A.mhaLowpBackward(**good, **{which: bad})
            with pytest.raises(ValueError, match="dB shares a storage with B"):
                pool = z(14, 2)
                A.mhaLowpBackward(**good, B=pool[:7], dB=pool[7:])
        assert calls == []
        A.close()


class _Info:
    transpose_built = 1


class _FakeHandle:
    """what _LowpMultiheadAttention.backward touches of a handle, recording the calls"""

    def __init__(self, vt, log):
        self._vt, self._m, self._n, self._nnz, self.log = vt, 6, 4, 7, log

    def setStream(self, s):
        return 0

    def info(self):
        return _Info()

    def mhaLowpBackward(self, Q, K, V, dO, dQ, dK, dV, work, B=None, scale=1.0, dB=None):
        self.log.append(("lowp", tuple(t.dtype for t in (Q, K, V, dO)), [None if t is None else t.dtype for t in (dQ, dK, dV, work, B, dB)]))
        return 0

    def mhaEdgeBiasBackward(self, Q, K, V, dO, dQ, dK, dV, work, B=None, scale=1.0, dB=None):
        self.log.append(("edge", tuple(t.dtype for t in (Q, K, V, dO)), [None if t is None else t.dtype for t in (dQ, dK, dV, work, B, dB)]))
        return 0


def test_the_16_bit_backward_is_routed_by_the_handles_dtype(monkeypatch):
    torch = pytest.importorskip("torch")
    from benchmark_spmv_using_csr5_amd import autograd
    monkeypatch.setattr(autograd, "_on_current_stream", lambda A, device: None)

    class Ctx:
        pass
    for dt in (torch.bfloat16, torch.float16):
        z = lambda *s: torch.zeros(*s, dtype=dt)  # noqa: E731
        for vt, wide in ((_capi.F32, torch.float32), (_capi.F64, torch.float64)):
            for need, has_bias in (((True, True, True), True), ((True, False, False), True), ((False, False, True), False)):
                log = []
                ctx = Ctx()
                ctx.A, ctx.scale, ctx.has_bias = _FakeHandle(vt, log), 0.5, has_bias
                ctx.needs_input_grad = (False,) + need + (False, has_bias)
                ctx.saved_tensors = (z(6, 2, 3), z(4, 2, 3), z(4, 2, 5)) + ((z(7, 2),) if has_bias else ())
                grads = autograd._LowpMultiheadAttention.backward(ctx, z(6, 2, 5))
                assert len(log) == 1 and len(grads) == 6
                route, ins, outs = log[0]
                column = need[1] or need[2]
                if vt == _capi.F32:  # ONE mhaLowpBackward on the 16-bit tensors, a float32 workspace only for dK / dV, no widened copy
                    assert route == "lowp" and ins == (dt,) * 4
                    assert outs == [dt if n else None for n in need] + [torch.float32 if column else None, dt if has_bias else None,
                                                                        dt if has_bias else None]
                else:                # the stopgap as it was: everything widened to fp64
                    assert route == "edge" and ins == (wide,) * 4
                    assert outs == [wide if n else None for n in need] + [wide if column else None, wide if has_bias else None,
                                                                          wide if has_bias else None]
                for g, n in zip(grads[1:4], need):
                    assert (g is not None) == n and (g is None or g.dtype == dt)
                assert (grads[5] is not None) == has_bias and (grads[5] is None or grads[5].dtype == dt)
            # nothing runs when no input needs a gradient
            log = []
            ctx = Ctx()
            ctx.A, ctx.scale, ctx.has_bias = _FakeHandle(vt, log), 0.5, True
            ctx.needs_input_grad = (False,) * 6
            ctx.saved_tensors = (z(6, 2, 3), z(4, 2, 3), z(4, 2, 5), z(7, 2))
            assert autograd._LowpMultiheadAttention.backward(ctx, z(6, 2, 5)) == (None,) * 6 and log == []
    for text in (autograd.__doc__, autograd.multihead_attention.__doc__):
        assert "mhaLowpBackward" in text and "stopgap" in text.lower() and "fp64" in text


def _sanitizers_link(cxx, tmp_path):
    src = tmp_path / "probe.cpp"
    src.write_text("int main() { return 0; }\n")
    r = subprocess.run([cxx, "-fsanitize=address,undefined", str(src), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    return r.returncode == 0 and subprocess.run([str(tmp_path / "probe")]).returncode == 0


def test_host_emulation_under_the_sanitizers(tmp_path):
    """scripts/host_emulation/run_mha_lowp_backward.py: a stand-alone program built from the kernel source with
    -fsanitize=address,undefined; kat0 and duplicates, one head and three, (k, d) = (3, 5) and (16, 16) (element loads; 16-byte loads
    in the unpadded configurations), both operand types.  Every operand, output, B, dB, the workspace and the map is a heap block of
    exactly its declared size.  --wrong: the word comparison rejects the modelled kernel whose workspace is kept in 16 bits, in both
    types; the kernel that rounds the exact result once differs from the right one in about one word in 2^15 (bf16) or 2^12 (fp16),
    too rarely for these matrices, so the script reports its count and ``test_the_expectation_tells_one_rounding_from_two`` shows
    on constructed ties that the expectation is not that kernel's."""
    cxx = "/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else "clang++"
    try:
        linked = _sanitizers_link(cxx, tmp_path)
    except OSError:
        linked = False
    if not linked:
        pytest.skip(f"{cxx} cannot link a program with -fsanitize=address,undefined (no sanitizer runtime)")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "host_emulation", "run_mha_lowp_backward.py"), "--matrices",
                        "kat0,duplicates", "--heads", "1,3", "--kd", "3x5,16x16", "--types", "bf16,f16", "--cxx", cxx, "--wrong"],
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.count(": ok") == 16 and r.stdout.count("heads=3 k=16 d=16: ok") == 4, r.stdout
    assert r.stdout.count(": wrong kernel exact-once,") == 16 and r.stdout.count(": wrong kernel work16,") == 16, r.stdout
    assert "wrong kernel work16 bf16: rejected" in r.stdout and "wrong kernel work16 f16: rejected" in r.stdout, r.stdout
    assert "wrong kernel exact-once bf16:" in r.stdout and "wrong kernel exact-once f16:" in r.stdout, r.stdout


def test_the_expectation_tells_one_rounding_from_two():
    """the kernel whose last multiplication is folded into the conversion stores the EXACT product rounded once; the definition
    stores the float product rounded.  They differ where the float product is a tie of the operand type and the exact one is not:
    x = tie +- 2^-30 relative.  ``round_once`` (the script's model of the wrong kernel) goes to the side the exact value lies on, the
    expectation ``to_words(float32(x))`` to the even neighbour; away from ties both agree."""
    sys.path.insert(0, ROOT)
    from scripts.host_emulation.emulation import round_once
    for kind, bits in (("bf16", 8), ("f16", 11)):
        ulp = 2.0 ** (1 - bits)                                    # of the operand type in [1, 2)
        even, odd = 1.0 + 2 * ulp, 1.0 + 3 * ulp                   # neighbours; the tie between them is 1 + 2.5 ulp
        tie = 1.0 + 2.5 * ulp
        above, below = tie * (1 + 2.0 ** -30), tie * (1 - 2.0 ** -30)
        assert np.float32(above) == np.float32(tie) == np.float32(below)  # the float rounding lands on the tie
        w = lambda v: L.widen(v, kind).astype(np.float64)  # noqa: E731
        two = w(L.to_words(np.array([above, below], dtype=np.float64).astype(np.float32), kind))
        one = w(round_once(np.array([above, below]), kind))
        assert two.tolist() == [even, even] and one.tolist() == [odd, even]
        x = np.random.default_rng(4).uniform(-2, 2, 200000)
        same = round_once(x, kind) == L.to_words(x.astype(np.float32), kind)
        assert same.mean() > 0.999 and (kind == "bf16" or not same.all())  # (fp16: some of 200 000 are such near-ties)


@pytest.mark.parametrize("kind", L.KINDS)
def test_the_conditions_of_the_float64_comparison(kind):
    """for the inputs of tests/test_gpu_mha_lowp_backward.py's float64 comparison, in numpy: STAGES rho <= FIRST_ORDER (8 and 2**-6,
    tests/test_gpu_attention_autograd.py) with rho the fp32 rho of tests/edge_bias_reference.py on the widened operands; the operands
    lie in [-1, 1]; the forward operands are tests/lowp_reference.f64_case's words"""
    for mat in (E.class_edges(), EB.random_matrix()):
        words, c = LB.f64_case(mat, kind, EB.F_HEADS, EB.F_K, EB.F_D)
        fwd, c0 = L.f64_case(mat, kind, EB.F_HEADS, EB.F_K, EB.F_D)
        assert c == c0 and all(np.array_equal(a, b) for a, b in zip(words[:4], fwd))
        assert words[4].shape == (mat.m, EB.F_HEADS, EB.F_D)
        for w in words:
            t = L.widen(w, kind)
            assert np.isfinite(t).all() and np.abs(t).max() <= 1.0
        rho = LB.rho(mat, kind, EB.F_HEADS, EB.F_K, EB.F_D)
        print(f"{mat.name} {kind}: rho {rho:.3e}")
        assert 8 * rho <= 2.0 ** -6, (mat.name, rho)


def test_the_masked_bias_masks_one_head_only():
    mat = E.class_edges()
    for kind in L.KINDS:
        words = L.to_words(np.random.default_rng(1).uniform(-2, 2, size=(mat.nnz, 3)).astype(np.float32), kind)
        out, row = LB.masked_bias(mat, words, kind)
        ninf = np.isneginf(L.widen(out, kind))
        a, b = int(mat.row_ptr[row]), int(mat.row_ptr[row + 1])
        assert b - a >= 2 and ninf[a:b, 0].all() and not ninf[:, 1:].any() and ninf[::7, 0].all()
        assert np.array_equal(out[~ninf], words[~ninf])
