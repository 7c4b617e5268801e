"""The dropped attention calls on 16-bit operands (csr5hip_dropout_lowp.h) on the host side (no GPU): the C ABI symbols and their
declarations, the C++ class members, the return codes and their order, the Python argument checks, the routing of
``autograd.dropout_attention`` by Q's dtype, and the host emulation of the two kernel sources under the address and
undefined-behaviour sanitizers (a stand-alone program)."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

from benchmark_spmv_using_csr5_amd import _capi
from benchmark_spmv_using_csr5_amd import handle as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
DECLS = {
    "csr5hip_dropout_mha_lowp": """
int csr5hip_dropout_mha_lowp(csr5hip_handle h, int operand_type, int heads, double scale, const void *d_B, int ldb,
        const void *d_Q, int ldq, const void *d_K, int ldk, int k, const void *d_V, int ldv, int d, void *d_O, int ldo,
        double p, unsigned long long seed, unsigned long long offset, int head0);
""",
    "csr5hip_dropout_mha_lowp_backward": """
int csr5hip_dropout_mha_lowp_backward(csr5hip_handle h, int operand_type, int heads, double scale, const void *d_B, int ldb,
        const void *d_Q, int ldq, const void *d_K, int ldk, int k, const void *d_V, int ldv, int d,
        const void *d_dO, int lddo, void *d_dQ, int lddq, void *d_dK, int lddk, void *d_dV, int lddv,
        void *d_work, void *d_dB, int lddb,
        double p, unsigned long long seed, unsigned long long offset, int head0);
""",
}


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_two_symbols_with_the_declared_signatures():
    import torch  # noqa: F401  (one HIP runtime per process: see _capi.load)
    lib = C.CDLL(_capi.LIB_PATH)
    with open(os.path.join(INC, "csr5hip.h")) as f:
        main = f.read()
    assert '#include "csr5hip_dropout_lowp.h"' in main  # (csr5hip.h brings the declarations in: users include that header)
    assert main.index('#include "csr5hip_lowp.h"') < main.index('#include "csr5hip_dropout_lowp.h"')  # (its operand-type constants)
    with open(os.path.join(INC, "csr5hip_dropout_lowp.h")) as f:
        raw = f.read()
    for name, decl in DECLS.items():
        assert hasattr(lib, name)
        assert decl in raw, name                                              # verbatim, line for line
    declared = sorted(set(re.findall(r"\b(csr5hip_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", raw, flags=re.S))))
    assert declared == sorted(DECLS) == sorted(n for n, _, _ in _capi.SYMBOLS_DROPOUT_LOWP)
    bound = {name: (res, args) for name, res, args in _capi.SYMBOLS_DROPOUT_LOWP}
    p, i, dbl, ull = C.c_void_p, C.c_int, C.c_double, C.c_ulonglong
    tail = [dbl, ull, ull, i]
    fwd, bwd = [p, i, p, i, i, p, i, i, p, i], [p, i, p, i, i, p, i, i, p, i, p, i, p, i, p, i, p, p, i]
    assert bound == {"csr5hip_dropout_mha_lowp": (i, [p, i, i, dbl, p, i] + fwd + tail),
                     "csr5hip_dropout_mha_lowp_backward": (i, [p, i, i, dbl, p, i] + bwd + tail)}
    loaded = _capi.load()
    for name in bound:
        assert getattr(loaded, name).argtypes == bound[name][1], name          # load() binds them
    others = (_capi.SYMBOLS + _capi.SYMBOLS_BIASED + _capi.SYMBOLS_EDGE_BIAS + _capi.SYMBOLS_LOWP + _capi.SYMBOLS_LOWP_BACKWARD
              + _capi.SYMBOLS_GAT + _capi.SYMBOLS_DROPOUT)
    assert not {n for n, _, _ in others} & set(bound)                          # (the other lists are as they were)
    for header in ("csr5hip_dropout.h", "csr5hip_lowp.h"):                     # (and so are the pinned headers)
        with open(os.path.join(INC, header)) as f:
            assert "csr5hip_dropout_mha_lowp" not in f.read(), header


def test_cpp_class_has_the_members(tmp_path):
    src = tmp_path / "use_dropout_lowp.cpp"
    src.write_text(
        '#include "anonymouslib_hip.h"\n'
        "int use(anonymouslibHandle<int, unsigned, double> &A, const void *B, const void *Q, const void *K, const void *V, const void *dO,\n"
        "        void *O, void *dQ, void *dK, void *dV, float *work, void *dB)\n"
        "{ return A.dropoutMhaLowp(CSR5HIP_BF16, 4, 0.25, B, 6, Q, 32, K, 32, 8, V, 64, 16, O, 64, 0.1, 9ull, 3ull, 2)\n"
        "       + A.dropoutMhaLowpBackward(CSR5HIP_F16, 4, 0.25, B, 6, Q, 32, K, 32, 8, V, 64, 16, dO, 64, dQ, 32, dK, 32, dV, 64, work, dB, 4,\n"
        "                                  0.1, 9ull, 3ull, 2); }\n"
        "int use32(anonymouslibHandle<int, unsigned, float> &A, const void *Q, const void *K, const void *V, void *O, void *dQ)\n"
        "{ return A.dropoutMhaLowp(CSR5HIP_F16, 4, 1.0, nullptr, 4, Q, 4, K, 4, 1, V, 64, 16, O, 64, 0.5, 1ull)\n"
        "       + A.dropoutMhaLowpBackward(CSR5HIP_BF16, 4, 1.0, nullptr, 4, Q, 4, K, 4, 1, V, 64, 16, O, 64, dQ, 4, nullptr, 4, nullptr, 64,\n"
        "                                  nullptr, nullptr, 4, 0.5, 1ull); }\n")
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", f"-I{INC}", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _info_bytes(lib, h):
    info = _capi.Csr5Info()
    assert lib.csr5hip_get_info(h, C.byref(info)) == 0
    return bytes(info)


@pytest.mark.parametrize("value_type", (_capi.F64, _capi.F32), ids=("fp64-handle", "fp32-handle"))
def test_return_codes_in_order_without_a_gpu(value_type):
    """Decided on the host, with fake non-null pointers, on a handle with null arrays (unknown format, then CSR format): the null
    handle; the operand type, before a bad p; the seven bad (p, head0) cases in the FIRST group, before the leading dimensions, the
    null operands, the companion and the format; everything after in csr5hip_dropout_mha's / csr5hip_dropout_mha_backward's order;
    get_info unchanged throughout.  The handle's value type plays no part."""
    lib = _capi.load()
    h = C.c_void_p()
    assert lib.csr5hip_create(C.byref(h), 10, 12, value_type) == 0
    f = C.c_void_p(64)
    INV, CSR, UNK, TYPE = _capi.INVALID_ARGUMENT, _capi.UNSUPPORTED_CSR_SPMV, _capi.UNKOWN_FORMAT, _capi.UNSUPPORTED_VALUE_TYPE

    def fwd(type=_capi.BF16, heads=3, scale=0.5, B=f, ldb=3, Q=f, ldq=12, K=f, ldk=12, k=4, V=f, ldv=15, d=5, O=f, ldo=15, p=0.5, seed=1,
            offset=2, head0=0, handle=h):
        return lib.csr5hip_dropout_mha_lowp(handle, type, heads, scale, B, ldb, Q, ldq, K, ldk, k, V, ldv, d, O, ldo, p, seed, offset, head0)

    def bwd(type=_capi.F16, heads=3, scale=0.5, B=f, ldb=3, Q=f, ldq=12, K=f, ldk=12, k=4, V=f, ldv=15, d=5, dO=f, lddo=15, dQ=f, lddq=12,
            dK=None, lddk=12, dV=None, lddv=15, work=None, dB=None, lddb=3, p=0.5, seed=1, offset=2, head0=0, handle=h):
        return lib.csr5hip_dropout_mha_lowp_backward(handle, type, heads, scale, B, ldb, Q, ldq, K, ldk, k, V, ldv, d, dO, lddo, dQ, lddq,
                                                     dK, lddk, dV, lddv, work, dB, lddb, p, seed, offset, head0)

    bad_drop = (dict(p=float("nan")), dict(p=float("inf")), dict(p=-float("inf")), dict(p=-0.25), dict(p=1.0), dict(p=1.5), dict(head0=-1))
    before = _info_bytes(lib, h)
    for call in (fwd, bwd):  # the unknown state: before inputCSR
        assert call(handle=None) == INV and call(handle=None, type=7) == INV   # the handle first
        for t in (_capi.F64, _capi.F32, 7, -1):
            assert call(type=t) == TYPE, t
            for bad in bad_drop:
                assert call(type=t, **bad) == TYPE, (t, bad)                   # the type before a bad p and a bad head0
            assert call(type=t, heads=-1) == TYPE and call(type=t, ldq=11) == TYPE
        for t in (_capi.BF16, _capi.F16):
            assert call(type=t) == UNK and call(type=t, B=None) == UNK and call(type=t, p=0.0) == UNK
        assert call(p=1.0 - 2.0 ** -40) == UNK
        assert call(seed=2 ** 64 - 1, offset=2 ** 64 - 1, head0=2 ** 31 - 1 - 3) == UNK
        assert call(head0=2 ** 31 - 3) == INV and call(head0=2 ** 31 - 1) == INV  # head0 + heads beyond INT_MAX
        assert call(heads=0, head0=2 ** 31 - 1) == UNK
        assert call(heads=-1) == INV and call(k=-1) == INV and call(d=-1) == INV and call(scale=float("nan")) == INV
        for bad in bad_drop:
            assert call(**bad) == INV, bad
            assert call(heads=0, **bad) == INV, bad                            # before the successful no-op of heads = 0
        assert call(ldq=11) == INV and call(ldb=2) == INV
    assert bwd(dK=f, work=f) == INV and "csr5hip_dropout_mha_lowp_backward:" in _capi.last_error()
    assert "csr5hip_build_transpose" in _capi.last_error()
    assert bwd(type=7, dK=f, work=f) == TYPE                                   # the type comes before the companion too
    assert _info_bytes(lib, h) == before
    assert lib.csr5hip_input_csr(h, 100, None, None, None) == 0                # CSR format, nnz > 0: no CSR5 structure
    before = _info_bytes(lib, h)
    for call in (fwd, bwd):
        assert call() == CSR and call(heads=0) == CSR and call(p=0.0) == CSR and call(B=None) == CSR
        assert call(type=0) == TYPE and call(type=0, Q=None) == TYPE
        for bad in bad_drop:
            assert call(**bad) == INV, bad
            assert call(Q=None, **bad) == INV and call(ldq=11, **bad) == INV   # (every one of them INVALID_ARGUMENT: the group is one)
        for bad in (dict(ldq=11), dict(ldk=11), dict(ldv=14), dict(ldb=2), dict(Q=None), dict(K=None), dict(V=None)):
            assert call(**bad) == INV, bad
    assert fwd(O=None) == INV and fwd(ldo=14) == INV
    for bad in (dict(lddq=11), dict(lddo=14), dict(dB=f, lddb=2), dict(dO=None), dict(dK=f), dict(dV=f)):
        assert bwd(**bad) == INV, bad
    assert bwd(dQ=None, dB=f) == CSR and bwd(Q=None, K=None, V=None, dO=None, dQ=None) == CSR
    # the sibling's order afterwards: the same mistakes, the same codes, the companion's message under each call's own name
    def sib(**kw):
        a = dict(heads=3, scale=0.5, B=f, ldb=3, Q=f, ldq=12, K=f, ldk=12, k=4, V=f, ldv=15, d=5, dO=f, lddo=15, dQ=f, lddq=12, dK=None,
                 lddk=12, dV=None, lddv=15, work=None, dB=None, lddb=3, p=0.5, seed=1, offset=2, head0=0)
        a.update(kw)
        return lib.csr5hip_dropout_mha_backward(h, *a.values())
    for changes in (dict(dK=f, work=f), dict(dV=f, work=f), dict(dK=f), dict(dK=f, work=f, Q=None), dict(dV=f, work=f, dO=None),
                    dict(dK=f, work=f, p=1.0), dict(heads=0, dK=f), dict(dQ=None, dB=f, Q=None), dict(lddv=14), dict(k=-1, dK=f, work=f)):
        want = sib(**changes)
        text = _capi.last_error() if want == INV else None
        got = bwd(**changes)
        assert got == want, changes
        if text and "csr5hip_build_transpose" in text and "csr5hip_dropout_mha_backward:" in text:
            assert _capi.last_error() == text.replace("csr5hip_dropout_mha_backward:", "csr5hip_dropout_mha_lowp_backward:"), changes
    assert bwd(dK=f, work=f) == INV and _capi.last_error().startswith("csr5hip_dropout_mha_lowp_backward: dK and dV need")
    assert _info_bytes(lib, h) == before
    assert lib.csr5hip_free(h) == 0


# ---- the Python layers ------------------------------------------------------------------------------------------------------------------
def test_python_methods_reject_bad_arguments_before_the_library():
    torch = pytest.importorskip("torch")
    for handle_dtype in ("float64", "float32"):
        A = H.anonymouslibHandle(6, 4, dtype=handle_dtype)
        calls = []
        for name in ("dropout_mha_lowp_ptr", "dropout_mha_lowp_backward_ptr"):
            setattr(A, name, lambda *a: calls.append(a) or 0)  # nothing may reach the library
        for dt, other in ((torch.bfloat16, torch.float16), (torch.float16, torch.bfloat16)):
            z = lambda *s: torch.zeros(*s, dtype=dt)  # noqa: E731
            fwd = dict(Q=z(6, 2, 3), K=z(4, 2, 3), V=z(4, 2, 5), O=z(6, 2, 5))
            bwd = dict(Q=z(6, 2, 3), K=z(4, 2, 3), V=z(4, 2, 5), dO=z(6, 2, 5), dQ=z(6, 2, 3), dK=z(4, 2, 3), dV=z(4, 2, 5), work=torch.zeros(48))
            methods = ((A.dropoutMhaLowp, fwd, "O"), (A.dropoutMhaLowpBackward, bwd, "dO"))
            if A._nnz is None:
                for method, good, _ in methods:
                    with pytest.raises(ValueError, match="inputCSR"):
                        method(**good, p=0.5, seed=1)
                assert A.inputCSR(7, None, None, None) == 0
            for method, good, last in methods:
                with pytest.raises(ValueError, match="GPU"):
                    method(**good, p=0.5, seed=1, offset=2, head0=3)               # host tensors: everything else is in order
                for bad in (float("nan"), float("inf"), -0.1, 1.0, 2, None, "0.5", True):
                    with pytest.raises(ValueError, match=" p must"):
                        method(**good, p=bad, seed=1)
                for bad in (-1, 2 ** 64, 1.0, None, True):
                    with pytest.raises(ValueError, match=" seed must"):
                        method(**good, p=0.5, seed=bad)
                    with pytest.raises(ValueError, match=" offset must"):
                        method(**good, p=0.5, seed=1, offset=bad)
                for bad in (-1, 2 ** 31, 1.0, None, True):
                    with pytest.raises(ValueError, match=" head0 must"):
                        method(**good, p=0.5, seed=1, head0=bad)
                with pytest.raises(ValueError, match=" p must"):                   # p is judged first: before the tensors and the dtype
                    method(**dict(good, Q=torch.zeros(6, 2, 3)), p=1.0, seed=1)
                for bad in (torch.zeros(6, 2, 3), torch.zeros(6, 2, 3, dtype=torch.float64), None):  # fp32 tensors into the lowp wrapper
                    with pytest.raises(ValueError, match="Q must be a torch.bfloat16 or torch.float16 tensor"):
                        method(**dict(good, Q=bad), p=0.5, seed=1)
                for name in ("K", "V", last):                                      # mixed dtypes
                    for wrong in (other, torch.float32):
                        with pytest.raises(ValueError, match=f"{name} has dtype .*Q has {dt}"):
                            method(**dict(good, **{name: good[name].to(wrong)}), p=0.5, seed=1)
                for bad, word in ((z(7), "shape"), (torch.zeros(7, 2), "dtype"), (z(7, 2).to(other), "dtype"), (z(7, 3), "shape")):
                    with pytest.raises(ValueError, match=f" B .*{word}"):
                        method(**good, p=0.5, seed=1, B=bad)
                with pytest.raises(ValueError, match="scale"):
                    method(**good, p=0.5, seed=1, scale=float("nan"))
                with pytest.raises(ValueError, match="Q has 2 heads, K 3"):
                    method(**dict(good, K=z(4, 3, 3)), p=0.5, seed=1)
            for bad, word in ((z(48), "float32"), (torch.zeros(48, dtype=torch.float64), "float32"), (torch.zeros(47), "shape")):
                with pytest.raises(ValueError, match=word):
                    A.dropoutMhaLowpBackward(**dict(bwd, work=bad), p=0.5, seed=1)
            with pytest.raises(ValueError, match=" dB .*dtype"):
                A.dropoutMhaLowpBackward(**bwd, p=0.5, seed=1, dB=torch.zeros(7, 2))
        assert calls == []
        A.close()
    from scripts import attention_wrapper_transcript as T
    assert len(T.METHODS) == 12 and not any(m.lower().startswith("dropout") for m in T.METHODS)


def test_the_wrappers_pass_the_siblings_arguments_and_the_four_numbers():
    torch = pytest.importorskip("torch")
    from scripts import attention_wrapper_transcript as T
    A = H.anonymouslibHandle(6, 4)
    assert A.inputCSR(7, None, None, None) == 0
    got = {}
    for name in ("dropout_mha_lowp_ptr", "mha_lowp_ptr", "dropout_mha_lowp_backward_ptr", "mha_lowp_backward_ptr"):
        setattr(A, name, lambda *a, _n=name: got.__setitem__(_n, a) or 0)
    for dt, ot in ((torch.bfloat16, _capi.BF16), (torch.float16, _capi.F16)):
        g = lambda *s: T.OnGpu(torch.zeros(*s, dtype=dt))  # noqa: E731
        fwd = dict(Q=g(6, 2, 3), K=g(4, 2, 3), V=g(4, 2, 5), O=g(6, 2, 5))
        B = g(7, 2)
        assert A.dropoutMhaLowp(**fwd, p=0.25, seed=2 ** 63 + 5, offset=2 ** 32 + 1, head0=3, B=B, scale=0.5) == 0
        assert A.mhaLowp(**fwd, B=B, scale=0.5) == 0
        assert got["dropout_mha_lowp_ptr"][:-4] == got["mha_lowp_ptr"] and got["mha_lowp_ptr"][0] == ot
        assert got["dropout_mha_lowp_ptr"][-4:] == (0.25, 2 ** 63 + 5, 2 ** 32 + 1, 3)
        bwd = dict(Q=g(6, 2, 3), K=g(4, 2, 3), V=g(4, 2, 5), dO=g(6, 2, 5), dQ=g(6, 2, 3), dK=g(4, 2, 3), dV=g(4, 2, 5),
                   work=T.OnGpu(torch.zeros(48)))
        assert A.dropoutMhaLowpBackward(**bwd, p=0.6, seed=9, B=B, scale=0.5, dB=g(7, 2)) == 0
        assert A.mhaLowpBackward(**bwd, B=B, scale=0.5, dB=g(7, 2)) == 0
        a, b = got["dropout_mha_lowp_backward_ptr"], got["mha_lowp_backward_ptr"]
        assert a[-4:] == (0.6, 9, 0, 0) and len(a) == len(b) + 4 and a[0] == ot
        assert [x for x in a[:-4] if not hasattr(x, "data_ptr")] == [x for x in b if not hasattr(x, "data_ptr")]
    A.close()


class _Info:
    transpose_built = 1


class _FakeHandle:
    """what the 16-bit autograd functions touch of a handle, recording the calls"""

    def __init__(self, vt, log):
        self._vt, self._m, self._n, self._nnz, self.log = vt, 6, 4, 7, log

    def setStream(self, s):
        return 0

    def info(self):
        return _Info()

    def _record(self, name, ins, outs, numbers):
        self.log.append((name, tuple(t.dtype for t in ins), [None if t is None else t.dtype for t in outs], numbers))
        return 0

    def dropoutMhaLowp(self, Q, K, V, O, p, seed, offset=0, head0=0, B=None, scale=1.0):
        return self._record("dropoutMhaLowp", (Q, K, V), (O, B), (p, seed, offset, head0, scale))

    def dropoutMhaLowpBackward(self, Q, K, V, dO, p, seed, offset=0, head0=0, dQ=None, dK=None, dV=None, work=None, B=None, scale=1.0, dB=None):
        return self._record("dropoutMhaLowpBackward", (Q, K, V, dO), (dQ, dK, dV, work, B, dB), (p, seed, offset, head0, scale))

    def mhaLowp(self, Q, K, V, O, B=None, scale=1.0):
        return self._record("mhaLowp", (Q, K, V), (O, B), (scale,))

    def dropoutMha(self, *a, **kw):
        raise AssertionError("the fp32 / fp64 route")


def test_autograd_routes_16_bit_tensors_to_the_new_calls(monkeypatch):
    torch = pytest.importorskip("torch")
    from benchmark_spmv_using_csr5_amd import autograd
    monkeypatch.setattr(autograd, "_on_current_stream", lambda A, device: None)
    monkeypatch.setattr(autograd, "_with_transpose", lambda A: None)
    for dt, other in ((torch.bfloat16, torch.float16), (torch.float16, torch.bfloat16)):
        for vt in (_capi.F32, _capi.F64):                                      # on fp32 and fp64 handles alike: no stopgap
            for has_bias, need in ((True, (True, True, True, True)), (True, (True, False, False, False)), (False, (False, False, True, False))):
                log = []
                A = _FakeHandle(vt, log)
                Q, K, V = (torch.zeros(*s, dtype=dt, requires_grad=n) for s, n in (((6, 2, 3), need[0]), ((4, 2, 3), need[1]), ((4, 2, 5), need[2])))
                bias = torch.zeros(7, 2, dtype=dt, requires_grad=need[3]) if has_bias else None
                out = autograd.dropout_attention(A, Q, K, V, 0.6, 2 ** 63 + 1, offset=5, scale=0.5, bias=bias)
                assert out.dtype == dt and tuple(out.shape) == (6, 2, 5)
                assert log == [("dropoutMhaLowp", (dt,) * 3, [dt, dt if has_bias else None], (0.6, 2 ** 63 + 1, 5, 0, 0.5))]
                out.backward(torch.zeros_like(out))
                assert len(log) == 2
                name, ins, outs, numbers = log[1]
                column = need[1] or need[2]
                assert name == "dropoutMhaLowpBackward" and ins == (dt,) * 4 and numbers == (0.6, 2 ** 63 + 1, 5, 0, 0.5)  # the same numbers
                assert outs == [dt if n else None for n in need[:3]] + [torch.float32 if column else None, dt if has_bias else None,
                                                                         dt if need[3] else None]
                for t, n in zip((Q, K, V), need):
                    assert (t.grad is not None) == n and (t.grad is None or t.grad.dtype == dt)
                assert bias is None or (bias.grad is not None) == need[3]
            # nothing runs in backward when nothing needs a gradient
            log = []
            A = _FakeHandle(vt, log)

            class Ctx:
                pass
            ctx = Ctx()
            ctx.A, ctx.scale, ctx.drop, ctx.needs_input_grad = A, 0.5, (0.6, 1, 2), (False,) * 9
            z = lambda *s: torch.zeros(*s, dtype=dt)  # noqa: E731
            ctx.saved_tensors = (z(6, 2, 3), z(4, 2, 3), z(4, 2, 5), z(7, 2))
            assert autograd._LowpDropoutAttention.backward(ctx, z(6, 2, 5)) == (None,) * 9 and log == []
            # training=False reaches mhaLowp; a scale without a bias at training=False reaches the new call with p = 0
            Q, K, V, bias = z(6, 2, 3), z(4, 2, 3), z(4, 2, 5), z(7, 2)
            autograd.dropout_attention(A, Q, K, V, 0.6, 7, offset=3, scale=0.5, bias=bias, training=False)
            autograd.dropout_attention(A, Q, K, V, 0.6, 7, training=False)
            autograd.dropout_attention(A, Q, K, V, 0.0, 7)
            assert [e[0] for e in log] == ["mhaLowp"] * 3 and log[0][3] == (0.5,) and log[1][3] == (1.0,)
            del log[:]
            autograd.dropout_attention(A, Q, K, V, 0.6, 7, offset=3, scale=0.5, training=False)
            assert log == [("dropoutMhaLowp", (dt,) * 3, [dt, None], (0.0, 7, 3, 0, 0.5))]
            # K, V and the bias share Q's dtype
            for kw in (dict(K=K.to(other)), dict(V=V.float()), dict(bias=bias.to(other)), dict(bias=bias.double())):
                args = dict(dict(K=K, V=V, bias=bias), **kw)
                with pytest.raises(ValueError, match="bf16 / fp16 operands"):
                    autograd.dropout_attention(A, Q, args["K"], args["V"], 0.6, 7, bias=args["bias"])
            with pytest.raises(ValueError, match="2-D"):
                autograd.dropout_attention(A, Q, K, V, 0.6, 7, bias=z(7))
    doc = autograd.dropout_attention.__doc__
    assert "there is no 16-bit route" not in doc
    for word in ("dropoutMhaLowp", "dropoutMhaLowpBackward", "torch.bfloat16", "float32"):
        assert word in doc, word


# ---- the host emulation -----------------------------------------------------------------------------------------------------------------
def _sanitizers_link(cxx, tmp_path):
    src = tmp_path / "probe.cpp"
    src.write_text("int main() { return 0; }\n")
    r = subprocess.run([cxx, "-fsanitize=address,undefined", str(src), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    return r.returncode == 0 and subprocess.run([str(tmp_path / "probe")]).returncode == 0


def test_host_emulation_under_the_sanitizers(tmp_path):
    """scripts/host_emulation/run_dropout_lowp.py: a stand-alone program built from the two kernel sources (and the float dropped
    ones) with -fsanitize=address,undefined; kat0 and duplicates, one head and three (with head0 = 2 three heads straddle a Philox
    block), (k, d) = (3, 5) and (16, 16) (element loads; 16-byte loads in the unpadded configurations), both operand types: against
    the numpy float64 reference with the reference mask, and against the float dropped launchers' results rounded in integer
    arithmetic.  Every buffer is a heap block of exactly its size with NaN words in all padding; the patterns carry no value array."""
    cxx = "/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else "clang++"
    try:
        linked = _sanitizers_link(cxx, tmp_path)
    except OSError:
        linked = False
    if not linked:
        pytest.skip(f"{cxx} cannot link a program with -fsanitize=address,undefined (no sanitizer runtime)")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "host_emulation", "run_dropout_lowp.py"), "--matrices",
                        "kat0,duplicates", "--heads", "1,3", "--kd", "3x5,16x16", "--types", "bf16,f16", "--cxx", cxx],
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.count(": ok") == 16 and r.stdout.count("duplicates") == 8 and r.stdout.count("heads=3 k=16 d=16: ok") == 4, r.stdout
