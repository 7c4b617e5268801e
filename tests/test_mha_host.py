"""csr5hip_mha / csr5hip_mha_backward on the host side (no GPU): the C ABI symbols and their declarations, the C++ class members,
the return codes and their order, the Python argument checks on packed (rows, heads, width) tensors, and
``autograd.multihead_attention``."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from benchmark_spmv_using_csr5_amd import _capi
from benchmark_spmv_using_csr5_amd import handle as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
DECLS = {
    "csr5hip_mha": ("int csr5hip_mha(csr5hip_handle h, int heads, const void *d_Q, int ldq, const void *d_K, int ldk, int k, "
                    "const void *d_V, int ldv, int d, void *d_O, int ldo);"),
    "csr5hip_mha_backward": ("int csr5hip_mha_backward(csr5hip_handle h, int heads, const void *d_Q, int ldq, const void *d_K, int ldk, "
                             "int k, const void *d_V, int ldv, int d, const void *d_dO, int lddo, void *d_dQ, int lddq, void *d_dK, "
                             "int lddk, void *d_dV, int lddv, void *d_work);"),
}
INT_MAX = 2 ** 31 - 1


def test_library_exports_both_symbols_with_the_declared_signatures():
    import torch  # noqa: F401  (one HIP runtime per process: see _capi.load)
    lib = C.CDLL(_capi.LIB_PATH)
    with open(os.path.join(INC, "csr5hip.h")) as f:
        text = re.sub(r"\s+", " ", f.read())
    for name, decl in DECLS.items():
        assert hasattr(lib, name)
        assert decl in text
    bound = {name: (res, args) for name, res, args in _capi.SYMBOLS if name.startswith("csr5hip_mha")}
    p, i = C.c_void_p, C.c_int
    assert bound == {"csr5hip_mha": (i, [p, i, p, i, p, i, i, p, i, i, p, i]),
                     "csr5hip_mha_backward": (i, [p, i, p, i, p, i, i, p, i, i, p, i, p, i, p, i, p, i, p])}
    # the single-head calls keep their prefix to themselves
    assert [n for n, _, _ in _capi.SYMBOLS if n.startswith("csr5hip_attention")] == ["csr5hip_attention", "csr5hip_attention_backward"]


def test_cpp_class_has_the_mha_members(tmp_path):
    src = tmp_path / "use_mha.cpp"
    src.write_text(
        '#include "anonymouslib_hip.h"\n'
        "int use(anonymouslibHandle<int, unsigned, double> &A, const double *Q, const double *K, const double *V, const double *dO,\n"
        "        double *O, double *dQ, double *dK, double *dV, double *work)\n"
        "{ return A.mha(4, Q, 32, K, 32, 8, V, 64, 16, O, 64)\n"
        "       + A.mhaBackward(4, Q, 32, K, 32, 8, V, 64, 16, dO, 64, dQ, 32, dK, 32, dV, 64, work); }\n"
        "int use32(anonymouslibHandle<int, unsigned, float> &A, const float *Q, const float *K, const float *V, const float *dO,\n"
        "          float *O, float *dQ)\n"
        "{ return A.mha(4, Q, 32, K, 32, 8, V, 64, 16, O, 64)\n"
        "       + A.mhaBackward(4, Q, 32, K, 32, 8, V, 64, 16, dO, 64, dQ, 32, nullptr, 32, nullptr, 64, nullptr); }\n")
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", f"-I{INC}", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _info_bytes(lib, h):
    info = _capi.Csr5Info()
    assert lib.csr5hip_get_info(h, C.byref(info)) == 0
    return bytes(info)


def test_return_codes_in_order_without_a_gpu():
    """Decided on the host, with fake non-null pointers, in the order of the single-head calls: the arguments (heads included, a
    leading dimension against heads times its width in 64 bits), the operands (judged only with heads > 0 and nnz > 0), for the
    backward the missing companion, then the CSR format, then the missing matrix; heads = 0 ends at the format's code.
    get_info unchanged throughout."""
    lib = _capi.load()
    h = C.c_void_p()
    assert lib.csr5hip_create(C.byref(h), 10, 12, _capi.F64) == 0
    f = C.c_void_p(64)
    INV, CSR, UNK = _capi.INVALID_ARGUMENT, _capi.UNSUPPORTED_CSR_SPMV, _capi.UNKOWN_FORMAT

    def fwd(heads=3, Q=f, ldq=12, K=f, ldk=12, k=4, V=f, ldv=15, d=5, O=f, ldo=15, handle=h):
        return lib.csr5hip_mha(handle, heads, Q, ldq, K, ldk, k, V, ldv, d, O, ldo)

    def bwd(heads=3, Q=f, ldq=12, K=f, ldk=12, k=4, V=f, ldv=15, d=5, dO=f, lddo=15, dQ=f, lddq=12, dK=None, lddk=12, dV=None, lddv=15,
            work=None, handle=h):
        return lib.csr5hip_mha_backward(handle, heads, Q, ldq, K, ldk, k, V, ldv, d, dO, lddo, dQ, lddq, dK, lddk, dV, lddv, work)

    def no_companion(**kw):
        return bwd(**kw) == INV and "csr5hip_build_transpose" in _capi.last_error()
    before = _info_bytes(lib, h)
    for call in (fwd, bwd):
        assert call(handle=None) == INV
        assert call() == UNK                                           # before inputCSR: nnz counts as 0, no operand is judged
        assert call(Q=None, K=None, V=None) == UNK
        assert call(heads=0) == UNK                                    # heads = 0 is decided after the format
        assert call(heads=-1) == INV and call(k=-1) == INV and call(d=-1) == INV   # the arguments come before the format
    assert no_companion(dK=f, work=f) and no_companion(dV=f, work=f) and no_companion(heads=0, dK=f)
    assert _info_bytes(lib, h) == before
    assert lib.csr5hip_input_csr(h, 100, None, None, None) == 0       # CSR format, nnz > 0
    before = _info_bytes(lib, h)
    assert fwd() == CSR and bwd() == CSR
    assert fwd(heads=0) == CSR and bwd(heads=0) == CSR
    assert fwd(heads=0, Q=None, K=None, V=None, O=None) == CSR        # heads = 0: no operand is judged
    assert fwd(ldq=13, ldk=14, ldv=16, ldo=17) == CSR                 # leading dimensions above heads * width
    for bad in (dict(heads=-1), dict(k=-1), dict(d=-1), dict(ldq=11), dict(ldk=11), dict(ldv=14), dict(ldo=14),
                dict(Q=None), dict(K=None), dict(V=None), dict(O=None)):
        assert fwd(**bad) == INV, bad
    for bad in (dict(heads=-1), dict(k=-1), dict(d=-1), dict(ldq=11), dict(ldk=11), dict(lddq=11), dict(lddk=11), dict(ldv=14),
                dict(lddo=14), dict(lddv=14), dict(Q=None), dict(K=None), dict(V=None), dict(dO=None), dict(dK=f), dict(dV=f)):
        assert bwd(**bad) == INV, bad
    # heads * k beyond INT_MAX: compared in 64 bits, no leading dimension can reach it
    big = 2 ** 16
    assert fwd(heads=big, k=big, ldq=INT_MAX, ldk=INT_MAX, d=1, ldv=INT_MAX, ldo=INT_MAX) == INV
    assert fwd(heads=big, d=big, k=1, ldq=INT_MAX, ldk=INT_MAX, ldv=INT_MAX, ldo=INT_MAX) == INV
    assert bwd(heads=big, k=big, d=1, ldq=INT_MAX, ldk=INT_MAX, lddq=INT_MAX, lddk=INT_MAX, ldv=INT_MAX, lddo=INT_MAX, lddv=INT_MAX) == INV
    assert fwd(heads=big, k=big // 2 - 1, d=1, ldq=INT_MAX, ldk=INT_MAX, ldv=INT_MAX, ldo=INT_MAX) == CSR   # just below: legal
    assert fwd(Q=None, K=None, k=0, ldq=0, ldk=0) == CSR              # k = 0: Q and K may be null
    assert fwd(V=None, O=None, d=0, ldv=0, ldo=0) == CSR              # d = 0: V and O may be null
    # backward: the companion is judged before the format, and only where dK or dV is wanted
    assert no_companion(dK=f, work=f) and no_companion(dV=f, work=f) and no_companion(dQ=None, dV=f, work=f)
    assert bwd(dQ=f, work=f) == CSR                                    # dQ alone passes on to the format's code
    assert bwd(Q=None, K=None, V=None, dO=None, dQ=None) == CSR        # nothing wanted: nothing judged but the format
    assert _info_bytes(lib, h) == before
    assert lib.csr5hip_input_csr(h, 0, None, None, None) == 0          # nnz = 0: no operand is needed
    assert fwd(Q=None, K=None, V=None) == CSR and fwd(Q=None, K=None, V=None, O=None) == INV
    assert bwd(Q=None, K=None, V=None, dO=None) == CSR
    assert no_companion(Q=None, K=None, V=None, dO=None, dK=f)
    assert lib.csr5hip_free(h) == 0


def test_python_methods_reject_bad_tensors_before_the_library():
    torch = pytest.importorskip("torch")
    A = H.anonymouslibHandle(6, 4)
    calls = []
    A.mha_ptr = lambda *a: calls.append(a) or 0  # nothing may reach the library
    A.mha_backward_ptr = lambda *a: calls.append(a) or 0
    f64 = torch.float64
    z = lambda *s: torch.zeros(*s, dtype=f64)  # noqa: E731
    fwd = dict(Q=z(6, 2, 3), K=z(4, 2, 3), V=z(4, 2, 5), O=z(6, 2, 5))
    bwd = dict(Q=z(6, 2, 3), K=z(4, 2, 3), V=z(4, 2, 5), dO=z(6, 2, 5), dQ=z(6, 2, 3), dK=z(4, 2, 3), dV=z(4, 2, 5), work=z(48))
    with pytest.raises(ValueError, match="inputCSR"):
        A.mha(**fwd)
    with pytest.raises(ValueError, match="inputCSR"):
        A.mhaBackward(**bwd)
    assert A.inputCSR(7, None, None, None) == 0
    with pytest.raises(ValueError, match="GPU"):
        A.mha(**fwd)                                                   # host tensors: everything else is in order
    with pytest.raises(ValueError, match="GPU"):
        A.mhaBackward(**bwd)
    with pytest.raises(ValueError, match="GPU"):
        A.mhaBackward(bwd["Q"], bwd["K"], bwd["V"], bwd["dO"], dQ=bwd["dQ"])   # dQ alone: no workspace needed
    for method, good in ((A.mha, fwd), (A.mhaBackward, bwd)):
        for name in (n for n in good if n != "work"):
            rows, heads, width = good[name].shape
            for bad, word in ((z(rows, heads * width), "shape"),                              # 2-D
                              (good[name].float(), "dtype"),
                              (z(rows + 1, heads, width), "shape"),
                              (z(rows, heads, 2 * width)[:, :, :width], "stride\\(1\\)"),      # stride(1) != width
                              (z(rows, heads, 2 * width)[:, :, ::2], "stride\\(2\\)"),          # stride(2) != 1
                              (z(1, heads, width).expand(rows, heads, width), "overlap"),     # expanded rows
                              (np.zeros((rows, heads, width)), "tensor")):
                with pytest.raises(ValueError, match=f"{name} .*{word}"):
                    method(**dict(good, **{name: bad}))
    with pytest.raises(ValueError, match="Q has 2 heads, K 3"):
        A.mha(**dict(fwd, K=z(4, 3, 3)))
    with pytest.raises(ValueError, match="V has width 5, O 4"):
        A.mha(**dict(fwd, O=z(6, 2, 4)))
    with pytest.raises(ValueError, match="Q has width 3, K 2"):
        A.mha(**dict(fwd, K=z(4, 2, 2)))
    with pytest.raises(ValueError, match="Q has 2 heads, dV 1"):
        A.mhaBackward(**dict(bwd, dV=z(4, 1, 5)))
    with pytest.raises(ValueError, match="V has width 5, dO 6"):
        A.mhaBackward(**dict(bwd, dO=z(6, 2, 6)))
    both = z(4 + 6, 2, 5)
    with pytest.raises(ValueError, match="O shares storage with V .*aliased"):
        A.mha(**dict(fwd, V=both[:4], O=both[4:]))
    with pytest.raises(ValueError, match="dV shares storage with V .*aliased"):
        two = z(8, 2, 5)
        A.mhaBackward(**dict(bwd, V=two[:4], dV=two[4:]))
    with pytest.raises(ValueError, match="dK shares storage with dQ .*aliased"):
        pool = z(10, 2, 3)
        A.mhaBackward(**dict(bwd, dQ=pool[:6], dK=pool[6:]))
    for bad, word in ((None, "tensor"), (torch.zeros(48), "dtype"), (z(47), "shape"), (z(6, 8), "shape"), (z(96)[::2], "contiguous")):
        with pytest.raises(ValueError, match=f"work .*{word}"):
            A.mhaBackward(**dict(bwd, work=bad))
    with pytest.raises(ValueError, match="GPU"):
        A.mha(**dict(fwd, Q=z(6, 5, 3)[:, 1:3]))                        # a slice of a wider tensor (stride(0) > heads * width) is legal
    assert calls == []
    A.close()


def test_multihead_attention_is_exported_without_a_gpu():
    from benchmark_spmv_using_csr5_amd import autograd
    assert "multihead_attention" in autograd.__all__ and callable(autograd.multihead_attention)
