"""csr5hip_attention_backward on the host side (no GPU): the C ABI symbol and its declaration, the C++ class member, the return
codes and their order (the missing companion included), the Python argument checks, and the ``backward`` argument of
``autograd.fused_attention``."""
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
NAME = "csr5hip_attention_backward"
DECL = ("int csr5hip_attention_backward(csr5hip_handle h, const void *d_Q, int ldq, const void *d_K, int ldk, int k, "
        "const void *d_V, int ldv, int d, const void *d_dO, int lddo, void *d_dQ, int lddq, void *d_dK, int lddk, "
        "void *d_dV, int lddv, void *d_work);")


def test_library_exports_the_symbol_with_the_declared_signature():
    import torch  # noqa: F401  (one HIP runtime per process: see _capi.load)
    lib = C.CDLL(_capi.LIB_PATH)
    assert hasattr(lib, NAME)
    with open(os.path.join(INC, "csr5hip.h")) as f:
        text = re.sub(r"\s+", " ", f.read())
    assert DECL in text
    bound = {name: (res, args) for name, res, args in _capi.SYMBOLS if name == NAME}
    p, i = C.c_void_p, C.c_int
    assert bound == {NAME: (i, [p, p, i, p, i, i, p, i, i, p, i, p, i, p, i, p, i, p])}
    # the forward keeps its own binding
    assert [name for name, _, _ in _capi.SYMBOLS if name.startswith("csr5hip_attention")] == ["csr5hip_attention", NAME]


def test_cpp_class_has_the_attention_backward_member(tmp_path):
    src = tmp_path / "use_attention_backward.cpp"
    src.write_text(
        '#include "anonymouslib_hip.h"\n'
        "int use(anonymouslibHandle<int, unsigned, double> &A, const double *Q, const double *K, const double *V, const double *dO,\n"
        "        double *dQ, double *dK, double *dV, double *work)\n"
        "{ return A.attentionBackward(Q, 8, K, 8, 8, V, 16, 16, dO, 16, dQ, 8, dK, 8, dV, 16, work); }\n"
        "int use32(anonymouslibHandle<int, unsigned, float> &A, const float *Q, const float *K, const float *V, const float *dO,\n"
        "          float *dQ)\n"
        "{ return A.attentionBackward(Q, 8, K, 8, 8, V, 16, 16, dO, 16, dQ, 8, nullptr, 8, nullptr, 16, nullptr); }\n")
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", f"-I{INC}", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _info_bytes(lib, h):
    info = _capi.Csr5Info()
    assert lib.csr5hip_get_info(h, C.byref(info)) == 0
    return bytes(info)


def test_return_codes_in_order_without_a_gpu():
    """Decided on the host, with fake non-null pointers: the arguments first, then the operands and the workspace (judged only
    where an output is wanted and nnz > 0), then the missing companion (only where dK or dV is wanted), then the CSR format,
    then the missing matrix.  A handle that was never converted has no companion, so every call that wants dK or dV ends at
    INVALID_ARGUMENT with a text, and dQ alone passes on to the format's code.  get_info unchanged throughout."""
    lib = _capi.load()
    bwd = lib.csr5hip_attention_backward
    h = C.c_void_p()
    assert lib.csr5hip_create(C.byref(h), 10, 12, _capi.F64) == 0
    f = C.c_void_p(64)
    INV, CSR, UNK = _capi.INVALID_ARGUMENT, _capi.UNSUPPORTED_CSR_SPMV, _capi.UNKOWN_FORMAT

    def call(Q=f, ldq=4, K=f, ldk=4, k=4, V=f, ldv=5, d=5, dO=f, lddo=5, dQ=f, lddq=4, dK=None, lddk=4, dV=None, lddv=5, work=None,
             handle=h):
        return bwd(handle, Q, ldq, K, ldk, k, V, ldv, d, dO, lddo, dQ, lddq, dK, lddk, dV, lddv, work)

    def no_companion(**kw):
        rc = call(**kw)
        return rc == INV and "csr5hip_build_transpose" in _capi.last_error()
    before = _info_bytes(lib, h)
    assert call(handle=None) == INV
    # before inputCSR: nnz counts as 0, so no operand is judged
    assert call() == UNK
    assert call(Q=None, K=None, V=None, dO=None) == UNK
    assert call(dQ=None) == UNK                                      # nothing wanted: the format's code
    assert call(k=-1) == INV and call(d=-1) == INV                   # the arguments come before the format
    assert no_companion(dK=f, work=f) and no_companion(dV=f, work=f) and no_companion(dQ=None, dK=f, dV=f, work=f)
    assert _info_bytes(lib, h) == before
    assert lib.csr5hip_input_csr(h, 100, None, None, None) == 0      # CSR format, nnz > 0
    before = _info_bytes(lib, h)
    assert call() == CSR
    assert call(ldq=9, ldk=7, ldv=8, lddo=6, lddq=5, lddk=6, lddv=9) == CSR   # leading dimensions above the widths
    for bad in (dict(k=-1), dict(d=-1), dict(ldq=3), dict(ldk=3), dict(lddq=3), dict(lddk=3), dict(ldv=4), dict(lddo=4), dict(lddv=4),
                dict(Q=None), dict(K=None), dict(V=None), dict(dO=None),          # null operands with k > 0, d > 0
                dict(dK=f), dict(dV=f), dict(dQ=None, dK=f)):                       # dK or dV without a workspace
        assert call(**bad) == INV, bad
    assert call(lddk=3, dK=None) == INV and call(lddv=4, dV=None) == INV       # judged even for an output that is not wanted
    assert call(handle=None, k=-1, d=-1) == INV
    assert call(Q=None, K=None, k=0, ldq=0, ldk=0, lddq=0, lddk=0) == CSR      # k = 0: Q and K may be null
    assert call(V=None, dO=None, d=0, ldv=0, lddo=0, lddv=0) == CSR            # d = 0: V and dO may be null
    assert call(Q=None, K=None, V=None, dO=None, dQ=None) == CSR               # nothing wanted: nothing judged but the format
    # the companion is judged before the format
    assert no_companion(dK=f, work=f) and no_companion(dV=f, work=f) and no_companion(dQ=None, dV=f, work=f)
    assert call(dQ=f, work=f) == CSR                                            # dQ alone needs no companion
    assert _info_bytes(lib, h) == before
    assert lib.csr5hip_input_csr(h, 0, None, None, None) == 0                   # nnz = 0: no operand is needed
    assert call(Q=None, K=None, V=None, dO=None) == CSR
    assert no_companion(Q=None, K=None, V=None, dO=None, dK=f)
    assert lib.csr5hip_free(h) == 0


def test_python_method_rejects_bad_tensors_before_the_library():
    torch = pytest.importorskip("torch")
    A = H.anonymouslibHandle(6, 4)
    calls = []
    A.attention_backward_ptr = lambda *a: calls.append(a) or 0  # nothing may reach the library
    f64 = torch.float64
    z = lambda r, c: torch.zeros(r, c, dtype=f64)  # noqa: E731
    good = dict(Q=z(6, 3), K=z(4, 3), V=z(4, 5), dO=z(6, 5), dQ=z(6, 3), dK=z(4, 3), dV=z(4, 5), work=torch.zeros(24, dtype=f64))
    with pytest.raises(ValueError, match="inputCSR"):
        A.attentionBackward(**good)
    assert A.inputCSR(7, None, None, None) == 0
    with pytest.raises(ValueError, match="GPU"):
        A.attentionBackward(**good)                                             # host tensors: everything else is in order
    with pytest.raises(ValueError, match="GPU"):
        A.attentionBackward(good["Q"], good["K"], good["V"], good["dO"], dQ=good["dQ"])   # dQ alone: no workspace needed
    for name in ("Q", "K", "V", "dO", "dQ", "dK", "dV"):
        rows, cols = good[name].shape
        for bad, word in ((good[name].float(), "dtype"), (z(rows + 1, cols), "shape"), (torch.zeros(rows * cols, dtype=f64), "shape"),
                          (z(rows, 2 * cols)[:, ::2], "stride"), (z(cols, rows).t(), "stride"), (z(1, cols).expand(rows, cols), "overlap"),
                          (np.zeros((rows, cols)), "tensor")):
            with pytest.raises(ValueError, match=f"{name} .*{word}"):
                A.attentionBackward(**dict(good, **{name: bad}))
    for name, other, text in (("K", z(4, 2), "Q has 3 columns, K 2"), ("dQ", z(6, 2), "Q has 3 columns, dQ 2"),
                              ("dK", z(4, 4), "Q has 3 columns, dK 4"), ("dO", z(6, 4), "V has 5 columns, dO 4"),
                              ("dV", z(4, 6), "V has 5 columns, dV 6")):
        with pytest.raises(ValueError, match=text):
            A.attentionBackward(**dict(good, **{name: other}))
    for bad, word in ((None, "tensor"), (torch.zeros(24), "dtype"), (torch.zeros(23, dtype=f64), "shape"), (z(6, 4), "shape"),
                      (torch.zeros(48, dtype=f64)[::2], "contiguous")):
        with pytest.raises(ValueError, match=f"work .*{word}"):
            A.attentionBackward(**dict(good, work=bad))
    wide = z(6, 10)
    with pytest.raises(ValueError, match="dQ shares storage with Q .*aliased"):
        A.attentionBackward(**dict(good, Q=wide[:, :3], dQ=wide[:, 5:8]))     # column slices of one tensor
    with pytest.raises(ValueError, match="dV shares storage with dK .*aliased"):
        big = z(4, 8)
        A.attentionBackward(**dict(good, dK=big[:, :3], dV=big[:, 3:]))
    with pytest.raises(ValueError, match="dK shares storage with K .*aliased"):
        both = z(8, 3)
        A.attentionBackward(**dict(good, K=both[:4], dK=both[4:]))
    with pytest.raises(ValueError, match="dV shares storage with work .*aliased"):
        pool = torch.zeros(44, dtype=f64)
        A.attentionBackward(**dict(good, work=pool[:24], dV=pool[24:].view(4, 5)))
    with pytest.raises(ValueError, match="GPU"):
        A.attentionBackward(**dict(good, Q=wide[:, :3], V=z(4, 9)[:, 2:7]))    # slices (ld > width) are legal operands
    assert calls == []
    A.close()


def test_fused_attention_takes_the_backward_argument_without_a_gpu():
    import inspect

    from benchmark_spmv_using_csr5_amd import autograd
    assert inspect.signature(autograd.fused_attention).parameters["backward"].default == "recompute"
    for bad in ("", "Fused", "eager", None, True):
        with pytest.raises(ValueError, match="backward must be 'recompute' or 'fused'"):
            autograd.fused_attention(None, None, None, None, backward=bad)     # judged before anything is touched
    # both legal values pass that check and fail later, at the operands
    for ok in ("recompute", "fused"):
        with pytest.raises(Exception) as e:
            autograd.fused_attention(None, None, None, None, backward=ok)
        assert "backward must be" not in str(e.value)
