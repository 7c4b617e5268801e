"""update_values on the host side (no GPU): the two C ABI symbols and their declarations, the C++ class members, the return
codes that are decided before any device work, and the Python argument checks."""
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


def test_library_exports_update_values_with_the_declared_signatures():
    import torch  # noqa: F401  (one HIP runtime per process: see _capi.load)
    lib = C.CDLL(_capi.LIB_PATH)
    with open(os.path.join(INC, "csr5hip.h")) as f:
        text = re.sub(r"\s+", " ", f.read())
    for name, decl in (("csr5hip_update_values", "int csr5hip_update_values(csr5hip_handle h, const void *d_val_csr);"),
                       ("csr5hip_multi_update_values", "int csr5hip_multi_update_values(csr5hip_multi mh, const void *d_val_csr);")):
        assert hasattr(lib, name)
        assert decl in text
        assert [(n, r, a) for n, r, a in _capi.SYMBOLS if n == name] == [(name, C.c_int, [C.c_void_p, C.c_void_p])]


def test_cpp_classes_have_update_values_members(tmp_path):
    src = tmp_path / "use_update_values.cpp"
    src.write_text(
        '#include "anonymouslib_hip.h"\n'
        "int use(anonymouslibHandle<int, unsigned, double> &A, const double *v) { return A.updateValues(v); }\n"
        "int use32(anonymouslibHandle<int, unsigned, float> &A, const float *v) { return A.updateValues(v); }\n")
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", f"-I{INC}", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_update_values_return_codes_without_a_gpu():
    """Decided on the host, in this order: the handle, the format, nnz = 0, the pointer, the overlap with the handle's own
    value array."""
    lib = _capi.load()
    h = C.c_void_p()
    assert lib.csr5hip_create(C.byref(h), 10, 10, _capi.F64) == 0
    new = C.c_void_p(1 << 30)
    assert lib.csr5hip_update_values(None, new) == _capi.INVALID_ARGUMENT       # null handle
    assert lib.csr5hip_update_values(h, new) == _capi.UNKOWN_FORMAT             # before inputCSR
    assert lib.csr5hip_update_values(h, None) == _capi.UNKOWN_FORMAT
    val = 1 << 20                                                               # a made-up device address: never dereferenced
    assert lib.csr5hip_input_csr(h, 100, None, None, C.c_void_p(val)) == 0
    assert lib.csr5hip_update_values(h, None) == _capi.INVALID_ARGUMENT         # null pointer, nnz > 0
    for inside in (val, val + 8, val + 99 * 8, val + 100 * 8 - 1, val - 8):     # inside (or reaching into) the 800 bytes of val
        assert lib.csr5hip_update_values(h, C.c_void_p(inside)) == _capi.INVALID_ARGUMENT, inside
        assert "overlaps" in _capi.last_error()
    assert lib.csr5hip_input_csr(h, 0, None, None, None) == 0
    assert lib.csr5hip_update_values(h, None) == _capi.SUCCESS                  # nnz = 0: a no-op
    assert lib.csr5hip_free(h) == 0
    assert lib.csr5hip_multi_update_values(None, new) == _capi.INVALID_ARGUMENT


def test_python_update_values_rejects_bad_tensors_before_the_library():
    torch = pytest.importorskip("torch")
    A = H.anonymouslibHandle(6, 4)
    calls = []
    A.updateValues_ptr = lambda *a: calls.append(a) or 0  # nothing may reach the library
    with pytest.raises(ValueError, match="inputCSR"):
        A.updateValues(torch.zeros(5, dtype=torch.float64))
    mine = torch.zeros(9, dtype=torch.float64)
    assert A.inputCSR(9, None, None, 1 << 20) == 0                              # (a made-up device address: never dereferenced)
    A._keep["val"] = mine                                                       # what inputCSR keeps when given a tensor
    with pytest.raises(ValueError, match="GPU"):
        A.updateValues(torch.zeros(9, dtype=torch.float64))                     # a host tensor, otherwise right
    with pytest.raises(ValueError, match="dtype"):
        A.updateValues(torch.zeros(9, dtype=torch.float32))
    with pytest.raises(ValueError, match="tensor"):
        A.updateValues(np.zeros(9))
    with pytest.raises(ValueError, match="shape"):
        A.updateValues(torch.zeros(8, dtype=torch.float64))                     # wrong length
    with pytest.raises(ValueError, match="shape"):
        A.updateValues(torch.zeros(3, 3, dtype=torch.float64))                  # not 1-D
    with pytest.raises(ValueError, match="contiguous"):
        A.updateValues(torch.zeros(18, dtype=torch.float64)[::2])
    with pytest.raises(ValueError, match="aliased"):
        A.updateValues(mine)
    with pytest.raises(ValueError, match="aliased"):
        A.updateValues(mine.view(9))                                            # another tensor on the same storage
    assert calls == []
    A.close()
