"""csr5hip_attention on the host side (no GPU): the C ABI symbol and its declaration, the C++ class member, the return codes and
their order, the Python argument checks, the autograd export, and the rank -> storage rule of the kernel against the conversion."""
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
DECL = ("int csr5hip_attention(csr5hip_handle h, const void *d_Q, int ldq, const void *d_K, int ldk, int k, "
        "const void *d_V, int ldv, int d, void *d_O, int ldo);")


def test_library_exports_the_symbol_with_the_declared_signature():
    import torch  # noqa: F401  (one HIP runtime per process: see _capi.load)
    lib = C.CDLL(_capi.LIB_PATH)
    assert hasattr(lib, "csr5hip_attention")
    with open(os.path.join(INC, "csr5hip.h")) as f:
        text = re.sub(r"\s+", " ", f.read())
    assert DECL in text
    bound = {name: (res, args) for name, res, args in _capi.SYMBOLS if name == "csr5hip_attention"}
    p, i = C.c_void_p, C.c_int
    assert bound == {"csr5hip_attention": (i, [p, p, i, p, i, i, p, i, i, p, i])}
    # the prefixes by which other host tests select their bindings stay theirs
    assert not any(name.startswith(("csr5hip_row_softmax", "csr5hip_sddmm")) for name in bound)


def test_cpp_class_has_the_attention_member(tmp_path):
    src = tmp_path / "use_attention.cpp"
    src.write_text(
        '#include "anonymouslib_hip.h"\n'
        "int use(anonymouslibHandle<int, unsigned, double> &A, const double *Q, const double *K, const double *V, double *O)\n"
        "{ return A.attention(Q, 8, K, 8, 8, V, 16, 16, O, 16); }\n"
        "int use32(anonymouslibHandle<int, unsigned, float> &A, const float *Q, const float *K, const float *V, float *O)\n"
        "{ return A.attention(Q, 8, K, 8, 8, V, 16, 16, O, 16); }\n")
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", f"-I{INC}", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _info_bytes(lib, h):
    info = _capi.Csr5Info()
    assert lib.csr5hip_get_info(h, C.byref(info)) == 0
    return bytes(info)


def test_return_codes_in_order_without_a_gpu():
    """Decided on the host, with fake non-null pointers: the arguments first, then the CSR format, then the missing matrix.
    d = 0 makes a null V and a null O legal, k = 0 a null Q and K: such calls pass the argument checks and end at the format's
    code (the success of d = 0 on a converted handle is asserted in tests/test_gpu_fused_attention.py: a conversion needs a
    device).  get_info unchanged throughout."""
    lib = _capi.load()
    att = lib.csr5hip_attention
    h = C.c_void_p()
    assert lib.csr5hip_create(C.byref(h), 10, 12, _capi.F64) == 0
    f = C.c_void_p(64)
    INV, CSR, UNK = _capi.INVALID_ARGUMENT, _capi.UNSUPPORTED_CSR_SPMV, _capi.UNKOWN_FORMAT
    before = _info_bytes(lib, h)
    assert att(None, f, 4, f, 4, 4, f, 5, 5, f, 5) == INV
    # before inputCSR: nnz counts as 0, so Q, K and V are not judged; O is (m > 0)
    assert att(h, f, 4, f, 4, 4, f, 5, 5, f, 5) == UNK
    assert att(h, None, 4, None, 4, 4, None, 5, 5, f, 5) == UNK
    assert att(h, f, 4, f, 4, 4, f, 5, 5, None, 5) == INV
    assert att(h, f, 4, f, 4, 4, None, 5, 0, None, 5) == UNK           # d = 0: no O needed
    assert att(h, f, 4, f, 4, -1, f, 5, 5, f, 5) == INV                 # the arguments come before the format
    assert att(h, f, 4, f, 4, 4, f, 5, -1, f, 5) == INV
    assert _info_bytes(lib, h) == before
    assert lib.csr5hip_input_csr(h, 100, None, None, None) == 0          # CSR format, nnz > 0
    before = _info_bytes(lib, h)
    assert att(h, f, 4, f, 4, 4, f, 5, 5, f, 5) == CSR
    assert att(h, f, 9, f, 7, 4, f, 8, 5, f, 6) == CSR                   # leading dimensions above the widths
    for bad in ((f, 4, f, 4, -1, f, 5, 5, f, 5), (f, 4, f, 4, 4, f, 5, -1, f, 5),          # k < 0, d < 0
                (f, 3, f, 4, 4, f, 5, 5, f, 5), (f, 4, f, 3, 4, f, 5, 5, f, 5),            # ldq < k, ldk < k
                (f, 4, f, 4, 4, f, 4, 5, f, 5), (f, 4, f, 4, 4, f, 5, 5, f, 4),            # ldv < d, ldo < d
                (None, 4, f, 4, 4, f, 5, 5, f, 5), (f, 4, None, 4, 4, f, 5, 5, f, 5),      # null Q, null K with k > 0
                (f, 4, f, 4, 4, None, 5, 5, f, 5), (f, 4, f, 4, 4, f, 5, 5, None, 5)):     # null V, null O with d > 0
        assert att(h, *bad) == INV, bad
    assert att(None, None, 0, None, 0, -1, None, 0, -1, None, 0) == INV
    assert att(h, None, 0, None, 0, 0, f, 5, 5, f, 5) == CSR             # k = 0: Q and K may be null
    assert att(h, f, 4, f, 4, 4, None, 0, 0, None, 0) == CSR             # d = 0: V and O may be null
    assert att(h, None, 0, None, 0, 0, None, 0, 0, None, 0) == CSR
    assert _info_bytes(lib, h) == before
    assert lib.csr5hip_input_csr(h, 0, None, None, None) == 0            # nnz = 0: only O is needed
    assert att(h, None, 4, None, 4, 4, None, 5, 5, f, 5) == CSR
    assert att(h, None, 4, None, 4, 4, None, 5, 5, None, 5) == INV
    assert lib.csr5hip_free(h) == 0


def test_python_method_rejects_bad_tensors_before_the_library():
    torch = pytest.importorskip("torch")
    A = H.anonymouslibHandle(6, 4)
    calls = []
    A.attention_ptr = lambda *a: calls.append(a) or 0  # nothing may reach the library
    f64 = torch.float64
    Q, K = torch.zeros(6, 3, dtype=f64), torch.zeros(4, 3, dtype=f64)
    V, O = torch.zeros(4, 5, dtype=f64), torch.zeros(6, 5, dtype=f64)
    with pytest.raises(ValueError, match="inputCSR"):
        A.attention(Q, K, V, O)
    assert A.inputCSR(7, None, None, None) == 0
    with pytest.raises(ValueError, match="GPU"):
        A.attention(Q, K, V, O)                                              # host tensors: everything else is in order
    good = dict(Q=Q, K=K, V=V, O=O)
    for name, t in good.items():
        rows, cols = t.shape
        for bad, word in ((t.float(), "dtype"), (torch.zeros(rows + 1, cols, dtype=f64), "shape"),
                          (torch.zeros(rows * cols, dtype=f64), "shape"), (torch.zeros(rows, 2 * cols, dtype=f64)[:, ::2], "stride"),
                          (torch.zeros(cols, rows, dtype=f64).t(), "stride"), (torch.zeros(1, cols, dtype=f64).expand(rows, cols), "overlap"),
                          (np.zeros((rows, cols)), "tensor")):
            with pytest.raises(ValueError, match=f"{name} .*{word}"):
                A.attention(**dict(good, **{name: bad}))
    with pytest.raises(ValueError, match="Q has 3 columns, K 2"):
        A.attention(Q, torch.zeros(4, 2, dtype=f64), V, O)
    with pytest.raises(ValueError, match="V has 5 columns, O 4"):
        A.attention(Q, K, V, torch.zeros(6, 4, dtype=f64))
    wide = torch.zeros(6, 10, dtype=f64)
    with pytest.raises(ValueError, match="with Q .*aliased"):
        A.attention(wide[:, :3], K, V, wide[:, 5:])                          # column slices of one tensor
    big = torch.zeros(10, 5, dtype=f64)
    with pytest.raises(ValueError, match="with V .*aliased"):
        A.attention(Q, K, big[:4], big[4:])
    sq = H.anonymouslibHandle(4, 4)
    sq.attention_ptr = A.attention_ptr
    assert sq.inputCSR(3, None, None, None) == 0
    X = torch.zeros(4, 3, dtype=f64)
    with pytest.raises(ValueError, match="with K .*aliased"):
        sq.attention(torch.zeros(4, 3, dtype=f64), X, torch.zeros(4, 3, dtype=f64), X)
    with pytest.raises(ValueError, match="GPU"):
        sq.attention(X, X, X, torch.zeros(4, 3, dtype=f64))                  # Q, K and V may be one tensor: only the device is wrong
    with pytest.raises(ValueError, match="GPU"):
        A.attention(wide[:, :3], K, big[:4], O)                              # slices (ld > width) are legal operands
    assert calls == []
    sq.close()
    A.close()


def test_autograd_exports_fused_attention_without_a_gpu():
    from benchmark_spmv_using_csr5_amd import autograd
    assert "fused_attention" in autograd.__all__ and "attention" in autograd.__all__
    assert callable(autograd.fused_attention) and autograd.fused_attention is not autograd.attention


def test_rank_to_storage_rule_of_the_header_matches_the_conversion():
    """the rule csr5_attention.hip takes its columns by, restated in numpy (one division by T for the row's first entry, a second
    one only past that tile, the division by sigma as a multiplication by its rounded-up reciprocal in 20 fractional bits),
    against the oracle's converted column_index on every zoo matrix and sigma"""
    from oracle.csr5_oracle import Oracle
    from tests import zoo
    orc = Oracle()
    met = {"moved": False, "fast-track": False, "tail": False, "row across tiles": False}
    for mat in zoo.small_zoo():
        rp = mat.row_ptr.astype(np.int64)
        rank_in_row = np.arange(mat.nnz, dtype=np.int64) - np.repeat(rp[:-1], np.diff(rp))
        first = np.repeat(rp[:-1], np.diff(rp))
        for sigma in (4, 7, 16, 32):
            fmt = orc.convert(64, sigma, mat.m, mat.row_ptr, mat.col, np.ones(mat.nnz))
            T, tiles = 64 * sigma, max(fmt.p - 1, 0)
            recip = (1 << 20) // sigma + 1
            t0 = first // T
            x = first - t0 * T + rank_in_row
            t = t0 + x // T
            x = x % T
            tp = fmt.tile_ptr.astype(np.int64)
            tc = np.minimum(t, max(tiles - 1, 0))
            moved = (t < tiles) & (tp[tc] != tp[tc + 1]) if tiles else np.zeros(mat.nnz, dtype=bool)
            lane = (x * recip) >> 20
            assert np.array_equal(lane, x // sigma)
            step = x - lane * sigma
            pos = np.where(moved, t * T + step * 64 + lane, t * T + x)
            assert np.array_equal(fmt.col[pos], mat.col[:mat.nnz]), (mat.name, sigma)
            met["moved"] |= bool(moved.any())
            met["fast-track"] |= bool(((t < tiles) & ~moved).any())
            met["tail"] |= bool((t >= tiles).any())
            met["row across tiles"] |= bool((t > t0).any())
    assert all(met.values()), met
