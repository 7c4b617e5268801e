"""The dropped attention calls (csr5hip_dropout.h) on the host side (no GPU): the known answers of Philox4x32-10 and the kept fraction
of the reference mask, the C ABI symbols and their declarations, the C++ class members, the return codes and their order, the Python
argument checks, the routing of the two autograd functions, that the numpy reference rejects two wrong kernels -- Z summed over the
kept entries only, and the mask indexed by the companion's position instead of the parent's rank -- and the host emulation of the
kernel sources under the address and undefined-behaviour sanitizers (a stand-alone program)."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from benchmark_spmv_using_csr5_amd import _capi
from benchmark_spmv_using_csr5_amd import handle as H
from tests import dropout_reference as DR
from tests import sddmm_reference as S
from tests import zoo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
_TAIL = "double p, unsigned long long seed, unsigned long long offset, int head0);"
_FWD = "const void *d_Q, int ldq, const void *d_K, int ldk, int k, const void *d_V, int ldv, int d, void *d_O, int ldo, "
_BWD = ("const void *d_Q, int ldq, const void *d_K, int ldk, int k, const void *d_V, int ldv, int d, const void *d_dO, int lddo, "
        "void *d_dQ, int lddq, void *d_dK, int lddk, void *d_dV, int lddv, void *d_work, void *d_dB, int lddb, ")
_GAT = "int heads, double negative_slope, const void *d_a, double scale, const void *d_B, int ldb, "
_EDGE = "int heads, double scale, const void *d_B, int ldb, "
DECLS = {
    "csr5hip_dropout_mha": "int csr5hip_dropout_mha(csr5hip_handle h, " + _EDGE + _FWD + _TAIL,
    "csr5hip_dropout_mha_backward": "int csr5hip_dropout_mha_backward(csr5hip_handle h, " + _EDGE + _BWD + _TAIL,
    "csr5hip_dropout_gat": "int csr5hip_dropout_gat(csr5hip_handle h, " + _GAT + _FWD + _TAIL,
    "csr5hip_dropout_gat_backward": "int csr5hip_dropout_gat_backward(csr5hip_handle h, " + _GAT + _BWD + "void *d_dAr, int lddar, " + _TAIL,
    "csr5hip_dropout_mask": ("int csr5hip_dropout_mask(csr5hip_handle h, int heads, double p, unsigned long long seed, "
                             "unsigned long long offset, int head0, void *d_mask, int ldm);"),
}


def _small():
    return {m.name: m for m in zoo.small_zoo()}["kat0"], S.duplicates_matrix()


# ---- the mask -------------------------------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    for counter, key, want in DR.KNOWN_ANSWERS:
        got = DR.philox4x32_10(counter, key)
        assert tuple(int(w) for w in got) == want, [hex(int(w)) for w in got]
    # vectorised over the first counter word: element i is the scalar call's
    many = DR.philox4x32_10((np.arange(5), 1, 2, 3), (4, 5))
    for i in range(5):
        assert [int(w[i]) for w in many] == [int(w) for w in DR.philox4x32_10((i, 1, 2, 3), (4, 5))]


def test_threshold_and_cd():
    assert DR.threshold(0.0) == 0 and DR.threshold(0.5) == 2 ** 31 and DR.threshold(0.25) == 2 ** 30
    assert DR.threshold(1.0 - 2.0 ** -40) == 2 ** 32 - 1                      # llrint gives 2^32: clamped
    assert DR.threshold(0.1) == int(np.rint(0.1 * 2.0 ** 32)) == 429496730
    assert DR.cd_of(0.0, np.float32) == 1 and DR.cd_of(0.5, np.float64) == 2 and DR.cd_of(0.6, np.float32) == np.float32(2.5)
    assert DR.cd_of(0.1, np.float32) == np.float32(1.0 / 0.9) and DR.cd_of(0.1, np.float32).dtype == np.float32


def test_kept_fraction_of_the_reference_mask():
    """15 000 draws (3 000 entries, 5 heads: two Philox word groups) at seed 0x1234 and offset 7: the dropped fraction within 4
    binomial sigma of p.  Deterministic"""
    n = 15000
    for p in (0.1, 0.5, 0.6):
        m = DR.mask(3000, 5, p, 0x1234, 7)
        assert m.dtype == np.uint8 and m.shape == (3000, 5) and set(np.unique(m)) <= {0, 1}
        dropped = 1.0 - m.mean()
        print(f"p = {p}: dropped {dropped:.4f}")
        assert abs(dropped - p) <= 4 * np.sqrt(p * (1 - p) / n), (p, dropped)
    assert DR.mask(100, 3, 0.0, 1, 2).all()                                   # thr = 0 drops nothing
    # a pure function of (seed, offset, entry, absolute head): head0 moves the columns, another offset or seed another mask
    full = DR.mask(500, 8, 0.5, 2 ** 63 + 5, 2 ** 32 + 1)
    assert np.array_equal(DR.mask(500, 5, 0.5, 2 ** 63 + 5, 2 ** 32 + 1, head0=3), full[:, 3:8])
    assert not np.array_equal(DR.mask(500, 8, 0.5, 2 ** 63 + 5, 2 ** 32 + 2), full)
    assert not np.array_equal(DR.mask(500, 8, 0.5, 2 ** 63 + 5, 1), full)      # the high offset word is part of the counter
    assert not np.array_equal(DR.mask(500, 8, 0.5, 5, 2 ** 32 + 1), full)      # the high seed word is part of the key


# ---- rejection --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("fp64", "fp32"))
def test_the_reference_rejects_two_wrong_kernels(dtype):
    """what two wrong kernels would compute, judged by the allowance of the float64 comparison (STAGES = 8).  Z over the kept entries
    only is a softmax over the survivors: everything misses.  The mask by the companion's position gives the column side another
    mask than the row side: dK and dV miss, the row side's O, dQ and dB do not."""
    for mat in _small():
        heads, k, d = 3, 3, 5
        rng = np.random.default_rng([41, mat.nnz])
        Q = (rng.uniform(-1, 1, (mat.m, heads, k)) * 2).astype(dtype)
        K, V, dO = (rng.uniform(-1, 1, s).astype(dtype) for s in ((mat.n, heads, k), (mat.n, heads, d), (mat.m, heads, d)))
        bias = rng.uniform(-2, 2, (mat.nnz, heads)).astype(dtype)
        c = float(dtype(0.5))
        keep, cd = DR.mask(mat.nnz, heads, 0.5, 77, 3), DR.cd_of(0.5, dtype)
        assert 0 < keep.mean() < 1
        rho, ref, allow = DR.allowances(mat, c, bias, Q, K, V, dO, keep, cd, dtype, 8)
        assert 8 * rho <= 2.0 ** -6
        for r, al, n in zip(ref, allow, DR.NAMES):  # the reference passes its own allowance when rounded to the type: it is not empty
            assert DR.compare(r.astype(dtype), r, al, n) <= 1.0, n

        def misses(wrong):
            got = DR.numpy_reference(mat, c, bias, Q, K, V, dO, keep, cd, wrong=wrong)[0]
            out = []
            for g, r, al, n in zip(got, ref, allow, DR.NAMES):
                try:
                    bad = DR.compare(g, r, al, n) > 1.0
                except AssertionError:  # (NaN where the reference has none: a row whose every entry is dropped under the wrong Z)
                    bad = True
                if bad:
                    out.append(n)
            return out
        assert misses("z-over-kept") == list(DR.NAMES), mat.name
        assert misses("mask-by-companion-position") == ["dK", "dV"], mat.name


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_five_symbols_with_the_declared_signatures():
    import torch  # noqa: F401  (one HIP runtime per process: see _capi.load)
    lib = C.CDLL(_capi.LIB_PATH)
    with open(os.path.join(INC, "csr5hip.h")) as f:
        assert '#include "csr5hip_dropout.h"' in f.read()  # (csr5hip.h brings the declarations in: users include that header)
    with open(os.path.join(INC, "csr5hip_dropout.h")) as f:
        raw = f.read()
    text = re.sub(r"\s+", " ", raw)
    for name, decl in DECLS.items():
        assert hasattr(lib, name)
        assert decl in text, name
    assert "replay" in raw and "by-value" in raw.lower()                      # the header says what a captured call repeats
    declared = sorted(set(re.findall(r"\b(csr5hip_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", raw, flags=re.S))))
    assert declared == sorted(DECLS) == sorted(n for n, _, _ in _capi.SYMBOLS_DROPOUT)
    bound = {name: (res, args) for name, res, args in _capi.SYMBOLS_DROPOUT}
    p, i, dbl, ull = C.c_void_p, C.c_int, C.c_double, C.c_ulonglong
    tail = [dbl, ull, ull, i]
    fwd, bwd = [p, i, p, i, i, p, i, i, p, i], [p, i, p, i, i, p, i, i, p, i, p, i, p, i, p, i, p, p, i]
    assert bound == {"csr5hip_dropout_mha": (i, [p, i, dbl, p, i] + fwd + tail),
                     "csr5hip_dropout_mha_backward": (i, [p, i, dbl, p, i] + bwd + tail),
                     "csr5hip_dropout_gat": (i, [p, i, dbl, p, dbl, p, i] + fwd + tail),
                     "csr5hip_dropout_gat_backward": (i, [p, i, dbl, p, dbl, p, i] + bwd + [p, i] + tail),
                     "csr5hip_dropout_mask": (i, [p, i, dbl, ull, ull, i, p, i])}
    loaded = _capi.load()
    for name in bound:
        assert getattr(loaded, name).argtypes == bound[name][1], name          # load() binds them
    others = (_capi.SYMBOLS + _capi.SYMBOLS_BIASED + _capi.SYMBOLS_EDGE_BIAS + _capi.SYMBOLS_LOWP + _capi.SYMBOLS_LOWP_BACKWARD
              + _capi.SYMBOLS_GAT)
    assert not {n for n, _, _ in others} & set(bound)                          # (the other lists are as they were)


def test_cpp_class_has_the_dropout_members(tmp_path):
    src = tmp_path / "use_dropout.cpp"
    src.write_text(
        '#include "anonymouslib_hip.h"\n'
        "int use(anonymouslibHandle<int, unsigned, double> &A, const double *a, const double *B, const double *Q, const double *K,\n"
        "        const double *V, const double *dO, double *O, double *dQ, double *dK, double *dV, double *work, double *dB, double *dAr,\n"
        "        unsigned char *mask)\n"
        "{ return A.dropoutMha(4, 0.25, B, 6, Q, 32, K, 32, 8, V, 64, 16, O, 64, 0.1, 9ull, 3ull, 0)\n"
        "       + A.dropoutMhaBackward(4, 0.25, B, 6, Q, 32, K, 32, 8, V, 64, 16, dO, 64, dQ, 32, dK, 32, dV, 64, work, dB, 4, 0.1, 9ull, 3ull, 0)\n"
        "       + A.dropoutGat(4, 0.2, a, 0.25, B, 6, Q, 32, K, 32, 8, V, 64, 16, O, 64, 0.6, 9ull)\n"
        "       + A.dropoutGatBackward(4, 0.2, a, 0.25, B, 6, Q, 32, K, 32, 8, V, 64, 16, dO, 64, dQ, 32, dK, 32, dV, 64, work, dB, 4, dAr, 32,\n"
        "                              0.6, 9ull, 1ull, 2)\n"
        "       + A.dropoutMask(4, 0.6, 9ull, 1ull, 2, mask, 4); }\n"
        "int use32(anonymouslibHandle<int, unsigned, float> &A, const float *Q, const float *K, const float *V, float *O)\n"
        "{ return A.dropoutMha(4, 1.0, nullptr, 4, Q, 4, K, 4, 1, V, 64, 16, O, 64, 0.5, 1ull); }\n")
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", f"-I{INC}", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _info_bytes(lib, h):
    info = _capi.Csr5Info()
    assert lib.csr5hip_get_info(h, C.byref(info)) == 0
    return bytes(info)


def test_return_codes_in_order_without_a_gpu():
    """Decided on the host, with fake non-null pointers, on a handle with null arrays (unknown format, then CSR format): p not finite,
    p < 0, p >= 1 and head0 < 0 belong to the FIRST group, before the leading dimensions, the null operands, the companion and the
    format; everything after follows the undropped sibling's order; get_info unchanged throughout"""
    lib = _capi.load()
    h = C.c_void_p()
    assert lib.csr5hip_create(C.byref(h), 10, 12, _capi.F64) == 0
    f = C.c_void_p(64)
    INV, CSR, UNK = _capi.INVALID_ARGUMENT, _capi.UNSUPPORTED_CSR_SPMV, _capi.UNKOWN_FORMAT

    def mha(heads=3, scale=0.5, B=f, ldb=3, Q=f, ldq=12, K=f, ldk=12, k=4, V=f, ldv=15, d=5, O=f, ldo=15, p=0.5, seed=1, offset=2, head0=0,
            handle=h):
        return lib.csr5hip_dropout_mha(handle, heads, scale, B, ldb, Q, ldq, K, ldk, k, V, ldv, d, O, ldo, p, seed, offset, head0)

    def mha_b(heads=3, scale=0.5, B=f, ldb=3, Q=f, ldq=12, K=f, ldk=12, k=4, V=f, ldv=15, d=5, dO=f, lddo=15, dQ=f, lddq=12, dK=None,
              lddk=12, dV=None, lddv=15, work=None, dB=None, lddb=3, p=0.5, seed=1, offset=2, head0=0, handle=h):
        return lib.csr5hip_dropout_mha_backward(handle, heads, scale, B, ldb, Q, ldq, K, ldk, k, V, ldv, d, dO, lddo, dQ, lddq, dK, lddk,
                                                dV, lddv, work, dB, lddb, p, seed, offset, head0)

    def gat(heads=3, ns=0.2, a=f, scale=0.5, B=f, ldb=3, Q=f, ldq=12, K=f, ldk=12, k=4, V=f, ldv=15, d=5, O=f, ldo=15, p=0.5, seed=1,
            offset=2, head0=0, handle=h):
        return lib.csr5hip_dropout_gat(handle, heads, ns, a, scale, B, ldb, Q, ldq, K, ldk, k, V, ldv, d, O, ldo, p, seed, offset, head0)

    def gat_b(heads=3, ns=0.2, a=f, scale=0.5, B=f, ldb=3, Q=f, ldq=12, K=f, ldk=12, k=4, V=f, ldv=15, d=5, dO=f, lddo=15, dQ=f, lddq=12,
              dK=None, lddk=12, dV=None, lddv=15, work=None, dB=None, lddb=3, dAr=None, lddar=12, p=0.5, seed=1, offset=2, head0=0,
              handle=h):
        return lib.csr5hip_dropout_gat_backward(handle, heads, ns, a, scale, B, ldb, Q, ldq, K, ldk, k, V, ldv, d, dO, lddo, dQ, lddq, dK,
                                                lddk, dV, lddv, work, dB, lddb, dAr, lddar, p, seed, offset, head0)

    def mask(heads=3, p=0.5, seed=1, offset=2, head0=0, m=f, ldm=3, handle=h):
        return lib.csr5hip_dropout_mask(handle, heads, p, seed, offset, head0, m, ldm)

    calls, backs = (mha, mha_b, gat, gat_b), (mha_b, gat_b)
    bad_drop = (dict(p=float("nan")), dict(p=float("inf")), dict(p=-float("inf")), dict(p=-0.25), dict(p=1.0), dict(p=1.5), dict(head0=-1))
    before = _info_bytes(lib, h)
    for call in calls:  # the unknown state: before inputCSR
        assert call(handle=None) == INV
        assert call() == UNK and call(B=None) == UNK and call(p=0.0) == UNK and call(p=1.0 - 2.0 ** -40) == UNK
        assert call(seed=2 ** 64 - 1, offset=2 ** 64 - 1, head0=2 ** 31 - 1 - 3) == UNK  # (3 heads: the last absolute head is INT_MAX - 1)
        assert call(head0=2 ** 31 - 3) == INV and call(head0=2 ** 31 - 1) == INV         # head0 + heads beyond INT_MAX
        assert call(heads=0, head0=2 ** 31 - 1) == UNK
        assert call(heads=-1) == INV and call(k=-1) == INV and call(d=-1) == INV and call(scale=float("nan")) == INV
        for bad in bad_drop:
            assert call(**bad) == INV, bad
            assert call(heads=0, **bad) == INV, bad                            # before the successful no-op of heads = 0
        assert call(ldq=11) == INV and call(ldb=2) == INV
    for call in backs:
        assert call(dK=f, work=f) == INV and "csr5hip_build_transpose" in _capi.last_error() and call.__name__[:3] in ("mha", "gat")
        assert "csr5hip_dropout_" in _capi.last_error()
    assert mask(handle=None) == INV and mask() == UNK and mask(m=None) == UNK and mask(heads=0, ldm=0) == UNK
    assert mask(heads=-1) == INV and mask(ldm=2) == INV and mask(head0=2 ** 31 - 3) == INV and mask(head0=2 ** 31 - 4) == UNK
    for bad in bad_drop:
        assert mask(**bad) == INV, bad
    assert lib.csr5hip_input_csr(h, 100, None, None, None) == 0                # CSR format, nnz > 0: no CSR5 structure
    before = _info_bytes(lib, h)
    for call in calls:
        assert call() == CSR and call(heads=0) == CSR and call(p=0.0) == CSR
        for bad in bad_drop:
            assert call(**bad) == INV, bad
            assert call(Q=None, **bad) == INV and call(ldq=11, **bad) == INV   # (every one of them INVALID_ARGUMENT: the group is one)
        for bad in (dict(ldq=11), dict(ldk=11), dict(ldv=14), dict(ldb=2), dict(Q=None), dict(K=None), dict(V=None)):
            assert call(**bad) == INV, bad
    assert mha(O=None) == INV and gat(O=None) == INV and mha(ldo=14) == INV
    for call in backs:
        for bad in (dict(lddq=11), dict(lddo=14), dict(dB=f, lddb=2), dict(dO=None), dict(dK=f), dict(dV=f)):
            assert call(**bad) == INV, bad
        assert call(dQ=None, dB=f) == CSR and call(Q=None, K=None, V=None, dO=None, dQ=None) == CSR
        assert call(dK=f, work=f) == INV and "csr5hip_build_transpose" in _capi.last_error()   # the companion before the format
        assert call(dK=f, work=f, p=1.0) == INV
    assert gat_b(dAr=f, lddar=11) == INV and gat_b(dQ=None, dAr=f) == CSR
    # the mask needs only nnz: CSR format is served (a null mask with entries and heads is a mistake; the launch itself needs a GPU)
    assert mask(m=None) == INV and mask(heads=0, ldm=0, m=None) == 0 and mask(ldm=2) == INV
    assert _info_bytes(lib, h) == before
    assert lib.csr5hip_free(h) == 0


# ---- the Python layers ------------------------------------------------------------------------------------------------------------------
def test_python_methods_reject_bad_arguments_before_the_library():
    torch = pytest.importorskip("torch")
    A = H.anonymouslibHandle(6, 4)
    calls = []
    for name in ("dropout_mha_ptr", "dropout_mha_backward_ptr", "dropout_gat_ptr", "dropout_gat_backward_ptr", "dropout_mask_ptr"):
        setattr(A, name, lambda *a: calls.append(a) or 0)  # nothing may reach the library
    f64 = torch.float64
    z = lambda *s: torch.zeros(*s, dtype=f64)  # noqa: E731
    fwd = dict(Q=z(6, 2, 3), K=z(4, 2, 3), V=z(4, 2, 5), O=z(6, 2, 5))
    bwd = dict(Q=z(6, 2, 3), K=z(4, 2, 3), V=z(4, 2, 5), dO=z(6, 2, 5), dQ=z(6, 2, 3), dK=z(4, 2, 3), dV=z(4, 2, 5), work=z(48))
    methods = ((A.dropoutMha, fwd), (A.dropoutMhaBackward, bwd), (A.dropoutGat, fwd), (A.dropoutGatBackward, bwd))
    for method, good in methods:
        with pytest.raises(ValueError, match="inputCSR"):
            method(**good, p=0.5, seed=1)
    with pytest.raises(ValueError, match="inputCSR"):
        A.dropoutMask(torch.zeros(7, 2, dtype=torch.uint8), 0.5, 1)
    assert A.inputCSR(7, None, None, None) == 0
    for method, good in methods:
        with pytest.raises(ValueError, match="GPU"):
            method(**good, p=0.5, seed=1, offset=2, head0=3)                   # host tensors: everything else is in order
        for bad in (float("nan"), float("inf"), -0.1, 1.0, 2, None, "0.5", True, z(1)):
            with pytest.raises(ValueError, match=" p must"):
                method(**good, p=bad, seed=1)
        for bad in (-1, 2 ** 64, 1.0, None, "1", True, z(1)):
            with pytest.raises(ValueError, match=" seed must"):
                method(**good, p=0.5, seed=bad)
            with pytest.raises(ValueError, match=" offset must"):
                method(**good, p=0.5, seed=1, offset=bad)
        for bad in (-1, 2 ** 31, 1.0, None, True):
            with pytest.raises(ValueError, match=" head0 must"):
                method(**good, p=0.5, seed=1, head0=bad)
        with pytest.raises(ValueError, match=" p must"):                       # p is judged first: before the tensors
            method(**dict(good, Q=None), p=1.0, seed=1)
        with pytest.raises(ValueError, match="Q has 2 heads, K 3"):
            method(**dict(good, K=z(4, 3, 3)), p=0.5, seed=1)
        with pytest.raises(ValueError, match=" B .*shape"):
            method(**good, p=0.5, seed=1, B=z(7, 3))
        with pytest.raises(ValueError, match="scale"):
            method(**good, p=0.5, seed=1, scale=float("nan"))
    with pytest.raises(ValueError, match="negative_slope"):
        A.dropoutGat(**fwd, p=0.5, seed=1, negative_slope=float("inf"))
    with pytest.raises(ValueError, match="work .*shape"):
        A.dropoutMhaBackward(**dict(bwd, work=z(47)), p=0.5, seed=1)
    with pytest.raises(ValueError, match="dAr shares storage with Q"):
        pool = z(2, 6, 2, 3)
        A.dropoutGatBackward(**dict(bwd, Q=pool[0]), p=0.5, seed=1, dAr=pool[1])
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)  # noqa: E731
    for bad, word in ((np.zeros((7, 2), dtype=np.uint8), "tensor"), (z(7, 2), "dtype"), (u8(7), "shape"), (u8(6, 2), "shape"),
                      (u8(7, 4)[:, ::2], "stride"), (u8(7, 2), "GPU")):
        with pytest.raises(ValueError, match=f"mask .*{word}"):
            A.dropoutMask(bad, 0.5, 1)
    with pytest.raises(ValueError, match=" p must"):
        A.dropoutMask(u8(7, 2), 1.0, 1)
    assert calls == []
    # the wrappers stay out of the table of the twelve: their names begin with "dropout"
    from scripts import attention_wrapper_transcript as T
    assert len(T.METHODS) == 12 and not any(m.lower().startswith("dropout") for m in T.METHODS)
    assert all(hasattr(H.anonymouslibHandle, n) for n in ("dropoutMha", "dropoutMhaBackward", "dropoutGat", "dropoutGatBackward",
                                                          "dropoutMask"))
    A.close()


def test_the_wrappers_pass_the_siblings_arguments_and_the_four_numbers():
    """with the checks of the devices out of the way (the transcript script's proxy): what reaches the *_ptr methods is the undropped
    sibling's tuple followed by (p, seed, offset, head0)"""
    torch = pytest.importorskip("torch")
    from scripts import attention_wrapper_transcript as T
    A = H.anonymouslibHandle(6, 4)
    assert A.inputCSR(7, None, None, None) == 0
    got = {}
    for name in ("dropout_mha_ptr", "mha_edge_bias_ptr", "dropout_gat_backward_ptr", "gat_backward_ptr"):
        setattr(A, name, lambda *a, _n=name: got.__setitem__(_n, a) or 0)
    g = lambda *s: T.OnGpu(torch.zeros(*s, dtype=torch.float64))  # noqa: E731
    fwd = dict(Q=g(6, 2, 3), K=g(4, 2, 3), V=g(4, 2, 5), O=g(6, 2, 5))
    B = g(7, 2)
    assert A.dropoutMha(**fwd, p=0.25, seed=2 ** 63 + 5, offset=2 ** 32 + 1, head0=3, B=B, scale=0.5) == 0
    assert A.mhaEdgeBias(**fwd, B=B, scale=0.5) == 0
    assert got["dropout_mha_ptr"][:-4] == got["mha_edge_bias_ptr"] and got["dropout_mha_ptr"][-4:] == (0.25, 2 ** 63 + 5, 2 ** 32 + 1, 3)
    bwd = dict(Q=g(6, 2, 3), K=g(4, 2, 3), V=g(4, 2, 5), dO=g(6, 2, 5), dQ=g(6, 2, 3), dK=g(4, 2, 3), dV=g(4, 2, 5), work=g(48))
    more = dict(a=g(2, 3), negative_slope=0.1, B=B, scale=0.5, dB=g(7, 2), dAr=g(6, 2, 3))
    assert A.dropoutGatBackward(**bwd, p=0.6, seed=9, **more) == 0
    assert A.gatBackward(**bwd, **more) == 0
    assert got["dropout_gat_backward_ptr"][:-4] == got["gat_backward_ptr"] and got["dropout_gat_backward_ptr"][-4:] == (0.6, 9, 0, 0)
    A.close()


def test_autograd_functions_route_and_are_documented_without_a_gpu(monkeypatch):
    torch = pytest.importorskip("torch")
    from benchmark_spmv_using_csr5_amd import autograd
    for name in ("dropout_attention", "gat_dropout_attention"):
        assert name in autograd.__all__ and callable(getattr(autograd, name))
    assert list(inspect.signature(autograd.dropout_attention).parameters) == ["A", "Q", "K", "V", "p", "seed", "offset", "scale", "bias",
                                                                                "training"]
    assert list(inspect.signature(autograd.gat_dropout_attention).parameters) == ["A", "Q", "K", "V", "p", "seed", "offset", "att",
                                                                                    "negative_slope", "scale", "bias", "training"]
    assert inspect.signature(autograd.dropout_attention).parameters["training"].default is True
    for word in ("offset = step", "dropoutMha", "dropoutMhaBackward", "training=False", "(nnz, H)"):
        assert word in autograd.dropout_attention.__doc__, word
    for word in ("GATConv", "dropoutGat", "dropoutGatBackward", "offset = step"):
        assert word in autograd.gat_dropout_attention.__doc__, word
    seen = []
    monkeypatch.setattr(autograd, "multihead_attention", lambda *a, **kw: seen.append(("mha", a, kw)) or "undropped")
    monkeypatch.setattr(autograd, "gat_attention", lambda *a, **kw: seen.append(("gat", a, kw)) or "undropped-gat")
    monkeypatch.setattr(autograd._DropoutAttention, "apply", staticmethod(lambda *a: seen.append(("drop", a)) or "dropped"))
    monkeypatch.setattr(autograd._GatDropoutAttention, "apply", staticmethod(lambda *a: seen.append(("gatdrop", a)) or "dropped-gat"))
    bias = torch.zeros(3, 2)
    # training=False and p == 0 reach the undropped functions with the caller's scale and bias
    assert autograd.dropout_attention("A", "Q", "K", "V", 0.6, 7, offset=3, scale=0.5, bias=bias, training=False) == "undropped"
    assert autograd.dropout_attention("A", "Q", "K", "V", 0.0, 7) == "undropped"
    assert autograd.dropout_attention("A", "Q", "K", "V", 0.6, 7, training=False) == "undropped"
    assert [s[0] for s in seen] == ["mha"] * 3 and seen[0][1] == ("A", "Q", "K", "V")
    assert seen[0][2]["scale"] == 0.5 and seen[0][2]["bias"] is bias and sorted(seen[0][2]) == ["bias", "scale"]
    assert seen[1][2] == dict(scale=None, bias=None)
    assert autograd.gat_dropout_attention("A", "Q", "K", "V", 0.6, 7, att="a", negative_slope=0.1, scale=2.0, bias=bias,
                                          training=False) == "undropped-gat"
    assert autograd.gat_dropout_attention("A", "Q", "K", "V", 0, 7) == "undropped-gat"
    assert seen[3][0] == "gat" and seen[3][2]["bias"] is bias
    assert {k: v for k, v in seen[3][2].items() if k != "bias"} == dict(att="a", negative_slope=0.1, scale=2.0)
    # training: the dropped Functions, with the numbers as given
    del seen[:]
    assert autograd.dropout_attention("A", "Q", "K", "V", 0.6, 2 ** 63, offset=5, scale=0.5, bias=bias) == "dropped"
    assert len(seen) == 1 and seen[0][0] == "drop" and seen[0][1][5] is bias
    assert seen[0][1][:5] + seen[0][1][6:] == ("A", "Q", "K", "V", 0.5, 0.6, 2 ** 63, 5)
    del seen[:]
    assert autograd.gat_dropout_attention("A", "Q", "K", "V", 0.1, 4, offset=9, att="a") == "dropped-gat"
    assert seen == [("gatdrop", ("A", "Q", "K", "V", "a", 0.2, 1.0, None, 0.1, 4, 9))]
    # a scale without a bias in evaluation: multihead_attention would read the handle's values, so the route is the dropped one at p = 0
    del seen[:]
    assert autograd.dropout_attention("A", "Q", "K", "V", 0.6, 7, scale=0.5, training=False) == "dropped"
    assert seen == [("drop", ("A", "Q", "K", "V", 0.5, None, 0.0, 7, 0))]
    for fn in (autograd.dropout_attention, autograd.gat_dropout_attention):
        with pytest.raises(ValueError, match="2-D"):
            fn(None, None, None, None, 0.5, 1, bias=np.zeros(3))
        for bad in (1.0, -0.5, None, True, "0.1"):
            with pytest.raises(ValueError, match=" p must"):
                fn(None, None, None, None, bad, 1)
        for bad in (-1, 2 ** 64, 0.5, None):
            with pytest.raises(ValueError, match=" seed must"):
                fn(None, None, None, None, 0.5, bad)
            with pytest.raises(ValueError, match=" offset must"):
                fn(None, None, None, None, 0.5, 1, offset=bad)


# ---- the host emulation -----------------------------------------------------------------------------------------------------------------
def _sanitizers_link(cxx, tmp_path):
    src = tmp_path / "probe.cpp"
    src.write_text("int main() { return 0; }\n")
    r = subprocess.run([cxx, "-fsanitize=address,undefined", str(src), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    return r.returncode == 0 and subprocess.run([str(tmp_path / "probe")]).returncode == 0


def test_host_emulation_under_the_sanitizers(tmp_path):
    """scripts/host_emulation/run_dropout.py: a stand-alone program built from the kernel sources with -fsanitize=address,undefined;
    kat0 and duplicates; 1, 3 and 5 heads (5 crosses a Philox word group); both precisions; the mask kernel, forward and backward of
    the dot-product and of the additive family against the numpy float64 reference with the reference mask.  Every buffer is a heap
    block of exactly its size, the padded configuration has NaN in all padding, the patterns carry no value array."""
    cxx = "/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else "clang++"
    try:
        linked = _sanitizers_link(cxx, tmp_path)
    except OSError:
        linked = False
    if not linked:
        pytest.skip(f"{cxx} cannot link a program with -fsanitize=address,undefined (no sanitizer runtime)")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "host_emulation", "run_dropout.py"), "--matrices", "kat0,duplicates",
                        "--heads", "1,3,5", "--cxx", cxx], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.count(": ok") == 12 and r.stdout.count("duplicates") == 6 and r.stdout.count("heads=5 k=3 d=5: ok") == 4, r.stdout
