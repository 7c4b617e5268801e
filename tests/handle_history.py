"""Handles with a history: the ways a converted handle comes to be other than inputCSR -> options -> asCSR5, a battery that runs
every pattern operation once on such a handle, and a bit-for-bit comparator.  Used by tests/test_gpu_handle_history.py; what needs
no GPU is checked in tests/test_handle_history_host.py.  Importing this module needs no GPU (torch is imported where it is used).

WHY BIT FOR BIT.  sddmm, rowSoftmax and every attention call promise bits that do not depend on sigma, path or options, and SpMV /
SpMM promise run-to-run identical bits for one conversion (include/csr5hip.h).  A handle that was loaded, reconverted, given a
second matrix or had options switched must therefore agree in every word with a FRESH handle of the same sigma and the same
effective options -- its TWIN.  A stale table, value array or source map shows as a wrong word, not as a rounding difference.

THE VALUES (``values``) are distinct per entry -- (a permutation of 0 .. nnz-1, centred) * 2**-s, in [-2, 2) -- so a value taken from
another entry's position is an error of order one; with the integer x of the battery (0 .. 9) every product is exact in fp32 and
fp64 (at most 17 + 4 bits for nnz < 2**17), which is what tests/exact_reference.py's order-free bound ("wide_range") asks for.
``fine=True`` multiplies by (1 + 2**-30): exact in fp64 (47 bits, 51 with x), not representable in fp32 -- values that
CSR5HIP_OPT_NARROW_VALUES must not narrow."""
from __future__ import annotations

import os
from dataclasses import dataclass

import numpy as np

from benchmark_spmv_using_csr5_amd import _capi
from benchmark_spmv_using_csr5_amd import handle as H
from benchmark_spmv_using_csr5_amd import matrices as M
from tests import attention_edges as E
from tests import edge_bias_reference as EB
from tests import lowp_reference as L
from tests import sddmm_reference as S
from tests import softmax_reference as SM
from tests.test_gpu_exact_reference import DEV, PATHS, Y0, Path, _close, _handle

AUTO = H.ANONYMOUSLIB_AUTO_TUNED_SIGMA
BY_NAME = {p.name: p for p in PATHS}
POISON_WORD = 0x5A5A  # (a finite number in bf16 and fp16, far above any output of operands in [-1, 1))
MHA = (3, 3, 5)       # heads, k, d of the packed calls
ONE = (8, 16)         # k, d of the single-head calls: 16-byte loads
LOWP = (2, 16, 16)
SCALE = 0.25
PARTS = ("products", "pattern", "attention", "lowp", "update", "autograd")


def _torch():
    import torch
    return torch


def _tdt(dtype):
    torch = _torch()
    return torch.float64 if np.dtype(dtype) == np.float64 else torch.float32


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).to(DEV)


def _host(t):
    return t.detach().cpu().numpy()


# ---- values and patterns ---------------------------------------------------------------------------------------------------------
def values(mat, seed, dtype, fine=False):
    """(nnz,) of `dtype`: see the module docstring"""
    nnz = mat.nnz
    bits = max(int(np.ceil(np.log2(max(nnz, 2)))), 2)
    assert bits <= 20, "the products with x in 0 .. 9 would not be exact in fp32"
    v = (np.random.default_rng([seed, nnz]).permutation(nnz) - nnz // 2).astype(np.float64) * 2.0 ** -(bits - 2)
    if fine:
        assert np.dtype(dtype) == np.float64
        v = v * (1 + 2.0 ** -30)
    return v.astype(dtype)


def second_pattern(P):
    """Q for the ``second-matrix`` history: P's rows in reverse order (each with its own columns), every third row emptied"""
    lens = np.diff(P.row_ptr).astype(np.int64)
    src = np.arange(P.m)[::-1]
    keep = np.arange(P.m) % 3 != 0
    qlens = np.where(keep, lens[src], 0)
    row_ptr = np.zeros(P.m + 1, dtype=np.int32)
    row_ptr[1:] = np.cumsum(qlens)
    col = np.concatenate([P.col[P.row_ptr[s]:P.row_ptr[s + 1]] for s, k in zip(src, keep) if k] or [np.zeros(0, dtype=np.int32)])
    return M.CsrMatrix(P.m, P.n, row_ptr, col.astype(np.int32), np.zeros(int(qlens.sum())), P.name + "-reversed-thinned")


def transposed(mat, val):
    """(A^T in CSR with every column's entries in A's CSR order, the values in that order)"""
    order = np.argsort(mat.col[:mat.nnz].astype(np.int64), kind="stable")
    return EB.transposed(mat), np.ascontiguousarray(val[order])


# ---- the operands of the battery, from the seed ------------------------------------------------------------------------------------
_OPERANDS = {}


def operands(mat, dtype, seed):
    """every input of ``battery`` as numpy arrays (16-bit operands as uint16 words): a function of (mat, dtype, seed) alone, so the
    history handle, its twin and the float64 references see the same numbers"""
    key = (mat.name, mat.m, mat.n, mat.nnz, np.dtype(dtype).name, seed)
    if key in _OPERANDS:
        return _OPERANDS[key]
    dt = np.float64 if np.dtype(dtype) == np.float64 else np.float32
    rng = np.random.default_rng([seed, mat.m, mat.n, mat.nnz, 64 if dt == np.float64 else 32])
    ints = lambda *shape: rng.integers(0, 10, size=shape).astype(dt)  # noqa: E731
    uni = lambda *shape: rng.uniform(-1, 1, size=shape).astype(dt)  # noqa: E731
    o = dict(x=ints(mat.n), X3=ints(mat.n, 3), xt=ints(mat.m), Xt3=ints(mat.m, 3))
    o["U13"], o["V13"] = S.make("integer", mat, 13, dt, seed)
    o["U8"], o["V8"] = S.make("integer", mat, 8, dt, seed)
    o["scores"] = SM.make_scores("uniform", mat.row_ptr, dt, seed)
    o["p"], o["g"] = SM.make_grad("softmax", mat.row_ptr, dt, seed)
    k, d = ONE
    o["Q1"], o["K1"], o["V1"], o["dO1"] = uni(mat.m, k) * dt(2), uni(mat.n, k), uni(mat.n, d), uni(mat.m, d)
    heads, k, d = MHA
    o["B"], _, (o["Q"], o["K"], o["V"], o["dO"]) = EB.case(mat, heads, k, d, dt, seed)
    o["slopes"] = rng.uniform(-1.5, 1.5, size=heads).astype(dt)
    for kind in L.KINDS:
        o["lowp." + kind], scale = L.f64_case(mat, kind, *LOWP, seed=seed)
        assert scale == SCALE
    o["v2"], o["v3"], o["bias1d"] = values(mat, seed + 1, dt), values(mat, seed + 2, dt), values(mat, seed + 3, dt)
    o["dY3"] = rng.integers(-4, 6, size=(mat.m, 3)).astype(dt)
    o["X3i"] = rng.integers(-4, 6, size=(mat.n, 3)).astype(dt)
    _OPERANDS[key] = o
    return o


# ---- the battery -------------------------------------------------------------------------------------------------------------------
def battery(A, mat, dtype, seed, parts=PARTS):
    """every operation once on the converted handle A (which holds the values the caller knows); dict name -> numpy array of every
    output, in a fixed order.  Outputs that a call promises to write everywhere start as NaN (16-bit: POISON_WORD) and are
    asserted to be written; the products start as Y0, which rows without entries keep (tests/exact_reference.py).
    ``A.last_values`` is set to the values the handle holds afterwards, in CSR order."""
    torch = _torch()
    tdt = _tdt(dtype)
    o = operands(mat, dtype, seed)
    res = {}
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=tdt, device=DEV)  # noqa: E731
    y0 = lambda *shape: torch.full(shape, Y0, dtype=tdt, device=DEV)  # noqa: E731
    ok = lambda rc: rc == 0 or _fail(rc)  # noqa: E731

    def written(name, t):
        assert not bool(torch.isnan(t).any()), (name, "an element was not written")
        res[name] = _host(t)

    def work(heads):
        return torch.empty(4 * mat.m * heads, dtype=tdt, device=DEV)

    def transpose_built():
        if not A.info().transpose_built:
            ok(A.buildTranspose())

    def spmv(name):
        xd, y = _dev(o["x"]), y0(mat.m)
        ok(A.setX(xd)) and ok(A.spmv(1.0, y))
        torch.cuda.synchronize()
        res[name] = _host(y)

    def spmvT(name):
        xd, y = _dev(o["xt"]), y0(mat.n)
        ok(A.spmvT(xd, y))
        torch.cuda.synchronize()
        res[name] = _host(y)

    def biased(prefix, backward):
        Q, K, V, dO, sl = (_dev(o[n]) for n in ("Q", "K", "V", "dO", "slopes"))
        O = nan(mat.m, MHA[0], MHA[2])
        ok(A.mhaBiased(Q, K, V, O, scale=SCALE, slopes=sl))
        outs = []
        if backward:
            outs = [nan(*t.shape) for t in (Q, K, V)] + [nan(mat.nnz, MHA[0])]
            ok(A.mhaBiasedBackward(Q, K, V, dO, outs[0], outs[1], outs[2], work(MHA[0]), scale=SCALE, slopes=sl, dS=outs[3]))
        torch.cuda.synchronize()
        for name, t in zip(("O", "dQ", "dK", "dV", "dS"), [O] + outs):
            written(f"{prefix}.{name}", t)

    assert A.setStream(None) == 0
    if "products" in parts:
        spmv("spmv")
        X, Y = _dev(o["X3"]), y0(mat.m, 3)
        ok(A.spmm(X, Y))
        torch.cuda.synchronize()
        res["spmm"] = _host(Y)
        transpose_built()
        spmvT("spmvT")
        X, Y = _dev(o["Xt3"]), y0(mat.n, 3)
        ok(A.spmmT(X, Y))
        torch.cuda.synchronize()
        res["spmmT"] = _host(Y)
    if "pattern" in parts:
        for k in (13, 8):
            U, V, out = _dev(o[f"U{k}"]), _dev(o[f"V{k}"]), nan(mat.nnz)
            ok(A.sddmm(U, V, out))
            torch.cuda.synchronize()
            written(f"sddmm{k}", out)
        s, out = _dev(o["scores"]), nan(mat.nnz)
        ok(A.rowSoftmax(s, out))
        torch.cuda.synchronize()
        written("rowSoftmax", out)
        p, g, out = _dev(o["p"]), _dev(o["g"]), nan(mat.nnz)
        ok(A.rowSoftmaxGrad(p, g, out))
        torch.cuda.synchronize()
        written("rowSoftmaxGrad", out)
    if "attention" in parts:
        transpose_built()
        Q, K, V, dO = (_dev(o[n]) for n in ("Q1", "K1", "V1", "dO1"))
        outs = [nan(mat.m, ONE[1])] + [nan(*t.shape) for t in (Q, K, V)]
        ok(A.attention(Q, K, V, outs[0]))
        ok(A.attentionBackward(Q, K, V, dO, outs[1], outs[2], outs[3], work(1)))
        torch.cuda.synchronize()
        for name, t in zip(("O", "dQ", "dK", "dV"), outs):
            written("attention." + name, t)
        Q, K, V, dO, B = (_dev(o[n]) for n in ("Q", "K", "V", "dO", "B"))
        outs = [nan(mat.m, MHA[0], MHA[2])] + [nan(*t.shape) for t in (Q, K, V)]
        ok(A.mha(Q, K, V, outs[0]))
        ok(A.mhaBackward(Q, K, V, dO, outs[1], outs[2], outs[3], work(MHA[0])))
        torch.cuda.synchronize()
        for name, t in zip(("O", "dQ", "dK", "dV"), outs):
            written("mha." + name, t)
        biased("mhaBiased", True)
        outs = [nan(mat.m, MHA[0], MHA[2])] + [nan(*t.shape) for t in (Q, K, V)] + [nan(mat.nnz, MHA[0])]
        ok(A.mhaEdgeBias(Q, K, V, outs[0], B=B, scale=SCALE))
        ok(A.mhaEdgeBiasBackward(Q, K, V, dO, outs[1], outs[2], outs[3], work(MHA[0]), B=B, scale=SCALE, dB=outs[4]))
        torch.cuda.synchronize()
        for name, t in zip(("O", "dQ", "dK", "dV", "dB"), outs):
            written("mhaEdgeBias." + name, t)
    if "lowp" in parts:
        for kind in L.KINDS:
            t16 = torch.bfloat16 if kind == "bf16" else torch.float16
            B, Q, K, V = (torch.from_numpy(w.view(np.int16)).to(DEV).view(t16) for w in o["lowp." + kind])
            O = torch.full((mat.m, LOWP[0], LOWP[2]), POISON_WORD, dtype=torch.int16, device=DEV).view(t16)
            ok(A.mhaLowp(Q, K, V, O, B=B, scale=SCALE))
            torch.cuda.synchronize()
            words = O.view(torch.int16).cpu().numpy().view(np.uint16)
            assert not (words == POISON_WORD).any(), ("mhaLowp", kind, "an element was not written")
            res["mhaLowp." + kind] = words
    if "update" in parts:
        v2 = _dev(o["v2"])
        ok(A.updateValues(v2))
        spmv("v2.spmv")
        transpose_built()
        spmvT("v2.spmvT")
        biased("v2.mhaBiased", False)
        A.last_values = o["v2"]
    if "autograd" in parts:
        from benchmark_spmv_using_csr5_amd import autograd
        v3, X = _dev(o["v3"]).requires_grad_(True), _dev(o["X3i"]).requires_grad_(True)
        Y = autograd.spmm(A, v3, X)
        Y.backward(_dev(o["dY3"]))
        torch.cuda.synchronize()
        for name, t in (("Y", Y), ("dval", v3.grad), ("dX", X.grad)):
            written("autograd.spmm." + name, t)
        q, k, v = (_dev(o[n]).requires_grad_(True) for n in ("Q1", "K1", "V1"))
        out = autograd.attention(A, q, k, v)
        out.backward(_dev(o["dO1"]))
        torch.cuda.synchronize()
        for name, t in (("O", out), ("dQ", q.grad), ("dK", k.grad), ("dV", v.grad)):
            written("autograd.attention." + name, t)
        q, k, v, b, sl = (_dev(o[n]).requires_grad_(True) for n in ("Q", "K", "V", "bias1d", "slopes"))
        out = autograd.multihead_attention(A, q, k, v, scale=SCALE, bias=b, slopes=sl)
        out.backward(_dev(o["dO"]))
        torch.cuda.synchronize()
        for name, t in (("O", out), ("dQ", q.grad), ("dK", k.grad), ("dV", v.grad), ("dbias", b.grad), ("dslopes", sl.grad)):
            written("autograd.mha." + name, t)
        A.last_values = o["bias1d"]
    assert A.setStream(None) == 0
    return res


def _fail(rc):
    raise AssertionError(f"a library call returned {rc}: {_capi.last_error()}")


# ---- the comparator ------------------------------------------------------------------------------------------------------------------
def same(results_a, results_b):
    """None when results_a (what a handle with a history gave) equals results_b (its twin's) bit for bit, key for key; else the
    first differing (operation, index) in results_b's order -- index None for a missing key, a dtype or a shape that differs.
    Floats through ``attention_edges.same_bits`` (the sign of zero counts; a NaN is accepted only where results_b has one),
    16-bit words and other integers by value."""
    for name in list(results_b) + [n for n in results_a if n not in results_b]:
        if name not in results_a or name not in results_b:
            return name, None
        got, want = np.ascontiguousarray(results_a[name]), np.ascontiguousarray(results_b[name])
        if got.dtype != want.dtype or got.shape != want.shape:
            return name, None
        if got.dtype.kind != "f":
            if not np.array_equal(got, want):
                return name, tuple(int(i) for i in np.argwhere(got != want)[0])
            continue
        if E.same_bits(got, want):
            continue
        word = np.uint64 if got.dtype == np.float64 else np.uint32
        nan = np.isnan(want)
        bad = np.where(nan, ~np.isnan(got), got.view(word) != want.view(word))
        return name, tuple(int(i) for i in np.argwhere(bad)[0])
    return None


# ---- the histories -----------------------------------------------------------------------------------------------------------------
@dataclass
class Twin:
    """the fresh conversion a history must equal: sigma and the options set before asCSR5; ``mat`` / ``val`` where they are not the
    history's own arguments (the second matrix; the values given last)"""
    sigma: int
    opts: tuple = ()
    mat: object = None
    val: object = None

    def path(self):
        return Path("twin", self.sigma, H.SPMV_FUSED, tuple(self.opts))


@dataclass(frozen=True)
class History:
    build: object        # (mat, val, dtype, tmp_path) -> (handle, Twin)
    sigma: int           # the twin's, known without running anything
    opts: tuple = ()
    loaded: bool = False  # the handle comes from anonymouslibHandle.load (it owns its CSR arrays: ``handle.arrays``)
    file_sigma: int = 0   # loaded: the sigma of the file ``handle.saved_file``

    def twin(self, mat=None, val=None):
        return Twin(self.sigma, self.opts, mat, val)


def fresh(mat, val, dtype, path):
    return _handle(mat, np.asarray(val, dtype=dtype), path, dtype)[0]


def _sigma_path(sigma, **opts):
    return Path("history", sigma, H.SPMV_FUSED, tuple(opts.items()))


def _save_and_load(A, tmp_path, name):
    f = os.path.join(str(tmp_path), name + ".csr5")
    assert A.save(f) == 0, _capi.last_error()
    B = H.anonymouslibHandle.load(f)
    B.saved_file = f
    return B


def _loaded(mat, val, dtype, tmp_path):
    A = fresh(mat, val, dtype, _sigma_path(7))
    B = _save_and_load(A, tmp_path, "loaded")
    _close(A)
    return B, HISTORIES["loaded"].twin()


def _loaded_from_slabs_hot(mat, val, dtype, tmp_path):
    A = fresh(mat, val, dtype, BY_NAME["slabs8-hot"])  # (asserts the path's `expect` where p >= 2)
    B = _save_and_load(A, tmp_path, "slabs-hot")
    _close(A)
    return B, HISTORIES["loaded-from-slabs-hot"].twin()


def _loaded_from_narrow(mat, val, dtype, tmp_path):
    torch = _torch()
    base = BY_NAME["xwin-narrow"]
    A = fresh(mat, val, dtype, Path(base.name, base.sigma, base.mode, base.opts + (("setNarrowValues", 1),), base.expect))
    f64 = np.dtype(dtype) == np.float64
    last = values(mat, 881, dtype, fine=f64)
    if f64 and mat.nnz:
        assert (last.astype(np.float32).astype(np.float64) != last).any()  # they do not narrow losslessly
    lt = _dev(last)
    assert A.updateValues(lt) == 0, _capi.last_error()
    B = _save_and_load(A, tmp_path, "narrow")
    torch.cuda.synchronize()
    _close(A)
    return B, HISTORIES["loaded-from-narrow"].twin(val=last)


def _saved_behind_a_side_stream(mat, val, dtype, tmp_path):
    torch = _torch()
    A = fresh(mat, val, dtype, _sigma_path(7))
    v1 = values(mat, 882, dtype)
    vt = _dev(v1)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert A.setStream(side) == 0
    with torch.cuda.stream(side):  # (about a TFLOP in front of it: the update is still pending when save is called)
        big = torch.ones((4096, 4096), dtype=torch.float32, device=DEV)
        for _ in range(8):
            big = (big @ big).clamp_(0, 1)
    assert A.updateValues(vt) == 0, _capi.last_error()  # enqueued on the side stream ...
    B = _save_and_load(A, tmp_path, "side-stream")      # ... and saved at once: no synchronisation in between
    torch.cuda.synchronize()
    assert A.setStream(None) == 0
    _close(A)
    return B, HISTORIES["saved-behind-a-side-stream"].twin(val=v1)


def _one_backward(A, mat, dtype):
    """one mhaBackward with dK and dV (the column kernel on the companion), on small operands"""
    torch = _torch()
    tdt = _tdt(dtype)
    Q, K, V, dO = (torch.ones((r, 1, 2), dtype=tdt, device=DEV) for r in (mat.m, mat.n, mat.n, mat.m))
    dQ, dK, dV = (torch.empty_like(t) for t in (Q, K, V))
    assert A.mhaBackward(Q, K, V, dO, dQ, dK, dV, torch.empty(4 * mat.m, dtype=tdt, device=DEV)) == 0, _capi.last_error()
    torch.cuda.synchronize()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def _reconverted(mat, val, dtype, tmp_path):
    torch = _torch()
    A = fresh(mat, val, dtype, _sigma_path(32))
    assert A.buildTranspose() == 0, _capi.last_error()
    junk = values(mat, 883, dtype)
    jt = _dev(junk)
    assert A.updateValues(jt) == 0, _capi.last_error()
    _one_backward(A, mat, dtype)
    assert A.asCSR() == 0, _capi.last_error()
    torch.cuda.synchronize()
    assert np.array_equal(_host(A._arrays[1]), mat.col[:mat.nnz].astype(np.int32))  # the caller's col: its original bits
    assert np.array_equal(_bits(_host(A._arrays[2])), _bits(junk))                    # val: the junk, in CSR order
    assert A.setSigma(7) == 0 and A.asCSR5() == 0, _capi.last_error()
    vt = _dev(np.asarray(val, dtype=dtype))
    assert A.updateValues(vt) == 0, _capi.last_error()
    torch.cuda.synchronize()
    return A, HISTORIES["reconverted"].twin()


def _loaded_then_reconverted(mat, val, dtype, tmp_path):
    B, _ = _loaded(mat, val, dtype, tmp_path)
    assert B.asCSR() == 0, _capi.last_error()
    owned = B.arrays.to_host()
    assert np.array_equal(owned.row_ptr, mat.row_ptr.astype(np.int32)) and np.array_equal(owned.col, mat.col[:mat.nnz].astype(np.int32))
    assert np.array_equal(_bits(owned.val), _bits(np.asarray(val, dtype=dtype)))
    assert B.setSigma(4) == 0 and B.asCSR5() == 0, _capi.last_error()
    return B, HISTORIES["loaded-then-reconverted"].twin()


def _second_matrix(mat, val, dtype, tmp_path):
    torch = _torch()
    tdt = _tdt(dtype)
    A = fresh(mat, val, dtype, _sigma_path(7))
    assert A.buildTranspose() == 0, _capi.last_error()
    X, Y = torch.ones((mat.n, 3), dtype=tdt, device=DEV), torch.empty((mat.m, 3), dtype=tdt, device=DEV)
    assert A.spmm(X, Y) == 0, _capi.last_error()
    _one_backward(A, mat, dtype)
    A.bytes_first = A.info().device_bytes
    Q = second_pattern(mat)
    qval = values(Q, 884, dtype)
    rp, ci, va = _dev(Q.row_ptr.astype(np.int32)), _dev(Q.col.astype(np.int32)), _dev(qval)
    A._arrays = (rp, ci, va)
    assert A.inputCSR(Q.nnz, rp, ci, va) == 0 and A.asCSR5() == 0, _capi.last_error()
    return A, HISTORIES["second-matrix"].twin(mat=Q, val=qval)


def _second_matrix_under_slabs(mat, val, dtype, tmp_path):
    """the second matrix arrives while the first one's column slabs, hot table and value source map are in use (no asCSR in
    between): nothing of them may survive into the structure built for Q"""
    torch = _torch()
    tdt = _tdt(dtype)
    A = fresh(mat, val, dtype, BY_NAME["slabs8-hot"])
    assert A.buildTranspose() == 0, _capi.last_error()
    other = _dev(values(mat, 885, dtype))
    assert A.updateValues(other) == 0, _capi.last_error()  # (the first update builds the slab child's source map, for P's columns)
    x, y = torch.ones(mat.n, dtype=tdt, device=DEV), torch.empty(mat.m, dtype=tdt, device=DEV)
    assert A.setX(x) == 0 and A.spmv(1.0, y) == 0, _capi.last_error()
    torch.cuda.synchronize()
    Q = second_pattern(mat)
    qval = values(Q, 886, dtype)
    rp, ci, va = _dev(Q.row_ptr.astype(np.int32)), _dev(Q.col.astype(np.int32)), _dev(qval)
    A._arrays = (rp, ci, va)
    assert A.inputCSR(Q.nnz, rp, ci, va) == 0 and A.asCSR5() == 0, _capi.last_error()
    return A, HISTORIES["second-matrix-under-slabs"].twin(mat=Q, val=qval)


TOGGLED = (("setColumnSlabs", 8), ("setSlabHot", 2), ("setZeroEmptyRows", 1))
DEFAULTS = (("setColumnSlabs", 1), ("setSlabHot", 1), ("setZeroEmptyRows", 0))


def _options_toggled(mat, val, dtype, tmp_path, back=False):
    A = fresh(mat, val, dtype, BY_NAME["fused-default"])
    assert A.buildTranspose() == 0, _capi.last_error()
    for setter, value in TOGGLED + (DEFAULTS if back else ()):
        assert getattr(A, setter)(value) == 0, (setter, _capi.last_error())
    return A, HISTORIES["options-toggled-and-back" if back else "options-toggled"].twin()


def _options_toggled_and_back(mat, val, dtype, tmp_path):
    return _options_toggled(mat, val, dtype, tmp_path, back=True)


HISTORIES = {
    "loaded": History(_loaded, 7, loaded=True, file_sigma=7),
    "loaded-from-slabs-hot": History(_loaded_from_slabs_hot, 16, loaded=True, file_sigma=16),
    "loaded-from-narrow": History(_loaded_from_narrow, 16, loaded=True, file_sigma=16),
    "saved-behind-a-side-stream": History(_saved_behind_a_side_stream, 7, loaded=True, file_sigma=7),
    "reconverted": History(_reconverted, 7),
    "loaded-then-reconverted": History(_loaded_then_reconverted, 4, loaded=True, file_sigma=7),
    "second-matrix": History(_second_matrix, 7),
    "second-matrix-under-slabs": History(_second_matrix_under_slabs, 16, BY_NAME["slabs8-hot"].opts),
    "options-toggled": History(_options_toggled, AUTO, TOGGLED),
    "options-toggled-and-back": History(_options_toggled_and_back, AUTO),
}
