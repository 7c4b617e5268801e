"""Python mirror of the reference's ``anonymouslibHandle<int, unsigned int, VALUE_TYPE>``.

Same member names, argument meaning, state machine and integer return codes as
CSR5_cuda/anonymouslib_cuda.h:11-53; every call goes straight through the C ABI of libcsr5hip.so
(include/csr5hip.h).  Arguments are *device* arrays owned by the caller -- here ``torch`` CUDA tensors
(torch is plumbing for device memory and streams only) or raw integer device pointers.  ``asCSR5``
permutes the caller's ``col_idx`` / ``val`` tensors in place, exactly as the reference does.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _capi

ANONYMOUSLIB_SUCCESS = _capi.SUCCESS
ANONYMOUSLIB_UNSUPPORTED_CSR5_OMEGA = _capi.UNSUPPORTED_CSR5_OMEGA
ANONYMOUSLIB_CSR_TO_CSR5_FAILED = _capi.CSR_TO_CSR5_FAILED
ANONYMOUSLIB_UNSUPPORTED_CSR_SPMV = _capi.UNSUPPORTED_CSR_SPMV
ANONYMOUSLIB_UNSUPPORTED_VALUE_TYPE = _capi.UNSUPPORTED_VALUE_TYPE
ANONYMOUSLIB_FORMAT_CSR = _capi.FORMAT_CSR
ANONYMOUSLIB_FORMAT_CSR5 = _capi.FORMAT_CSR5
ANONYMOUSLIB_CSR5_OMEGA = _capi.OMEGA
ANONYMOUSLIB_AUTO_TUNED_SIGMA = _capi.AUTO_TUNED_SIGMA

SPMV_TWO_PASS = 0
SPMV_FUSED = 1


def _ptr(t) -> int:
    if t is None:
        return 0
    if isinstance(t, int):
        return t
    return int(t.data_ptr())


def _value_type(dtype) -> int:
    name = str(dtype)
    if name.endswith("float64"):
        return _capi.F64
    if name.endswith("float32"):
        return _capi.F32
    raise TypeError(f"unsupported VALUE_TYPE {dtype}: only float64 and float32 "
                    "(README.md:71 of the reference)")


def _aliased(a, b) -> bool:
    """whether two tensors are views of one storage (tensors without elements own no memory: their storages all report the same
    null pointer and alias nothing)"""
    return bool(a.numel() and b.numel()) and a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()


def _finite(who: str, name: str, x) -> float:
    """``scale`` and ``negative_slope``: ValueError unless x is a finite Python number"""
    if isinstance(x, bool) or not isinstance(x, (int, float)) or not math.isfinite(x):
        raise ValueError(f"{who}: {name} must be a finite Python number, not {x!r}")
    return float(x)


class anonymouslibHandle:
    """``A = anonymouslibHandle(m, n, dtype)``; then ``inputCSR / setX / setSigma / asCSR5 / spmv /
    destroy`` as in CSR5_cuda/main.cu:59-104."""

    def __init__(self, m: int, n: int, dtype="float64", stream=None):
        self._lib = _capi.load()
        self._h = C.c_void_p()
        self._vt = _value_type(dtype)
        err = self._lib.csr5hip_create(C.byref(self._h), int(m), int(n), self._vt)
        if err:
            raise RuntimeError(f"csr5hip_create -> {err}")
        self._keep = {}  # borrowed tensors, kept alive while the handle points at them
        self._m, self._n = int(m), int(n)
        self._nnz = None  # known after inputCSR
        if stream is not None:
            self.setStream(stream)

    def _dtype_name(self) -> str:
        """the handle's dtype as ``str(tensor.dtype)`` spells it"""
        return "torch.float64" if self._vt == _capi.F64 else "torch.float32"

    # -- reference API ------------------------------------------------------------------------
    def warmup(self) -> int:
        return self._lib.csr5hip_warmup(self._h)

    def inputCSR(self, nnz: int, csr_row_pointer, csr_column_index, csr_value) -> int:
        self._keep.update(row_ptr=csr_row_pointer, col=csr_column_index, val=csr_value)
        self._nnz = int(nnz)
        self._autograd_key = None
        return self._lib.csr5hip_input_csr(self._h, int(nnz), _ptr(csr_row_pointer),
                                           _ptr(csr_column_index), _ptr(csr_value))

    def setX(self, x) -> int:
        self._keep.update(x=x)
        return self._lib.csr5hip_set_x(self._h, _ptr(x))

    def setSigma(self, sigma: int) -> int:
        return self._lib.csr5hip_set_sigma(self._h, int(sigma))

    def asCSR5(self) -> int:
        return self._lib.csr5hip_as_csr5(self._h)

    def asCSR(self) -> int:
        return self._lib.csr5hip_as_csr(self._h)

    def spmv(self, alpha, y) -> int:
        return self._lib.csr5hip_spmv(self._h, float(alpha), _ptr(y))

    def destroy(self) -> int:
        return self._lib.csr5hip_destroy(self._h)

    def spmm(self, X, Y) -> int:
        """Y = A * X for k dense vectors (csr5hip.h csr5hip_spmm): X (n, k) and Y (m, k) device tensors of the handle's
        dtype with stride(1) == 1; the leading dimensions are their stride(0).  Column c of Y equals a two-pass spmv() of
        X[:, c], bit for bit.  Wrong dtype, device, shape or inner stride raise ValueError before the library is called."""
        return self.spmm_ptr(*self._spmm_args("spmm", X, self._n, Y, self._m))

    def _spmm_args(self, who: str, X, x_rows: int, Y, y_rows: int):
        """the checks of spmm / spmmT: (X, ldx, k, Y, ldy) for the C call, or ValueError"""
        dt = self._dtype_name()
        for name, t, rows in (("X", X, x_rows), ("Y", Y, y_rows)):
            if not hasattr(t, "data_ptr") or not hasattr(t, "stride"):
                raise ValueError(f"{who}: {name} must be a torch tensor")
            if str(t.dtype) != dt:
                raise ValueError(f"{who}: {name} has dtype {t.dtype}, the handle holds {dt}")
            if t.dim() != 2 or t.shape[0] != rows:
                raise ValueError(f"{who}: {name} must have shape ({rows}, k), not {tuple(t.shape)}")
            if t.shape[1] > 1 and t.stride(1) != 1:
                raise ValueError(f"{who}: {name} must be row-major with stride(1) == 1, not {t.stride()}")
            if t.shape[0] > 1 and t.stride(0) < t.shape[1]:
                raise ValueError(f"{who}: {name} rows overlap (stride(0) {t.stride(0)} < k = {t.shape[1]})")
            if t.device.type != "cuda":
                raise ValueError(f"{who}: {name} must live on the GPU, not {t.device}")
        if X.shape[1] != Y.shape[1]:
            raise ValueError(f"{who}: X has {X.shape[1]} columns, Y {Y.shape[1]}")
        if X.device != Y.device:
            raise ValueError(f"{who}: X on {X.device}, Y on {Y.device}")
        k = int(X.shape[1])
        ldx = max(int(X.stride(0)), k) if X.shape[0] > 1 else k
        ldy = max(int(Y.stride(0)), k) if Y.shape[0] > 1 else k
        return X, ldx, k, Y, ldy

    def spmm_ptr(self, X, ldx: int, k: int, Y, ldy: int) -> int:
        """csr5hip_spmm on raw device pointers (or tensors): X with leading dimension ldx, Y with ldy"""
        return self._lib.csr5hip_spmm(self._h, _ptr(X), int(ldx), int(k), _ptr(Y), int(ldy))

    # -- products with the transpose (csr5hip.h csr5hip_build_transpose) ---------------------------
    def buildTranspose(self) -> int:
        """Give the converted handle a transposed companion (a library-owned CSR5 form of A^T, built on the device, kept current by
        ``updateValues``): once per conversion, allocates and synchronises.  ``spmvT`` / ``spmmT`` need it."""
        return self._lib.csr5hip_build_transpose(self._h)

    def spmvT(self, x, y) -> int:
        """y = A^T x: x (m,) and y (n,) contiguous GPU tensors of the handle's dtype; the handle's own x (setX) is not involved.
        Wrong dtype, device, shape or stride raise ValueError before the library is called."""
        dt = self._dtype_name()
        for name, t, rows in (("x", x, self._m), ("y", y, self._n)):
            if not hasattr(t, "data_ptr") or not hasattr(t, "is_contiguous"):
                raise ValueError(f"spmvT: {name} must be a torch tensor")
            if str(t.dtype) != dt:
                raise ValueError(f"spmvT: {name} has dtype {t.dtype}, the handle holds {dt}")
            if t.dim() != 1 or t.shape[0] != rows:
                raise ValueError(f"spmvT: {name} must have shape ({rows},), not {tuple(t.shape)}")
            if not t.is_contiguous():
                raise ValueError(f"spmvT: {name} must be contiguous, not stride {t.stride()}")
            if t.device.type != "cuda":
                raise ValueError(f"spmvT: {name} must live on the GPU, not {t.device}")
        if x.device != y.device:
            raise ValueError(f"spmvT: x on {x.device}, y on {y.device}")
        return self.spmvT_ptr(x, y)

    def spmvT_ptr(self, x, y) -> int:
        """csr5hip_spmv_t on raw device pointers (or tensors)"""
        return self._lib.csr5hip_spmv_t(self._h, _ptr(x), _ptr(y))

    def spmmT(self, X, Y) -> int:
        """Y = A^T X for k dense vectors: X (m, k), Y (n, k), otherwise as ``spmm``"""
        return self.spmmT_ptr(*self._spmm_args("spmmT", X, self._m, Y, self._n))

    def spmmT_ptr(self, X, ldx: int, k: int, Y, ldy: int) -> int:
        """csr5hip_spmm_t on raw device pointers (or tensors): X with leading dimension ldx, Y with ldy"""
        return self._lib.csr5hip_spmm_t(self._h, _ptr(X), int(ldx), int(k), _ptr(Y), int(ldy))

    # -- sampled dense-dense product on the pattern (csr5hip.h csr5hip_sddmm) ----------------------
    def sddmm(self, U, V, out) -> int:
        """out[e] = dot(U[row(e), :], V[col(e), :]) for every stored element e, in CSR order -- the order ``updateValues`` takes.
        U (m, k) and V (n, k) as ``spmm``'s operands (stride(1) == 1, leading dimension stride(0)); ``out`` a contiguous 1-D GPU
        tensor of nnz values of the handle's dtype that shares storage with neither U nor V.  The matrix values play no part.
        With U = dY and V = X this is the gradient of ``spmm`` with respect to the stored values.  Anything else raises
        ValueError before the library is called."""
        dt = self._dtype_name()
        for name, t, rows in (("U", U, self._m), ("V", V, self._n)):  # (the checks of _spmm_args; the device comes last)
            if not hasattr(t, "data_ptr") or not hasattr(t, "stride"):
                raise ValueError(f"sddmm: {name} must be a torch tensor")
            if str(t.dtype) != dt:
                raise ValueError(f"sddmm: {name} has dtype {t.dtype}, the handle holds {dt}")
            if t.dim() != 2 or t.shape[0] != rows:
                raise ValueError(f"sddmm: {name} must have shape ({rows}, k), not {tuple(t.shape)}")
            if t.shape[0] > 0 and t.shape[1] > 1 and t.stride(1) != 1:
                raise ValueError(f"sddmm: {name} must be row-major with stride(1) == 1, not {t.stride()}")
            if t.shape[0] > 1 and t.stride(0) < t.shape[1]:
                raise ValueError(f"sddmm: {name} rows overlap (stride(0) {t.stride(0)} < k = {t.shape[1]})")
        if U.shape[1] != V.shape[1]:
            raise ValueError(f"sddmm: U has {U.shape[1]} columns, V {V.shape[1]}")
        k = int(U.shape[1])
        ldu = max(int(U.stride(0)), k) if U.shape[0] > 1 else k
        ldv = max(int(V.stride(0)), k) if V.shape[0] > 1 else k
        if not hasattr(out, "data_ptr") or not hasattr(out, "is_contiguous"):
            raise ValueError("sddmm: out must be a torch tensor")
        if self._nnz is None:
            raise ValueError("sddmm: call inputCSR first")
        if str(out.dtype) != dt:
            raise ValueError(f"sddmm: out has dtype {out.dtype}, the handle holds {dt}")
        if out.dim() != 1 or out.shape[0] != self._nnz:
            raise ValueError(f"sddmm: out must have shape ({self._nnz},), not {tuple(out.shape)}")
        if not out.is_contiguous():
            raise ValueError(f"sddmm: out must be contiguous, not stride {out.stride()}")
        for name, t in (("U", U), ("V", V)):
            if _aliased(out, t):
                raise ValueError(f"sddmm: out shares storage with {name} (aliased)")
        for name, t in (("U", U), ("V", V), ("out", out)):
            if t.device.type != "cuda":
                raise ValueError(f"sddmm: {name} must live on the GPU, not {t.device}")
        if not (U.device == V.device == out.device):
            raise ValueError(f"sddmm: U on {U.device}, V on {V.device}, out on {out.device}")
        return self.sddmm_ptr(U, ldu, V, ldv, k, out)

    def sddmm_ptr(self, U, ldu: int, V, ldv: int, k: int, out) -> int:
        """csr5hip_sddmm on raw device pointers (or tensors): U with leading dimension ldu, V with ldv, out nnz values"""
        return self._lib.csr5hip_sddmm(self._h, _ptr(U), int(ldu), _ptr(V), int(ldv), int(k), _ptr(out))

    # -- max / min aggregation on the pattern (csr5hip_reduce.h csr5hip_spmm_reduce) ----------------
    _REDUCE_OPS = {"max": _capi.REDUCE_MAX, "min": _capi.REDUCE_MIN}

    def _reduce_matrix(self, who: str, name: str, t, rows: int, dt: str, k=None) -> int:
        """the checks of ``_spmm_args`` for one (rows, k) operand of dtype ``dt``, but for the device, which ``_reduce_apart`` judges
        after every operand's shape: its leading dimension, or ValueError"""
        if not hasattr(t, "data_ptr") or not hasattr(t, "stride"):
            raise ValueError(f"{who}: {name} must be a torch tensor")
        if str(t.dtype) != dt:
            raise ValueError(f"{who}: {name} has dtype {t.dtype}, expected {dt}")
        if t.dim() != 2 or t.shape[0] != rows or (k is not None and t.shape[1] != k):
            raise ValueError(f"{who}: {name} must have shape ({rows}, {'k' if k is None else k}), not {tuple(t.shape)}")
        if t.shape[1] > 1 and t.stride(1) != 1:
            raise ValueError(f"{who}: {name} must be row-major with stride(1) == 1, not {t.stride()}")
        if t.shape[0] > 1 and t.stride(0) < t.shape[1]:
            raise ValueError(f"{who}: {name} rows overlap (stride(0) {t.stride(0)} < k = {t.shape[1]})")
        return max(int(t.stride(0)), int(t.shape[1])) if t.shape[0] > 1 else int(t.shape[1])

    @staticmethod
    def _reduce_apart(who: str, outs, ins) -> None:
        """ValueError when an output shares storage with an input or with another output, a tensor does not live on the GPU, or the
        tensors live on several devices"""
        named = [p for p in outs + ins if p[1] is not None]
        for i, (name, t) in enumerate(outs):
            if t is None:
                continue
            for other, u in outs[i + 1:] + ins:
                if u is not None and _aliased(t, u):
                    raise ValueError(f"{who}: {name} shares storage with {other} (aliased)")
        for name, t in named:
            if t.device.type != "cuda":
                raise ValueError(f"{who}: {name} must live on the GPU, not {t.device}")
        if any(t.device != named[0][1].device for _, t in named):
            raise ValueError(f"{who}: " + ", ".join(f"{name} on {t.device}" for name, t in named))

    def spmmReduce(self, X, Y, reduce="max", arg=None, weighted=True) -> int:
        """Y[i, c] = max (``reduce="max"``) or min (``"min"``) over row i's stored entries e of a_e * X[col(e), c] -- of X[col(e), c]
        with ``weighted=False``, which does not read the handle's values -- and arg[i, c] = the winning entry's rank in CSR order
        (csr5hip_reduce.h: NaN first, then the value, then the smaller rank; a row without entries gets +0 and -1).  X (n, k) and
        Y (m, k) as ``spmm``'s operands; ``arg`` an int32 (m, k) tensor with stride(1) == 1, or None.  Every row of Y and arg is
        written.  Wrong dtype, device, shape, stride, ``reduce`` name or an output that shares storage with another operand raise
        ValueError before the library is called."""
        who = "spmmReduce"
        if reduce not in self._REDUCE_OPS:
            raise ValueError(f"{who}: reduce must be 'max' or 'min', not {reduce!r}")
        dt = self._dtype_name()
        ldx = self._reduce_matrix(who, "X", X, self._n, dt)
        k = int(X.shape[1])
        ldy = self._reduce_matrix(who, "Y", Y, self._m, dt, k)
        ldarg = k if arg is None else self._reduce_matrix(who, "arg", arg, self._m, "torch.int32", k)
        self._reduce_apart(who, [("Y", Y), ("arg", arg)], [("X", X)])
        return self.spmm_reduce_ptr(self._REDUCE_OPS[reduce], int(bool(weighted)), X, ldx, k, Y, ldy, arg, ldarg)

    def spmm_reduce_ptr(self, op: int, weighted: int, X, ldx: int, k: int, Y, ldy: int, arg, ldarg: int) -> int:
        """csr5hip_spmm_reduce on raw device pointers (or tensors)"""
        return self._lib.csr5hip_spmm_reduce(self._h, int(op), int(weighted), _ptr(X), int(ldx), int(k), _ptr(Y), int(ldy), _ptr(arg),
                                             int(ldarg))

    def spmmReduceBackward(self, X, dY, arg, dX=None, dVal=None, weighted=True) -> int:
        """The gradients of ``spmmReduce``'s Y from its ``arg`` and dY (m, k): dX (n, k), every row written, by a column kernel on the
        transposed companion (``buildTranspose`` first; no atomics), and -- ``weighted`` only -- dVal, nnz values in CSR order.
        Either may be None and is then not computed.  X is read for dVal only (None is allowed without it).  The checks are
        ``spmmReduce``'s."""
        who = "spmmReduceBackward"
        dt = self._dtype_name()
        lddy = self._reduce_matrix(who, "dY", dY, self._m, dt)
        k = int(dY.shape[1])
        ldarg = self._reduce_matrix(who, "arg", arg, self._m, "torch.int32", k)
        if X is None and dVal is not None:
            raise ValueError(f"{who}: dVal needs X")
        ldx = k if X is None else self._reduce_matrix(who, "X", X, self._n, dt, k)
        lddx = k if dX is None else self._reduce_matrix(who, "dX", dX, self._n, dt, k)
        if dVal is not None:
            if not weighted:
                raise ValueError(f"{who}: dVal exists only with weighted=True")
            self._csr_value_args(who, (("dVal", dVal),))
        self._reduce_apart(who, [("dX", dX), ("dVal", dVal)], [("X", X), ("dY", dY), ("arg", arg)])
        return self.spmm_reduce_backward_ptr(int(bool(weighted)), X, ldx, k, dY, lddy, arg, ldarg, dX, lddx, dVal)

    def spmm_reduce_backward_ptr(self, weighted: int, X, ldx: int, k: int, dY, lddy: int, arg, ldarg: int, dX, lddx: int, dVal) -> int:
        """csr5hip_spmm_reduce_backward on raw device pointers (or tensors)"""
        return self._lib.csr5hip_spmm_reduce_backward(self._h, int(weighted), _ptr(X), int(ldx), int(k), _ptr(dY), int(lddy), _ptr(arg),
                                                      int(ldarg), _ptr(dX), int(lddx), _ptr(dVal))

    # -- attention on the pattern: what the twelve wrappers below share ------
    def _forward_operands(self, Q, K, V, O):
        """(ins, outs) of a forward for ``_operand_args``: (name, tensor, rows, which width) each"""
        return (("Q", Q, self._m, "k"), ("K", K, self._n, "k"), ("V", V, self._n, "d")), (("O", O, self._m, "d"),)

    def _backward_operands(self, Q, K, V, dO, dQ, dK, dV, work, more=()):
        """(ins, outs, others) of a backward: ``outs`` holds the outputs that are wanted (not None), ``more`` (``gatBackward``:
        dAr) among them; ``others`` names everything a per-entry output must not share storage with"""
        ins = (("Q", Q, self._m, "k"), ("K", K, self._n, "k"), ("V", V, self._n, "d"), ("dO", dO, self._m, "d"))
        outs = tuple(o for o in (("dQ", dQ, self._m, "k"), ("dK", dK, self._n, "k"), ("dV", dV, self._n, "d")) + more if o[1] is not None)
        return ins, outs, tuple((name, t) for name, t, _, _ in ins + outs) + (("work", work),)

    def _operand_args(self, who: str, rank: int, ins, outs, work, dt=None, work_dt=None):
        """the checks of the operands, 2-D (rows, width) for ``attention`` or packed 3-D (rows, heads, width) for the others
        (``rank``): ValueError, naming the operand, unless each input and output has the handle's dtype, its row count, a unit
        inner stride, stride(1) == width (3-D) and rows that do not overlap; the head counts and widths agree; ``work`` (wanted
        with dK or dV) holds 4 m heads values; ``inputCSR`` was called; no output shares storage with an input, an earlier output
        or ``work``; all live on one GPU (the device comes last).  ``dt``: the dtype the operands must have instead of the
        handle's (``mhaLowp``: Q's); ``work_dt``: the dtype ``work`` must have instead of the operands' (``mhaLowpBackward``:
        float32).  Returns (heads, k, d, ld): heads is 1 for 2-D operands, ld the leading dimension by name, heads * width for a
        backward's output that is not among ``outs``."""
        holds = "the handle holds" if dt is None else "Q has"
        dt = dt or self._dtype_name()
        packed = rank == 3
        per_head, unit = ("heads, ", "have stride(2) == 1") if packed else ("", "be row-major with stride(1) == 1")
        for name, t, rows, width in ins + outs:
            if not hasattr(t, "data_ptr") or not hasattr(t, "stride"):
                raise ValueError(f"{who}: {name} must be a torch tensor")
            if str(t.dtype) != dt:
                raise ValueError(f"{who}: {name} has dtype {t.dtype}, {holds} {dt}")
            shape, stride = t.shape, t.stride()
            if len(shape) != rank or shape[0] != rows:
                raise ValueError(f"{who}: {name} must have shape ({rows}, {per_head}{width}), not {tuple(shape)}")
            if not t.numel():
                continue  # (a tensor without elements has no strides to judge)
            if shape[-1] > 1 and stride[-1] != 1:
                raise ValueError(f"{who}: {name} must {unit}, not {stride}")
            if packed and shape[1] > 1 and stride[1] != shape[2]:
                raise ValueError(f"{who}: {name} must be packed with stride(1) == {width} = {shape[2]}, not {stride}")
            row = shape[1] * shape[2] if packed else shape[1]
            if shape[0] > 1 and stride[0] < row:
                raise ValueError(f"{who}: {name} rows overlap (stride(0) {stride[0]} < {'heads * ' if packed else ''}{width} = {row})")
        Q, V = ins[0][1], ins[2][1]
        heads, k, d = int(Q.shape[1]) if packed else 1, int(Q.shape[-1]), int(V.shape[-1])
        for name, t, _, width in ins[1:] + outs:
            if packed and t.shape[1] != heads:
                raise ValueError(f"{who}: Q has {heads} heads, {name} {t.shape[1]}")
            first, want = ("Q", k) if width == "k" else ("V", d)
            if t.shape[-1] != want:
                raise ValueError(f"{who}: {first} has width {want}, {name} {t.shape[2]}" if packed else
                                 f"{who}: {first} has {want} columns, {name} {t.shape[1]}")
        if work is not None or any(name in ("dK", "dV") for name, _, _, _ in outs):
            if not hasattr(work, "data_ptr") or not hasattr(work, "is_contiguous"):
                raise ValueError(f"{who}: work must be a torch tensor when dK or dV is wanted")
            if work_dt is not None and str(work.dtype) != work_dt:
                raise ValueError(f"{who}: work has dtype {work.dtype}, it must be {work_dt} whatever the operands' dtype")
            if work_dt is None and str(work.dtype) != dt:
                raise ValueError(f"{who}: work has dtype {work.dtype}, the handle holds {dt}")
            if work.dim() != 1 or work.shape[0] < 4 * self._m * heads:
                raise ValueError(f"{who}: work must have shape ({4 * self._m * heads},) or longer, not {tuple(work.shape)}")
            if not work.is_contiguous():
                raise ValueError(f"{who}: work must be contiguous, not stride {work.stride()}")
        if self._nnz is None:
            raise ValueError(f"{who}: call inputCSR first")
        scratch = (("work", work, 0, ""),) if work is not None else ()
        for i, (oname, o, _, _) in enumerate(outs):
            for name, t, _, _ in ins + outs[:i] + scratch:
                if _aliased(o, t):
                    raise ValueError(f"{who}: {oname} shares storage with {name} (aliased)")
        for name, t, _, _ in ins + outs + scratch:
            if t.device.type != "cuda":
                raise ValueError(f"{who}: {name} must live on the GPU, not {t.device}")
        if any(t.device != Q.device for _, t, _, _ in ins + outs + scratch):
            raise ValueError(f"{who}: " + ", ".join(f"{name} on {t.device}" for name, t, _, _ in ins + outs + scratch))
        ld = dict(dQ=heads * k, dK=heads * k, dV=heads * d, dAr=heads * k)  # (an output that is not wanted)
        for name, t, _, width in ins + outs:
            w = heads * (k if width == "k" else d)
            # (a 2-D operand without columns reports its stride, as it always has; a packed one reports 0)
            ld[name] = max(int(t.stride(0)), w) if t.shape[0] > 1 and (w or not packed) else w
        return heads, k, d, ld

    @staticmethod
    def _mha_heads(Q) -> int:
        """the head count Q announces (judged by ``_operand_args`` afterwards); 0 when Q is no 3-D tensor, which that check rejects"""
        return int(Q.shape[1]) if hasattr(Q, "dim") and hasattr(Q, "shape") and Q.dim() == 3 else 0

    def _mha_entry_tensor(self, who: str, name: str, t, heads: int, dt: str, holds: str, others=()) -> int:
        """the checks of one per-entry tensor (``dS``, ``B``, ``dB``): ValueError unless it is a 2-D tensor of shape (nnz, heads)
        and dtype ``dt`` with stride(1) == 1 and non-overlapping rows that shares storage with none of the tensors among
        ``others`` (its device is the caller's to judge).  Returns its row stride; ``heads`` for None."""
        if t is None:
            return heads
        if not hasattr(t, "data_ptr") or not hasattr(t, "stride"):
            raise ValueError(f"{who}: {name} must be a torch tensor or None")
        if str(t.dtype) != dt:
            raise ValueError(f"{who}: {name} has dtype {t.dtype}, {holds} {dt}")
        if t.dim() != 2 or tuple(t.shape) != (self._nnz, heads):
            raise ValueError(f"{who}: {name} must have shape ({self._nnz}, {heads}), not {tuple(t.shape)}")
        if t.numel() and heads > 1 and t.stride(1) != 1:
            raise ValueError(f"{who}: {name} must have stride(1) == 1, not {t.stride()}")
        if t.numel() and t.shape[0] > 1 and t.stride(0) < heads:
            raise ValueError(f"{who}: {name} rows overlap (stride(0) {t.stride(0)} < heads = {heads})")
        for oname, o in others:  # (judged before the operands: an entry may be None or no tensor at all)
            if hasattr(o, "data_ptr") and _aliased(t, o):
                raise ValueError(f"{who}: {name} shares a storage with {oname} (views of one storage are rejected, disjoint or not)")
        return max(int(t.stride(0)), heads) if t.shape[0] > 1 and heads else heads

    def _small_tensor(self, who: str, name: str, t, rank: int, want, text: str) -> None:
        """the checks of ``slopes`` and ``a``: ValueError unless t is None or a contiguous GPU tensor of the handle's dtype, of
        ``rank`` dimensions and, where ``want`` is known, of that shape (``text`` describes it)"""
        if t is None:
            return
        dt = self._dtype_name()
        if not hasattr(t, "data_ptr") or not hasattr(t, "is_contiguous"):
            raise ValueError(f"{who}: {name} must be a torch tensor or None")
        if str(t.dtype) != dt:
            raise ValueError(f"{who}: {name} has dtype {t.dtype}, the handle holds {dt}")
        if t.dim() != rank or (want is not None and tuple(t.shape) != want):
            raise ValueError(f"{who}: {name} must have shape {text}, not {tuple(t.shape)}")
        if not t.is_contiguous():
            raise ValueError(f"{who}: {name} must be contiguous, not stride {t.stride()}")
        if t.device.type != "cuda":
            raise ValueError(f"{who}: {name} must live on the GPU, not {t.device}")

    def _mha_bias_args(self, who: str, heads: int, scale, slopes, dS, others):
        """the checks of ``scale``, ``slopes`` and ``dS``, made before those of the operands: ValueError unless scale is a finite
        number, slopes (or None) a contiguous 1-D GPU tensor of ``heads`` values of the handle's dtype, dS (or None) an
        (nnz, heads) GPU tensor of that dtype with stride(1) == 1 and non-overlapping rows that shares storage with none of
        ``others``.  Returns (scale, ldds)."""
        if self._nnz is None:
            raise ValueError(f"{who}: call inputCSR first")
        scale = _finite(who, "scale", scale)
        self._small_tensor(who, "slopes", slopes, 1, (heads,), f"({heads},)")
        ldds = self._mha_entry_tensor(who, "dS", dS, heads, self._dtype_name(), "the handle holds", others)
        if dS is not None and dS.device.type != "cuda":
            raise ValueError(f"{who}: dS must live on the GPU, not {dS.device}")
        return scale, ldds

    def _mha_edge_args(self, who: str, heads: int, scale, B, dB, others, dt=None):
        """the checks of ``scale``, ``B`` and ``dB``, made before those of the operands: ValueError unless scale is a finite
        number and B and dB (or None) are 2-D GPU tensors of shape (nnz, heads) and of the handle's dtype with stride(1) == 1 and
        non-overlapping rows; dB shares storage with none of ``others`` nor with B.  ``dt``: the dtype B and dB must have instead
        of the handle's (``mhaLowp``: Q's).  Returns (scale, ldb, lddb): the row strides."""
        holds = "the handle holds" if dt is None else "Q has"
        dt = dt or self._dtype_name()
        if self._nnz is None:
            raise ValueError(f"{who}: call inputCSR first")
        scale = _finite(who, "scale", scale)
        ldb = self._mha_entry_tensor(who, "B", B, heads, dt, holds)
        lddb = self._mha_entry_tensor(who, "dB", dB, heads, dt, holds, others + (("B", B),))
        for name, t in (("B", B), ("dB", dB)):
            if t is not None and t.device.type != "cuda":
                raise ValueError(f"{who}: {name} must live on the GPU, not {t.device}")
        return scale, ldb, lddb

    def _gat_args(self, who: str, Q, a, negative_slope):
        """the checks of ``negative_slope`` and ``a``, made after those of scale, B and dB and before those of the operands:
        ValueError unless negative_slope is a finite number and a (or None) is a contiguous (H, k) GPU tensor of the handle's
        dtype, H and k those Q announces.  Returns the slope as a float."""
        ns = _finite(who, "negative_slope", negative_slope)
        want = (int(Q.shape[1]), int(Q.shape[2])) if hasattr(Q, "dim") and Q.dim() == 3 else None  # (else _operand_args rejects Q)
        self._small_tensor(who, "a", a, 2, want, f"(heads, k) = {want}")
        return ns

    def _after_operands(self, who: str, Q, outs, read, named) -> None:
        """what is left to judge of the tensors beside the operands once ``_operand_args`` has passed: ValueError if an output
        of ``outs`` shares storage with an input of ``read`` (B, a), or a tensor of ``named`` is not on Q's device"""
        for name, t in read:
            if t is not None:
                for oname, o, _, _ in outs:
                    if _aliased(o, t):
                        raise ValueError(f"{who}: {oname} shares storage with {name} (aliased)")
        for name, t in named:
            if t is not None and t.device != Q.device:
                raise ValueError(f"{who}: {name} on {t.device}, Q on {Q.device}")

    _LOWP = {"torch.bfloat16": _capi.BF16, "torch.float16": _capi.F16}

    def _lowp_type(self, who: str, Q):
        """(the operand type of csr5hip_lowp.h, the dtype's name) of a 16-bit Q, or ValueError"""
        ot = self._LOWP.get(str(getattr(Q, "dtype", None)))
        if ot is None:
            raise ValueError(f"{who}: Q must be a torch.bfloat16 or torch.float16 tensor, not {getattr(Q, 'dtype', type(Q).__name__)}")
        return ot, str(Q.dtype)

    # -- attention on the pattern in one pass (csr5hip.h csr5hip_attention) -------------------------
    def attention(self, Q, K, V, O) -> int:
        """O = softmax over every row's stored entries of (Q K^T) times V in ONE launch: row i attends to the columns it stores.
        Q (m, k), K (n, k), V (n, d) and O (m, d) as ``sddmm``'s operands (stride(1) == 1, leading dimension stride(0), so column
        slices of wider tensors are legal: one call per head needs no copy); O shares storage with none of the inputs, which may
        share among themselves.  EVERY row of O is written in columns 0 .. d-1 -- rows without entries with +0 -- so O may be
        ``torch.empty``.  Nothing of length nnz is written and the handle (its values included) is left untouched.  Anything
        else raises ValueError before the library is called."""
        ins, outs = self._forward_operands(Q, K, V, O)
        _, k, d, ld = self._operand_args("attention", 2, ins, outs, None)
        return self.attention_ptr(Q, ld["Q"], K, ld["K"], k, V, ld["V"], d, O, ld["O"])

    def attention_ptr(self, Q, ldq: int, K, ldk: int, k: int, V, ldv: int, d: int, O, ldo: int) -> int:
        """csr5hip_attention on raw device pointers (or tensors): Q, K, V, O with leading dimensions ldq, ldk, ldv, ldo"""
        return self._lib.csr5hip_attention(self._h, _ptr(Q), int(ldq), _ptr(K), int(ldk), int(k), _ptr(V), int(ldv), int(d),
                                           _ptr(O), int(ldo))

    # -- the gradients of attention in two launches (csr5hip.h csr5hip_attention_backward) -----------
    def attentionBackward(self, Q, K, V, dO, dQ=None, dK=None, dV=None, work=None) -> int:
        """The gradients of ``attention``'s O for Q, K and V from the gradient dO (m, d) arriving for O: dQ (m, k), dK (n, k) and
        dV (n, d), each written in EVERY row (rows and columns of the matrix without entries with +0, so they may be
        ``torch.empty``) or None when not wanted.  Operands as ``attention``'s (stride(1) == 1, leading dimension stride(0)); an
        output shares storage with no input, no other output and not with ``work``.  dK and dV need ``work``, a contiguous 1-D
        tensor of at least 4 m values of scratch, and the transposed companion (``buildTranspose``; it is never built here).
        Nothing of length nnz is written and the handle (its values included) is left untouched.  Anything else raises ValueError
        before the library is called."""
        ins, outs, _ = self._backward_operands(Q, K, V, dO, dQ, dK, dV, work)
        _, k, d, ld = self._operand_args("attentionBackward", 2, ins, outs, work)
        return self.attention_backward_ptr(Q, ld["Q"], K, ld["K"], k, V, ld["V"], d, dO, ld["dO"], dQ, ld["dQ"], dK, ld["dK"],
                                           dV, ld["dV"], work)

    def attention_backward_ptr(self, Q, ldq: int, K, ldk: int, k: int, V, ldv: int, d: int, dO, lddo: int, dQ, lddq: int, dK, lddk: int,
                               dV, lddv: int, work) -> int:
        """csr5hip_attention_backward on raw device pointers (or tensors); None for an output that is not wanted"""
        return self._lib.csr5hip_attention_backward(self._h, _ptr(Q), int(ldq), _ptr(K), int(ldk), int(k), _ptr(V), int(ldv), int(d),
                                                    _ptr(dO), int(lddo), _ptr(dQ), int(lddq), _ptr(dK), int(lddk), _ptr(dV), int(lddv),
                                                    _ptr(work))

    # -- attention for all heads in one launch (csr5hip.h csr5hip_mha / csr5hip_mha_backward) -------
    def mha(self, Q, K, V, O) -> int:
        """``attention`` for all heads in ONE launch: Q (m, H, k), K (n, H, k), V (n, H, d) and O (m, H, d), packed (stride(2) == 1,
        stride(1) == width; stride(0) >= H * width, so a slice of a wider tensor is legal).  Head h of O has, bit for bit, what
        ``attention(Q[:, h], K[:, h], V[:, h], O[:, h])`` writes; EVERY row of O is written in all H * d columns, so O may be
        ``torch.empty``; O shares storage with none of the inputs.  The handle is left untouched.  Anything else raises
        ValueError before the library is called."""
        ins, outs = self._forward_operands(Q, K, V, O)
        heads, k, d, ld = self._operand_args("mha", 3, ins, outs, None)
        return self.mha_ptr(heads, Q, ld["Q"], K, ld["K"], k, V, ld["V"], d, O, ld["O"])

    def mha_ptr(self, heads: int, Q, ldq: int, K, ldk: int, k: int, V, ldv: int, d: int, O, ldo: int) -> int:
        """csr5hip_mha on raw device pointers (or tensors): packed Q, K, V, O with leading dimensions ldq, ldk, ldv, ldo"""
        return self._lib.csr5hip_mha(self._h, int(heads), _ptr(Q), int(ldq), _ptr(K), int(ldk), int(k), _ptr(V), int(ldv), int(d),
                                     _ptr(O), int(ldo))

    def mhaBackward(self, Q, K, V, dO, dQ=None, dK=None, dV=None, work=None) -> int:
        """``attentionBackward`` for all heads in TWO launches on ``mha``'s packed operands: dO (m, H, d) in; dQ (m, H, k),
        dK (n, H, k), dV (n, H, d) out, each written in every row and head (so they may be ``torch.empty``) or None when not
        wanted; head h has the bits of ``attentionBackward`` on that head's slices.  dK and dV need ``work``, a contiguous 1-D
        tensor of at least 4 m H values of scratch, and the transposed companion (``buildTranspose``; it is never built here).
        An output shares storage with no input, no other output and not with ``work``.  Anything else raises ValueError before
        the library is called."""
        ins, outs, _ = self._backward_operands(Q, K, V, dO, dQ, dK, dV, work)
        heads, k, d, ld = self._operand_args("mhaBackward", 3, ins, outs, work)
        return self.mha_backward_ptr(heads, Q, ld["Q"], K, ld["K"], k, V, ld["V"], d, dO, ld["dO"], dQ, ld["dQ"], dK, ld["dK"],
                                     dV, ld["dV"], work)

    def mha_backward_ptr(self, heads: int, Q, ldq: int, K, ldk: int, k: int, V, ldv: int, d: int, dO, lddo: int, dQ, lddq: int, dK,
                         lddk: int, dV, lddv: int, work) -> int:
        """csr5hip_mha_backward on raw device pointers (or tensors); None for an output that is not wanted"""
        return self._lib.csr5hip_mha_backward(self._h, int(heads), _ptr(Q), int(ldq), _ptr(K), int(ldk), int(k), _ptr(V), int(ldv),
                                              int(d), _ptr(dO), int(lddo), _ptr(dQ), int(lddq), _ptr(dK), int(lddk), _ptr(dV),
                                              int(lddv), _ptr(work))

    # -- the same with a softmax scale and a score bias from the stored values (csr5hip.h csr5hip_mha_biased) -------
    def mhaBiased(self, Q, K, V, O, scale=1.0, slopes=None) -> int:
        """``mha`` on the scores ``scale * Q K^T + slopes[h] * A``: softmax scale and an additive bias from the handle's STORED
        VALUES (what ``inputCSR`` gave or the last ``updateValues``), one value per stored entry, times a slope per head, in ONE
        launch.  Per entry and head s = fma(qk, scale, slopes[h] * a), every operation rounded once; ``slopes=None`` takes the
        value as it is.  A value of -Inf masks its entry.  Operands as ``mha``; ``scale`` is a finite Python number, ``slopes`` a
        contiguous 1-D tensor of H values of the handle's dtype.  The handle's values are read, never written.  Anything else
        raises ValueError before the library is called."""
        ins, outs = self._forward_operands(Q, K, V, O)
        scale, _ = self._mha_bias_args("mhaBiased", self._mha_heads(Q), scale, slopes, None, ())
        heads, k, d, ld = self._operand_args("mhaBiased", 3, ins, outs, None)
        return self.mha_biased_ptr(heads, scale, slopes, Q, ld["Q"], K, ld["K"], k, V, ld["V"], d, O, ld["O"])

    def mha_biased_ptr(self, heads: int, scale: float, slopes, Q, ldq: int, K, ldk: int, k: int, V, ldv: int, d: int, O, ldo: int) -> int:
        """csr5hip_mha_biased on raw device pointers (or tensors); slopes None for no slopes"""
        return self._lib.csr5hip_mha_biased(self._h, int(heads), float(scale), _ptr(slopes), _ptr(Q), int(ldq), _ptr(K), int(ldk),
                                            int(k), _ptr(V), int(ldv), int(d), _ptr(O), int(ldo))

    def mhaBiasedBackward(self, Q, K, V, dO, dQ=None, dK=None, dV=None, work=None, scale=1.0, slopes=None, dS=None) -> int:
        """the gradients of ``mhaBiased`` in TWO launches: operands, outputs and ``work`` as ``mhaBackward``, ``scale`` and
        ``slopes`` as in the forward.  ``dS`` (optional): an (nnz, H) tensor with stride(1) == 1 that receives, per stored entry
        in CSR order and head, the gradient for the biased score (before scale and slope); the gradient of the values is then
        ``(dS * slopes).sum(1)`` and that of the slopes ``(dS * val[:, None]).sum(0)``.  dK and dV need ``work`` and the
        transposed companion, dS and dQ neither.  The handle's values are read, never written.  Anything else raises ValueError
        before the library is called."""
        ins, outs, others = self._backward_operands(Q, K, V, dO, dQ, dK, dV, work)
        scale, ldds = self._mha_bias_args("mhaBiasedBackward", self._mha_heads(Q), scale, slopes, dS, others)
        heads, k, d, ld = self._operand_args("mhaBiasedBackward", 3, ins, outs, work)
        return self.mha_biased_backward_ptr(heads, scale, slopes, Q, ld["Q"], K, ld["K"], k, V, ld["V"], d, dO, ld["dO"], dQ, ld["dQ"],
                                            dK, ld["dK"], dV, ld["dV"], work, dS, ldds)

    def mha_biased_backward_ptr(self, heads: int, scale: float, slopes, Q, ldq: int, K, ldk: int, k: int, V, ldv: int, d: int, dO,
                                lddo: int, dQ, lddq: int, dK, lddk: int, dV, lddv: int, work, dS, ldds: int) -> int:
        """csr5hip_mha_biased_backward on raw device pointers (or tensors); None for an output that is not wanted"""
        return self._lib.csr5hip_mha_biased_backward(self._h, int(heads), float(scale), _ptr(slopes), _ptr(Q), int(ldq), _ptr(K),
                                                     int(ldk), int(k), _ptr(V), int(ldv), int(d), _ptr(dO), int(lddo), _ptr(dQ),
                                                     int(lddq), _ptr(dK), int(lddk), _ptr(dV), int(lddv), _ptr(work), _ptr(dS),
                                                     int(ldds))

    # -- the same with a per-head bias from a caller-owned (nnz, H) tensor (csr5hip_edge_bias.h csr5hip_mha_edge_bias) -------
    def mhaEdgeBias(self, Q, K, V, O, B=None, scale=1.0) -> int:
        """``mha`` on the scores ``scale * Q K^T + B``: softmax scale and an additive bias that differs per stored entry AND per
        head, from the caller's tensor ``B`` of shape (nnz, H) in CSR order (the order ``sddmm`` writes and ``updateValues``
        takes), in ONE launch.  Per entry and head s = fma(qk, scale, B[e, h]), one rounding.  B has the handle's dtype and
        stride(1) == 1; its row stride is free (a slice of a wider tensor is legal: the columns beyond H are never read).
        ``B=None`` is no bias.  A bias of -Inf masks its entry in that head.  Operands as ``mha``.  THE HANDLE'S VALUES ARE NOT
        READ and nothing of the handle changes.  Anything else raises ValueError before the library is called."""
        ins, outs = self._forward_operands(Q, K, V, O)
        scale, ldb, _ = self._mha_edge_args("mhaEdgeBias", self._mha_heads(Q), scale, B, None, ())
        heads, k, d, ld = self._operand_args("mhaEdgeBias", 3, ins, outs, None)
        self._after_operands("mhaEdgeBias", Q, outs, (("B", B),), (("B", B),))
        return self.mha_edge_bias_ptr(heads, scale, B, ldb, Q, ld["Q"], K, ld["K"], k, V, ld["V"], d, O, ld["O"])

    def mha_edge_bias_ptr(self, heads: int, scale: float, B, ldb: int, Q, ldq: int, K, ldk: int, k: int, V, ldv: int, d: int, O,
                          ldo: int) -> int:
        """csr5hip_mha_edge_bias on raw device pointers (or tensors); B None for no bias"""
        return self._lib.csr5hip_mha_edge_bias(self._h, int(heads), float(scale), _ptr(B), int(ldb), _ptr(Q), int(ldq), _ptr(K),
                                               int(ldk), int(k), _ptr(V), int(ldv), int(d), _ptr(O), int(ldo))

    def mhaEdgeBiasBackward(self, Q, K, V, dO, dQ=None, dK=None, dV=None, work=None, B=None, scale=1.0, dB=None) -> int:
        """the gradients of ``mhaEdgeBias`` in TWO launches: operands, outputs and ``work`` as ``mhaBackward``, ``B`` and ``scale``
        as in the forward.  ``dB`` (optional): an (nnz, H) tensor with stride(1) == 1 that receives THE GRADIENT OF B, entry by
        entry and head by head; no reduction is needed, and columns beyond H of a wider tensor it is a slice of stay untouched.
        dK and dV need ``work`` and the transposed companion, dB and dQ neither.  The handle's values, the companion's included,
        are not read.  Anything else raises ValueError before the library is called."""
        who = "mhaEdgeBiasBackward"
        ins, outs, others = self._backward_operands(Q, K, V, dO, dQ, dK, dV, work)
        scale, ldb, lddb = self._mha_edge_args(who, self._mha_heads(Q), scale, B, dB, others)
        heads, k, d, ld = self._operand_args(who, 3, ins, outs, work)
        self._after_operands(who, Q, outs, (("B", B),), (("B", B), ("dB", dB)))
        return self.mha_edge_bias_backward_ptr(heads, scale, B, ldb, Q, ld["Q"], K, ld["K"], k, V, ld["V"], d, dO, ld["dO"], dQ, ld["dQ"],
                                               dK, ld["dK"], dV, ld["dV"], work, dB, lddb)

    def mha_edge_bias_backward_ptr(self, heads: int, scale: float, B, ldb: int, Q, ldq: int, K, ldk: int, k: int, V, ldv: int, d: int,
                                   dO, lddo: int, dQ, lddq: int, dK, lddk: int, dV, lddv: int, work, dB, lddb: int) -> int:
        """csr5hip_mha_edge_bias_backward on raw device pointers (or tensors); None for B or for an output that is not wanted"""
        return self._lib.csr5hip_mha_edge_bias_backward(self._h, int(heads), float(scale), _ptr(B), int(ldb), _ptr(Q), int(ldq),
                                                        _ptr(K), int(ldk), int(k), _ptr(V), int(ldv), int(d), _ptr(dO), int(lddo),
                                                        _ptr(dQ), int(lddq), _ptr(dK), int(lddk), _ptr(dV), int(lddv), _ptr(work),
                                                        _ptr(dB), int(lddb))

    # -- the same with operands stored in bf16 / fp16, computed in fp32 (csr5hip_lowp.h csr5hip_mha_lowp and its backward) -------
    def mhaLowp(self, Q, K, V, O, B=None, scale=1.0) -> int:
        """``mhaEdgeBias`` on operands STORED IN 16 BITS: Q, K, V, O and B (when given) are all ``torch.bfloat16`` or all
        ``torch.float16``, WHATEVER THE HANDLE'S DTYPE -- only its pattern is used, and an fp32 and an fp64 handle give the same
        bits.  Everything is computed in fp32 and O is rounded once where it is stored, so the result is, bit for bit (NaN
        payloads apart), ``mhaEdgeBias(Q.float(), K.float(), V.float(), O32, B.float(), scale)`` on an fp32 handle cast to the
        operand type.  Layouts, strides, devices and aliasing as ``mhaEdgeBias``; ``B=None`` is no bias, a bias of -Inf masks its
        entry in that head; an fp16 O is +-Inf where the fp32 result exceeds 65 504.  ONE launch; the handle is left untouched.
        Anything else raises ValueError before the library is called."""
        ot, dt = self._lowp_type("mhaLowp", Q)
        ins, outs = self._forward_operands(Q, K, V, O)
        scale, ldb, _ = self._mha_edge_args("mhaLowp", self._mha_heads(Q), scale, B, None, (), dt)
        heads, k, d, ld = self._operand_args("mhaLowp", 3, ins, outs, None, dt)
        self._after_operands("mhaLowp", Q, outs, (("B", B),), (("B", B),))
        return self.mha_lowp_ptr(ot, heads, scale, B, ldb, Q, ld["Q"], K, ld["K"], k, V, ld["V"], d, O, ld["O"])

    def mha_lowp_ptr(self, operand_type: int, heads: int, scale: float, B, ldb: int, Q, ldq: int, K, ldk: int, k: int, V, ldv: int,
                     d: int, O, ldo: int) -> int:
        """csr5hip_mha_lowp on raw device pointers (or tensors): operand_type ``_capi.BF16`` or ``_capi.F16``, the leading
        dimensions in elements of that type; B None for no bias"""
        return self._lib.csr5hip_mha_lowp(self._h, int(operand_type), int(heads), float(scale), _ptr(B), int(ldb), _ptr(Q), int(ldq),
                                          _ptr(K), int(ldk), int(k), _ptr(V), int(ldv), int(d), _ptr(O), int(ldo))

    def mhaLowpBackward(self, Q, K, V, dO, dQ=None, dK=None, dV=None, work=None, B=None, scale=1.0, dB=None) -> int:
        """the gradients of ``mhaLowp`` in TWO launches, ``mhaEdgeBiasBackward`` on operands STORED IN 16 BITS: Q, K, V, dO, B
        (when given) and the wanted outputs dQ, dK, dV, dB are all ``torch.bfloat16`` or all ``torch.float16``, WHATEVER THE
        HANDLE'S DTYPE.  Everything is computed in fp32 and each output is rounded once where it is stored, so each is, bit for bit
        (NaN payloads apart), what ``mhaEdgeBiasBackward`` on an fp32 handle writes for the widened operands, cast to the operand
        type.  ``work`` is a contiguous 1-D ``torch.float32`` tensor of at least 4 m H values, whatever the operands' and the
        handle's dtype: it carries the row maxima, 1 / Z and D unrounded from the row kernel to the column kernel.  dK and dV need
        ``work`` and the transposed companion (``buildTranspose``; it is never built here), dB and dQ neither.  Layouts, strides,
        devices and aliasing as ``mhaEdgeBiasBackward``.  The handle's values are not read.  Anything else raises ValueError
        before the library is called."""
        who = "mhaLowpBackward"
        ot, dt = self._lowp_type(who, Q)
        ins, outs, others = self._backward_operands(Q, K, V, dO, dQ, dK, dV, work)
        scale, ldb, lddb = self._mha_edge_args(who, self._mha_heads(Q), scale, B, dB, others, dt)
        heads, k, d, ld = self._operand_args(who, 3, ins, outs, work, dt, "torch.float32")
        self._after_operands(who, Q, outs, (("B", B),), (("B", B), ("dB", dB)))
        return self.mha_lowp_backward_ptr(ot, heads, scale, B, ldb, Q, ld["Q"], K, ld["K"], k, V, ld["V"], d, dO, ld["dO"], dQ, ld["dQ"],
                                          dK, ld["dK"], dV, ld["dV"], work, dB, lddb)

    def mha_lowp_backward_ptr(self, operand_type: int, heads: int, scale: float, B, ldb: int, Q, ldq: int, K, ldk: int, k: int, V,
                              ldv: int, d: int, dO, lddo: int, dQ, lddq: int, dK, lddk: int, dV, lddv: int, work, dB, lddb: int) -> int:
        """csr5hip_mha_lowp_backward on raw device pointers (or tensors): operand_type ``_capi.BF16`` or ``_capi.F16``, the leading
        dimensions in elements of that type, work float; None for B or for an output that is not wanted"""
        return self._lib.csr5hip_mha_lowp_backward(self._h, int(operand_type), int(heads), float(scale), _ptr(B), int(ldb), _ptr(Q),
                                                   int(ldq), _ptr(K), int(ldk), int(k), _ptr(V), int(ldv), int(d), _ptr(dO), int(lddo),
                                                   _ptr(dQ), int(lddq), _ptr(dK), int(lddk), _ptr(dV), int(lddv), _ptr(work), _ptr(dB),
                                                   int(lddb))

    # -- additive (GAT, GATv2) attention: the non-linearity inside the score (csr5hip_gat.h csr5hip_gat and its backward) -------
    def gat(self, Q, K, V, O, a=None, negative_slope=0.2, B=None, scale=1.0) -> int:
        """additive attention in ONE launch: ``mhaEdgeBias`` with the score ``scale * sum_c a[h, c] LeakyReLU(Q[i, h, c] +
        K[j, h, c]) + B[e, h]`` in the dot product's place.  GAT is k = 1 with ``a=None`` (Q = el, K = er: s = LeakyReLU(el[i] +
        er[j])); GATv2 is k = the feature width with ``a`` of shape (H, k), contiguous, of the handle's dtype.  Per channel
        u = q + k, l = u > 0 ? u : negative_slope * u, z = fma(a, l, z) (``a=None``: a = 1), then s = fma(z, scale, B[e, h]), every
        operation rounded once; everything after the score is ``mha``'s.  Operands, ``B`` and ``scale`` as ``mhaEdgeBias``;
        ``negative_slope`` is a finite Python number.  Nothing of length nnz is written; THE HANDLE'S VALUES ARE NOT READ and nothing
        of the handle changes.  Anything else raises ValueError before the library is called."""
        ins, outs = self._forward_operands(Q, K, V, O)
        scale, ldb, _ = self._mha_edge_args("gat", self._mha_heads(Q), scale, B, None, ())
        ns = self._gat_args("gat", Q, a, negative_slope)
        heads, k, d, ld = self._operand_args("gat", 3, ins, outs, None)
        self._after_operands("gat", Q, outs, (("B", B), ("a", a)), (("B", B), ("a", a)))
        return self.gat_ptr(heads, ns, a, scale, B, ldb, Q, ld["Q"], K, ld["K"], k, V, ld["V"], d, O, ld["O"])

    def gat_ptr(self, heads: int, negative_slope: float, a, scale: float, B, ldb: int, Q, ldq: int, K, ldk: int, k: int, V, ldv: int,
                d: int, O, ldo: int) -> int:
        """csr5hip_gat on raw device pointers (or tensors); a None for a = 1, B None for no bias"""
        return self._lib.csr5hip_gat(self._h, int(heads), float(negative_slope), _ptr(a), float(scale), _ptr(B), int(ldb), _ptr(Q),
                                     int(ldq), _ptr(K), int(ldk), int(k), _ptr(V), int(ldv), int(d), _ptr(O), int(ldo))

    def gatBackward(self, Q, K, V, dO, dQ=None, dK=None, dV=None, work=None, a=None, negative_slope=0.2, B=None, scale=1.0, dB=None,
                    dAr=None) -> int:
        """the gradients of ``gat`` in TWO launches: operands, outputs, ``work``, ``B``, ``scale`` and ``dB`` as
        ``mhaEdgeBiasBackward``, ``a`` and ``negative_slope`` as in the forward.  ``dAr`` (optional): an (m, H, k) tensor, judged as
        dQ is, that receives THE ROW'S SHARE of the gradient of ``a``: the gradient of ``a`` is ``dAr.sum(0)``.  dK and dV need
        ``work`` and the transposed companion; dQ, dAr and dB neither.  An output shares storage with no other argument.  The
        handle's values, the companion's included, are not read.  Anything else raises ValueError before the library is called."""
        who = "gatBackward"
        ins, outs, others = self._backward_operands(Q, K, V, dO, dQ, dK, dV, work, (("dAr", dAr, self._m, "k"),))
        scale, ldb, lddb = self._mha_edge_args(who, self._mha_heads(Q), scale, B, dB, others + (("a", a),))
        ns = self._gat_args(who, Q, a, negative_slope)
        heads, k, d, ld = self._operand_args(who, 3, ins, outs, work)
        self._after_operands(who, Q, outs, (("B", B), ("a", a)), (("B", B), ("dB", dB), ("a", a)))
        return self.gat_backward_ptr(heads, ns, a, scale, B, ldb, Q, ld["Q"], K, ld["K"], k, V, ld["V"], d, dO, ld["dO"], dQ, ld["dQ"],
                                     dK, ld["dK"], dV, ld["dV"], work, dB, lddb, dAr, ld["dAr"])

    def gat_backward_ptr(self, heads: int, negative_slope: float, a, scale: float, B, ldb: int, Q, ldq: int, K, ldk: int, k: int, V,
                         ldv: int, d: int, dO, lddo: int, dQ, lddq: int, dK, lddk: int, dV, lddv: int, work, dB, lddb: int, dAr,
                         lddar: int) -> int:
        """csr5hip_gat_backward on raw device pointers (or tensors); None for a, for B or for an output that is not wanted"""
        return self._lib.csr5hip_gat_backward(self._h, int(heads), float(negative_slope), _ptr(a), float(scale), _ptr(B), int(ldb),
                                              _ptr(Q), int(ldq), _ptr(K), int(ldk), int(k), _ptr(V), int(ldv), int(d), _ptr(dO),
                                              int(lddo), _ptr(dQ), int(lddq), _ptr(dK), int(lddk), _ptr(dV), int(lddv), _ptr(work),
                                              _ptr(dB), int(lddb), _ptr(dAr), int(lddar))

    # -- dropout on the attention weights: a seeded mask inside the mha and gat kernels (csr5hip_dropout.h) ----------------------
    @staticmethod
    def _dropout_args(who: str, p, seed, offset, head0):
        """the checks of the mask's arguments, made before everything else of the call: ValueError unless p is a Python number with
        0 <= p < 1, seed and offset are Python ints in [0, 2**64) and head0 is a Python int >= 0 (bools are none of these).
        Returns (p, seed, offset, head0)."""
        if isinstance(p, bool) or not isinstance(p, (int, float)) or not math.isfinite(p) or not 0.0 <= p < 1.0:
            raise ValueError(f"{who}: p must be a Python number with 0 <= p < 1, not {p!r}")
        for name, x in (("seed", seed), ("offset", offset)):
            if isinstance(x, bool) or not isinstance(x, int) or not 0 <= x < 2 ** 64:
                raise ValueError(f"{who}: {name} must be a Python int in [0, 2**64), not {x!r}")
        if isinstance(head0, bool) or not isinstance(head0, int) or not 0 <= head0 < 2 ** 31:
            raise ValueError(f"{who}: head0 must be a Python int in [0, 2**31), not {head0!r}")
        return float(p), seed, offset, head0

    def dropoutMha(self, Q, K, V, O, p, seed, offset=0, head0=0, B=None, scale=1.0) -> int:
        """``mhaEdgeBias`` (``B=None``: no bias) with DROPOUT ON THE ATTENTION WEIGHTS in the same ONE launch: the softmax is over
        all stored entries, a weight is dropped with probability ``p`` (0 <= p < 1) after it, and the kept ones are scaled by
        1 / (1 - p).  The mask is a pure function of (p, seed, offset, entry's CSR rank, head0 + h) -- Philox4x32-10, written out
        in csr5hip_dropout.h and restated by ``dropoutMask`` -- so the same (seed, offset) gives the same bits, and ``offset = step``
        gives a fresh mask per step.  ``seed`` and ``offset`` are Python ints below 2**64; ``head0`` is the absolute head of
        Q[:, 0]: head h of a packed call is the H = 1 call with ``head0 + h`` on that head's slices.  With p = 0 every bit is
        ``mhaEdgeBias``'s.  Operands, ``B`` and ``scale`` as ``mhaEdgeBias``; nothing of length nnz is written and nothing of the
        handle changes.  Anything else raises ValueError before the library is called."""
        who = "dropoutMha"
        p, seed, offset, head0 = self._dropout_args(who, p, seed, offset, head0)
        ins, outs = self._forward_operands(Q, K, V, O)
        scale, ldb, _ = self._mha_edge_args(who, self._mha_heads(Q), scale, B, None, ())
        heads, k, d, ld = self._operand_args(who, 3, ins, outs, None)
        self._after_operands(who, Q, outs, (("B", B),), (("B", B),))
        return self.dropout_mha_ptr(heads, scale, B, ldb, Q, ld["Q"], K, ld["K"], k, V, ld["V"], d, O, ld["O"], p, seed, offset, head0)

    def dropout_mha_ptr(self, heads: int, scale: float, B, ldb: int, Q, ldq: int, K, ldk: int, k: int, V, ldv: int, d: int, O,
                        ldo: int, p: float, seed: int, offset: int, head0: int) -> int:
        """csr5hip_dropout_mha on raw device pointers (or tensors); B None for no bias"""
        return self._lib.csr5hip_dropout_mha(self._h, int(heads), float(scale), _ptr(B), int(ldb), _ptr(Q), int(ldq), _ptr(K),
                                             int(ldk), int(k), _ptr(V), int(ldv), int(d), _ptr(O), int(ldo), float(p), int(seed),
                                             int(offset), int(head0))

    def dropoutMhaBackward(self, Q, K, V, dO, p, seed, offset=0, head0=0, dQ=None, dK=None, dV=None, work=None, B=None, scale=1.0,
                           dB=None) -> int:
        """the gradients of ``dropoutMha`` in TWO launches, for the same (p, seed, offset, head0): both kernels recompute the
        forward's mask.  Operands, outputs, ``work``, ``B``, ``scale`` and ``dB`` as ``mhaEdgeBiasBackward``.  With p = 0 every bit
        is that call's.  Anything else raises ValueError before the library is called."""
        who = "dropoutMhaBackward"
        p, seed, offset, head0 = self._dropout_args(who, p, seed, offset, head0)
        ins, outs, others = self._backward_operands(Q, K, V, dO, dQ, dK, dV, work)
        scale, ldb, lddb = self._mha_edge_args(who, self._mha_heads(Q), scale, B, dB, others)
        heads, k, d, ld = self._operand_args(who, 3, ins, outs, work)
        self._after_operands(who, Q, outs, (("B", B),), (("B", B), ("dB", dB)))
        return self.dropout_mha_backward_ptr(heads, scale, B, ldb, Q, ld["Q"], K, ld["K"], k, V, ld["V"], d, dO, ld["dO"], dQ, ld["dQ"],
                                             dK, ld["dK"], dV, ld["dV"], work, dB, lddb, p, seed, offset, head0)

    def dropout_mha_backward_ptr(self, heads: int, scale: float, B, ldb: int, Q, ldq: int, K, ldk: int, k: int, V, ldv: int, d: int,
                                 dO, lddo: int, dQ, lddq: int, dK, lddk: int, dV, lddv: int, work, dB, lddb: int, p: float, seed: int,
                                 offset: int, head0: int) -> int:
        """csr5hip_dropout_mha_backward on raw device pointers (or tensors); None for B or for an output that is not wanted"""
        return self._lib.csr5hip_dropout_mha_backward(self._h, int(heads), float(scale), _ptr(B), int(ldb), _ptr(Q), int(ldq),
                                                      _ptr(K), int(ldk), int(k), _ptr(V), int(ldv), int(d), _ptr(dO), int(lddo),
                                                      _ptr(dQ), int(lddq), _ptr(dK), int(lddk), _ptr(dV), int(lddv), _ptr(work),
                                                      _ptr(dB), int(lddb), float(p), int(seed), int(offset), int(head0))

    # -- the dropped dot-product calls with operands stored in bf16 / fp16, computed in fp32 (csr5hip_dropout_lowp.h) ------------
    def dropoutMhaLowp(self, Q, K, V, O, p, seed, offset=0, head0=0, B=None, scale=1.0) -> int:
        """``dropoutMha`` on operands STORED IN 16 BITS: Q, K, V, O and B (when given) are all ``torch.bfloat16`` or all
        ``torch.float16``, WHATEVER THE HANDLE'S DTYPE.  Everything is computed in fp32 -- the kept weights' factor is
        ``float(1 / (1 - p))`` -- and O is rounded once where it is stored, so the result is, bit for bit (NaN payloads apart),
        ``dropoutMha`` on an fp32 handle for the widened operands, cast to the operand type.  The mask is ``dropoutMha``'s and
        ``dropoutMask``'s for the same (p, seed, offset, head0); with p = 0 every word is ``mhaLowp``'s.  The mask's arguments are
        judged first, as ``dropoutMha`` judges them; dtypes, layouts, strides, devices and aliasing as ``mhaLowp``.  ONE launch; the
        handle is left untouched.  Anything else raises ValueError before the library is called."""
        who = "dropoutMhaLowp"
        p, seed, offset, head0 = self._dropout_args(who, p, seed, offset, head0)
        ot, dt = self._lowp_type(who, Q)
        ins, outs = self._forward_operands(Q, K, V, O)
        scale, ldb, _ = self._mha_edge_args(who, self._mha_heads(Q), scale, B, None, (), dt)
        heads, k, d, ld = self._operand_args(who, 3, ins, outs, None, dt)
        self._after_operands(who, Q, outs, (("B", B),), (("B", B),))
        return self.dropout_mha_lowp_ptr(ot, heads, scale, B, ldb, Q, ld["Q"], K, ld["K"], k, V, ld["V"], d, O, ld["O"], p, seed, offset,
                                         head0)

    def dropout_mha_lowp_ptr(self, operand_type: int, heads: int, scale: float, B, ldb: int, Q, ldq: int, K, ldk: int, k: int, V,
                             ldv: int, d: int, O, ldo: int, p: float, seed: int, offset: int, head0: int) -> int:
        """csr5hip_dropout_mha_lowp on raw device pointers (or tensors): operand_type ``_capi.BF16`` or ``_capi.F16``, the leading
        dimensions in elements of that type; B None for no bias"""
        return self._lib.csr5hip_dropout_mha_lowp(self._h, int(operand_type), int(heads), float(scale), _ptr(B), int(ldb), _ptr(Q),
                                                  int(ldq), _ptr(K), int(ldk), int(k), _ptr(V), int(ldv), int(d), _ptr(O), int(ldo),
                                                  float(p), int(seed), int(offset), int(head0))

    def dropoutMhaLowpBackward(self, Q, K, V, dO, p, seed, offset=0, head0=0, dQ=None, dK=None, dV=None, work=None, B=None, scale=1.0,
                               dB=None) -> int:
        """the gradients of ``dropoutMhaLowp`` in TWO launches, for the same (p, seed, offset, head0): ``dropoutMhaBackward`` on
        operands STORED IN 16 BITS.  Q, K, V, dO, B (when given) and the wanted outputs dQ, dK, dV, dB are all ``torch.bfloat16`` or
        all ``torch.float16``, WHATEVER THE HANDLE'S DTYPE; ``work`` is a contiguous 1-D ``torch.float32`` tensor of at least
        4 m H values.  Everything is computed in fp32 and each output is rounded once where it is stored: each is, bit for bit (NaN
        payloads apart), what ``dropoutMhaBackward`` on an fp32 handle writes for the widened operands, cast to the operand type,
        and with p = 0 every word is ``mhaLowpBackward``'s.  dK and dV need ``work`` and the transposed companion
        (``buildTranspose``; it is never built here), dB and dQ neither.  Everything else as ``mhaLowpBackward``.  Anything else
        raises ValueError before the library is called."""
        who = "dropoutMhaLowpBackward"
        p, seed, offset, head0 = self._dropout_args(who, p, seed, offset, head0)
        ot, dt = self._lowp_type(who, Q)
        ins, outs, others = self._backward_operands(Q, K, V, dO, dQ, dK, dV, work)
        scale, ldb, lddb = self._mha_edge_args(who, self._mha_heads(Q), scale, B, dB, others, dt)
        heads, k, d, ld = self._operand_args(who, 3, ins, outs, work, dt, "torch.float32")
        self._after_operands(who, Q, outs, (("B", B),), (("B", B), ("dB", dB)))
        return self.dropout_mha_lowp_backward_ptr(ot, heads, scale, B, ldb, Q, ld["Q"], K, ld["K"], k, V, ld["V"], d, dO, ld["dO"], dQ,
                                                  ld["dQ"], dK, ld["dK"], dV, ld["dV"], work, dB, lddb, p, seed, offset, head0)

    def dropout_mha_lowp_backward_ptr(self, operand_type: int, heads: int, scale: float, B, ldb: int, Q, ldq: int, K, ldk: int, k: int,
                                      V, ldv: int, d: int, dO, lddo: int, dQ, lddq: int, dK, lddk: int, dV, lddv: int, work, dB,
                                      lddb: int, p: float, seed: int, offset: int, head0: int) -> int:
        """csr5hip_dropout_mha_lowp_backward on raw device pointers (or tensors): operand_type ``_capi.BF16`` or ``_capi.F16``, the
        leading dimensions in elements of that type, work float; None for B or for an output that is not wanted"""
        return self._lib.csr5hip_dropout_mha_lowp_backward(self._h, int(operand_type), int(heads), float(scale), _ptr(B), int(ldb),
                                                           _ptr(Q), int(ldq), _ptr(K), int(ldk), int(k), _ptr(V), int(ldv), int(d),
                                                           _ptr(dO), int(lddo), _ptr(dQ), int(lddq), _ptr(dK), int(lddk), _ptr(dV),
                                                           int(lddv), _ptr(work), _ptr(dB), int(lddb), float(p), int(seed),
                                                           int(offset), int(head0))

    def dropoutGat(self, Q, K, V, O, p, seed, offset=0, head0=0, a=None, negative_slope=0.2, B=None, scale=1.0) -> int:
        """``gat`` with ``dropoutMha``'s dropout on the attention weights, in ONE launch -- PyG's ``GATConv(dropout=p)`` recipe.  The
        score is ``gat``'s, bit for bit; the mask and everything after the score are ``dropoutMha``'s.  With p = 0 every bit is
        ``gat``'s.  Anything else raises ValueError before the library is called."""
        who = "dropoutGat"
        p, seed, offset, head0 = self._dropout_args(who, p, seed, offset, head0)
        ins, outs = self._forward_operands(Q, K, V, O)
        scale, ldb, _ = self._mha_edge_args(who, self._mha_heads(Q), scale, B, None, ())
        ns = self._gat_args(who, Q, a, negative_slope)
        heads, k, d, ld = self._operand_args(who, 3, ins, outs, None)
        self._after_operands(who, Q, outs, (("B", B), ("a", a)), (("B", B), ("a", a)))
        return self.dropout_gat_ptr(heads, ns, a, scale, B, ldb, Q, ld["Q"], K, ld["K"], k, V, ld["V"], d, O, ld["O"], p, seed, offset,
                                    head0)

    def dropout_gat_ptr(self, heads: int, negative_slope: float, a, scale: float, B, ldb: int, Q, ldq: int, K, ldk: int, k: int, V,
                        ldv: int, d: int, O, ldo: int, p: float, seed: int, offset: int, head0: int) -> int:
        """csr5hip_dropout_gat on raw device pointers (or tensors); a None for a = 1, B None for no bias"""
        return self._lib.csr5hip_dropout_gat(self._h, int(heads), float(negative_slope), _ptr(a), float(scale), _ptr(B), int(ldb),
                                             _ptr(Q), int(ldq), _ptr(K), int(ldk), int(k), _ptr(V), int(ldv), int(d), _ptr(O),
                                             int(ldo), float(p), int(seed), int(offset), int(head0))

    def dropoutGatBackward(self, Q, K, V, dO, p, seed, offset=0, head0=0, dQ=None, dK=None, dV=None, work=None, a=None,
                           negative_slope=0.2, B=None, scale=1.0, dB=None, dAr=None) -> int:
        """the gradients of ``dropoutGat`` in TWO launches, for the same (p, seed, offset, head0).  Operands, outputs, ``work``,
        ``a``, ``negative_slope``, ``B``, ``scale``, ``dB`` and ``dAr`` as ``gatBackward``.  With p = 0 every bit is that call's.
        Anything else raises ValueError before the library is called."""
        who = "dropoutGatBackward"
        p, seed, offset, head0 = self._dropout_args(who, p, seed, offset, head0)
        ins, outs, others = self._backward_operands(Q, K, V, dO, dQ, dK, dV, work, (("dAr", dAr, self._m, "k"),))
        scale, ldb, lddb = self._mha_edge_args(who, self._mha_heads(Q), scale, B, dB, others + (("a", a),))
        ns = self._gat_args(who, Q, a, negative_slope)
        heads, k, d, ld = self._operand_args(who, 3, ins, outs, work)
        self._after_operands(who, Q, outs, (("B", B), ("a", a)), (("B", B), ("dB", dB), ("a", a)))
        return self.dropout_gat_backward_ptr(heads, ns, a, scale, B, ldb, Q, ld["Q"], K, ld["K"], k, V, ld["V"], d, dO, ld["dO"], dQ,
                                             ld["dQ"], dK, ld["dK"], dV, ld["dV"], work, dB, lddb, dAr, ld["dAr"], p, seed, offset, head0)

    def dropout_gat_backward_ptr(self, heads: int, negative_slope: float, a, scale: float, B, ldb: int, Q, ldq: int, K, ldk: int,
                                 k: int, V, ldv: int, d: int, dO, lddo: int, dQ, lddq: int, dK, lddk: int, dV, lddv: int, work, dB,
                                 lddb: int, dAr, lddar: int, p: float, seed: int, offset: int, head0: int) -> int:
        """csr5hip_dropout_gat_backward on raw device pointers (or tensors); None for a, for B or for an output that is not wanted"""
        return self._lib.csr5hip_dropout_gat_backward(self._h, int(heads), float(negative_slope), _ptr(a), float(scale), _ptr(B),
                                                      int(ldb), _ptr(Q), int(ldq), _ptr(K), int(ldk), int(k), _ptr(V), int(ldv), int(d),
                                                      _ptr(dO), int(lddo), _ptr(dQ), int(lddq), _ptr(dK), int(lddk), _ptr(dV),
                                                      int(lddv), _ptr(work), _ptr(dB), int(lddb), _ptr(dAr), int(lddar), float(p),
                                                      int(seed), int(offset), int(head0))

    def dropoutMask(self, mask, p, seed, offset=0, head0=0) -> int:
        """the mask of the dropped calls, for reference implementations and tests: ``mask`` is a 2-D ``torch.uint8`` GPU tensor
        (nnz, H) with stride(1) == 1 (a column slice of a wider one is legal); element (e, h) becomes 1 where head ``head0 + h`` of
        the entry of CSR rank e is KEPT, 0 where it is dropped.  It needs only the pattern's nnz: CSR and CSR5 format alike.  One
        launch on the handle's stream.  Anything else raises ValueError before the library is called."""
        who = "dropoutMask"
        p, seed, offset, head0 = self._dropout_args(who, p, seed, offset, head0)
        if self._nnz is None:
            raise ValueError(f"{who}: call inputCSR first")
        if not hasattr(mask, "data_ptr") or not hasattr(mask, "stride"):
            raise ValueError(f"{who}: mask must be a torch tensor")
        if str(mask.dtype) != "torch.uint8":
            raise ValueError(f"{who}: mask has dtype {mask.dtype}, it must be torch.uint8")
        if mask.dim() != 2 or mask.shape[0] != self._nnz:
            raise ValueError(f"{who}: mask must have shape ({self._nnz}, heads), not {tuple(mask.shape)}")
        heads = int(mask.shape[1])
        if mask.numel() and heads > 1 and mask.stride(1) != 1:
            raise ValueError(f"{who}: mask must have stride(1) == 1, not {mask.stride()}")
        if mask.numel() and mask.shape[0] > 1 and mask.stride(0) < heads:
            raise ValueError(f"{who}: mask rows overlap (stride(0) {mask.stride(0)} < heads = {heads})")
        if mask.device.type != "cuda":
            raise ValueError(f"{who}: mask must live on the GPU, not {mask.device}")
        ldm = max(int(mask.stride(0)), heads) if mask.shape[0] > 1 and heads else heads
        return self.dropout_mask_ptr(heads, p, seed, offset, head0, mask, ldm)

    def dropout_mask_ptr(self, heads: int, p: float, seed: int, offset: int, head0: int, mask, ldm: int) -> int:
        """csr5hip_dropout_mask on a raw device pointer (or tensor): one byte per entry and head at mask[e * ldm + h]"""
        return self._lib.csr5hip_dropout_mask(self._h, int(heads), float(p), int(seed), int(offset), int(head0), _ptr(mask), int(ldm))

    # -- softmax over the stored entries of every row (csr5hip.h csr5hip_row_softmax) -------------
    def _csr_value_args(self, who: str, named) -> None:
        """the checks of sddmm's ``out`` for every (name, tensor) of ``named``, whose last entry is the output: ValueError unless
        each is a contiguous 1-D GPU tensor of nnz values of the handle's dtype, the output shares storage with no input, and
        all live on one device"""
        dt = self._dtype_name()
        for name, t in named:
            if not hasattr(t, "data_ptr") or not hasattr(t, "is_contiguous"):
                raise ValueError(f"{who}: {name} must be a torch tensor")
        if self._nnz is None:
            raise ValueError(f"{who}: call inputCSR first")
        for name, t in named:
            if str(t.dtype) != dt:
                raise ValueError(f"{who}: {name} has dtype {t.dtype}, the handle holds {dt}")
            if t.dim() != 1 or t.shape[0] != self._nnz:
                raise ValueError(f"{who}: {name} must have shape ({self._nnz},), not {tuple(t.shape)}")
            if not t.is_contiguous():
                raise ValueError(f"{who}: {name} must be contiguous, not stride {t.stride()}")
        out_name, out = named[-1]
        for name, t in named[:-1]:
            if _aliased(out, t):
                raise ValueError(f"{who}: {out_name} shares storage with {name} (aliased)")
        for name, t in named:
            if t.device.type != "cuda":
                raise ValueError(f"{who}: {name} must live on the GPU, not {t.device}")
        if any(t.device != out.device for _, t in named):
            raise ValueError(f"{who}: " + ", ".join(f"{name} on {t.device}" for name, t in named))

    def rowSoftmax(self, scores, out) -> int:
        """out[e] = exp(scores[e] - max of the row) / sum over the row, for every stored element, in CSR order -- the order
        ``sddmm`` writes and ``updateValues`` takes.  ``scores`` and ``out`` are contiguous 1-D GPU tensors of nnz values of the
        handle's dtype that share no storage.  Legal in CSR and CSR5 format alike; allocates nothing; non-finite scores behave
        as in ``torch.softmax``.  Anything else raises ValueError before the library is called."""
        self._csr_value_args("rowSoftmax", (("scores", scores), ("out", out)))
        return self.rowSoftmax_ptr(scores, out)

    def rowSoftmax_ptr(self, scores, out) -> int:
        """csr5hip_row_softmax on raw device pointers (or tensors): nnz values each"""
        return self._lib.csr5hip_row_softmax(self._h, _ptr(scores), _ptr(out))

    def rowSoftmaxGrad(self, p, g, out) -> int:
        """out[e] = p[e] * (g[e] - sum over the row of p * g): the gradient of ``rowSoftmax`` for its scores, from its output p and
        the gradient g arriving for p.  Arguments as ``rowSoftmax``; p and g may be the same tensor, ``out`` shares storage with
        neither."""
        self._csr_value_args("rowSoftmaxGrad", (("p", p), ("g", g), ("out", out)))
        return self.rowSoftmaxGrad_ptr(p, g, out)

    def rowSoftmaxGrad_ptr(self, p, g, out) -> int:
        """csr5hip_row_softmax_grad on raw device pointers (or tensors): nnz values each"""
        return self._lib.csr5hip_row_softmax_grad(self._h, _ptr(p), _ptr(g), _ptr(out))

    def updateValues(self, val) -> int:
        """New numerical values under the same pattern, without a new conversion (csr5hip.h csr5hip_update_values): ``val`` is a
        contiguous 1-D GPU tensor of the handle's dtype with nnz elements in CSR order -- the order ``inputCSR``'s value tensor
        had -- and must not share storage with that tensor (the handle keeps it in its own order).  Asynchronous on the
        handle's stream; ``val`` is only read.  Anything else raises ValueError before the library is called."""
        dt = self._dtype_name()
        if not hasattr(val, "data_ptr") or not hasattr(val, "is_contiguous"):
            raise ValueError("updateValues: val must be a torch tensor")
        if self._nnz is None:
            raise ValueError("updateValues: call inputCSR first")
        if str(val.dtype) != dt:
            raise ValueError(f"updateValues: val has dtype {val.dtype}, the handle holds {dt}")
        if val.dim() != 1 or val.shape[0] != self._nnz:
            raise ValueError(f"updateValues: val must have shape ({self._nnz},), not {tuple(val.shape)}")
        if not val.is_contiguous():
            raise ValueError(f"updateValues: val must be contiguous, not stride {val.stride()}")
        mine = self._keep.get("val")
        if hasattr(mine, "data_ptr") and _aliased(val, mine):  # (inputCSR also takes raw pointers, which name no storage)
            raise ValueError("updateValues: val shares storage with the tensor given to inputCSR (aliased)")
        if val.device.type != "cuda":
            raise ValueError(f"updateValues: val must live on the GPU, not {val.device}")
        return self.updateValues_ptr(val)

    def updateValues_ptr(self, val) -> int:
        """csr5hip_update_values on a raw device pointer (or tensor)"""
        self._autograd_key = None  # (autograd.spmm tracks which values the handle holds: these are not the ones it gave)
        return self._lib.csr5hip_update_values(self._h, _ptr(val))

    # -- additions (documented in include/csr5hip.h) ---------------------------------------------
    def spmv_repeat(self, alpha, y, count: int) -> int:
        return self._lib.csr5hip_spmv_repeat(self._h, float(alpha), _ptr(y), int(count))

    def snapshotX(self) -> int:
        """X_SNAPSHOT mode: take the permuted copy of x now, on the handle's stream (csr5hip.h csr5hip_snapshot_x)"""
        return self._lib.csr5hip_snapshot_x(self._h)

    @staticmethod
    def spmv_rotate(handles, ys, count: int) -> int:
        """`count` SpMVs from one hipGraph, the i-th on handles[i % k] into ys[i % k] (cold-cache protocol, csr5hip.h)."""
        k = len(handles)
        hs = (C.c_void_p * k)(*[h._h.value for h in handles])
        yp = (C.c_void_p * k)(*[_ptr(y) for y in ys])
        return handles[0]._lib.csr5hip_spmv_rotate(hs, yp, k, 1.0, int(count))

    def autotuneSigma(self, y):
        """Measured sigma selection: returns (err, sigma, us_per_spmv); leaves the matrix in CSR5."""
        sigma, us = C.c_int(0), C.c_double(0.0)
        err = self._lib.csr5hip_autotune_sigma(self._h, _ptr(y), C.byref(sigma), C.byref(us))
        return err, sigma.value, us.value

    def setStream(self, stream) -> int:
        raw = getattr(stream, "cuda_stream", stream)
        return self._lib.csr5hip_set_stream(self._h, C.c_void_p(int(raw) if raw else None))

    def setOption(self, option: int, value: int) -> int:
        return self._lib.csr5hip_set_option(self._h, int(option), int(value))

    def setSpmvMode(self, mode: int) -> int:
        return self.setOption(_capi.OPT_SPMV_MODE, mode)

    def setXWindow(self, value: int) -> int:
        """0 = off, 1 = auto (default), 2 = force the LDS x-window variant of the fused kernel."""
        return self.setOption(_capi.OPT_X_WINDOW, value)

    def setLdsY(self, value: int) -> int:
        """0 = off, 1 = auto (default), 2 = force the LDS compaction of a tile's y segments."""
        return self.setOption(_capi.OPT_LDS_Y, value)

    def setStreamNT(self, value: int) -> int:
        """0 off, 1 auto (non-temporal column/value loads when the streams exceed the Infinity Cache), 2 force"""
        return self.setOption(_capi.OPT_STREAM_NT, int(value))

    def setColumnSlabs(self, value: int) -> int:
        """0 off, 1 auto (default), 2..64 (power of two) = that many column slabs (kernel-side structure, csr5hip.h)"""
        return self.setOption(_capi.OPT_COLUMN_SLABS, int(value))

    def setSlabShift(self, value: int) -> int:
        return self.setOption(_capi.OPT_SLAB_SHIFT, int(value))

    def setSlabHot(self, value: int) -> int:
        """column slabs: 0 = no LDS hot table, 1 = auto (default), 2 = force (csr5hip.h CSR5HIP_OPT_SLAB_HOT)"""
        return self.setOption(_capi.OPT_SLAB_HOT, int(value))

    def setSlabMemoryMiB(self, value: int) -> int:
        """upper bound (MiB) on the device memory of the column-slab structure, 0 = none: a structure that would not fit
        is not built and spmv() runs the plain kernel (info().slab_fallback == 1)"""
        return self.setOption(_capi.OPT_SLAB_MEMORY_MIB, int(value))

    def setXSnapshot(self, value: int) -> int:
        """hot-table slab kernel: 0 (default) = its permuted copy of x is refreshed by every spmv() (x read live, as the
        reference does); 1 = once per setX() -- the caller promises not to change x's contents in between (what the
        reference CLI does: CSR5_cuda/main.cu:63); csr5hip.h CSR5HIP_OPT_X_SNAPSHOT"""
        return self.setOption(_capi.OPT_X_SNAPSHOT, int(value))

    def setNarrowValues(self, value: int) -> int:
        """fp64 + hot table: 1 = stream the values as fp32 when every one of them is exactly representable (same results bit
        for bit, 4 bytes less per non-zero); 0 (default) = off; csr5hip.h CSR5HIP_OPT_NARROW_VALUES"""
        return self.setOption(_capi.OPT_NARROW_VALUES, int(value))

    def setDeferCarries(self, value: int) -> int:
        """cut rows finished by a second small launch instead of inside the SpMV launch (no short-spill re-reads, no arrival
        atomics): 0 = off, 1 = auto (default), 2 = force; set before asCSR5 (csr5hip.h CSR5HIP_OPT_DEFER_CARRIES)"""
        return self.setOption(_capi.OPT_DEFER_CARRIES, int(value))

    def setFlaggedColumns(self, value: int) -> int:
        """plain kernel at sigma 4..8: stream column words that carry the row-start flag in bit 31 (no descriptor load): 1 = auto
        (default: matrices whose streams exceed the Infinity Cache), 0 = off, 2 = force (csr5hip.h CSR5HIP_OPT_FLAGGED_COLUMNS)"""
        return self.setOption(_capi.OPT_FLAGGED_COLUMNS, int(value))

    def setNarrowColumns(self, value: int) -> int:
        """x-window kernel: 1 = auto (default) stream 16-bit column codes (15 bits of column + the row-start flag) when every tile spans < 32 768 columns, 0 = off
        (csr5hip.h CSR5HIP_OPT_NARROW_COLUMNS)"""
        return self.setOption(_capi.OPT_NARROW_COLUMNS, int(value))

    def setZeroEmptyRows(self, value: int) -> int:
        """1 = spmv() also stores 0 into rows without non-zeros (solver coupling); 0 = reference behaviour"""
        return self.setOption(_capi.OPT_ZERO_EMPTY_ROWS, int(value))

    def info(self) -> _capi.Csr5Info:
        info = _capi.Csr5Info()
        err = self._lib.csr5hip_get_info(self._h, C.byref(info))
        if err:
            raise RuntimeError(f"csr5hip_get_info -> {err}")
        return info

    def timer_start(self) -> int:
        return self._lib.csr5hip_timer_start(self._h)

    def timer_stop(self) -> float:
        ms = C.c_double(0.0)
        err = self._lib.csr5hip_timer_stop(self._h, C.byref(ms))
        if err:
            raise RuntimeError(f"csr5hip_timer_stop -> {err}: {_capi.last_error()}")
        return ms.value

    def _d2h(self, dptr, count: int, dtype) -> np.ndarray:
        out = np.empty(count, dtype=dtype)
        if count:
            err = self._lib.csr5hip_memcpy_d2h(out.ctypes.data, dptr, out.nbytes)
            if err:
                raise RuntimeError(f"csr5hip_memcpy_d2h -> {err}: {_capi.last_error()}")
        return out

    def csr5_arrays(self) -> dict:
        """Host copies of the CSR5 auxiliary arrays (for parity tests)."""
        i = self.info()
        if i.format != _capi.FORMAT_CSR5:
            raise RuntimeError("matrix is not in CSR5 format")
        return dict(
            sigma=i.sigma, bit_y=i.bit_y_offset, bit_ss=i.bit_scansum_offset,
            num_packet=i.num_packet, p=i.p, tail_start=i.tail_partition_start,
            num_offsets=i.num_offsets,
            tile_ptr=self._d2h(i.d_tile_ptr, i.p + 1, np.uint32),
            tile_desc=self._d2h(i.d_tile_desc, i.p * i.omega * i.num_packet, np.uint32),
            offset_ptr=self._d2h(i.d_offset_ptr, i.p + 1, np.int32),
            offset=self._d2h(i.d_offset, i.num_offsets, np.int32),
        )

    def slab_view(self) -> _capi.SlabView:
        """csr5hip_get_slab_view: scalars and borrowed device pointers of the hot slab child (valid until the next conversion or option
        change); raises when the handle has none."""
        view = _capi.SlabView()
        err = self._lib.csr5hip_get_slab_view(self._h, C.byref(view))
        if err:
            raise RuntimeError(f"csr5hip_get_slab_view -> {err}: {_capi.last_error()}")
        return view

    def slab_child_arrays(self) -> dict:
        """Host copies of what the conversion built for the hot slab child (for the structure tests).  Values come as stored: tiles
        0 .. p-2 in lane-major 16-byte pieces, the CSR tail in CSR order; xperm holds the last x that spmv() permuted."""
        v = self.slab_view()
        nnz, S, tiles = self.info().nnz, v.S, v.p - 1
        vt = np.float64 if self._vt == _capi.F64 else np.float32
        return dict(
            S=v.S, capacity=v.capacity, slab_shift=v.slab_shift, slab_bits=v.slab_bits, sigma=v.sigma, T=v.T, p=v.p,
            tail_start=v.tail_start, segments=v.segments, cold_total=v.cold_total, stride=v.stride, min_count=v.min_count,
            values_narrowed=v.values_narrowed,
            slab_off=self._d2h(v.slab_off, S + 1, np.int32),
            tile0=self._d2h(v.hot_tile0, S + 1, np.int32),
            xcd_slabs=self._d2h(v.hot_tile0 + 4 * (S + 1), S, np.int32),
            hot_count=self._d2h(v.hot_count, S, np.int32),
            hot_cols=self._d2h(v.hot_cols, S * v.capacity, np.int32).reshape(S, v.capacity),
            cold_base=self._d2h(v.cold_base, S + 1, np.int32),
            cold_cols=self._d2h(v.cold_cols, v.cold_total, np.int32),
            col_lo=self._d2h(v.col_lo, tiles * v.T, np.uint16),
            col_hi=self._d2h(v.col_hi, tiles * v.T, np.uint8),
            row_ptr=self._d2h(v.row_ptr, v.segments + 1, np.int32),
            col=self._d2h(v.col, nnz, np.int32),
            val=self._d2h(v.val, nnz, vt),
            val32=self._d2h(v.val32, nnz, np.float32) if v.values_narrowed else None,
            tile_ptr=self._d2h(v.tile_ptr, v.p + 1, np.uint32),
            range_begin=self._d2h(v.range_begin, S * 257, np.int32).reshape(S, 257),
            range_cost=self._d2h(v.range_cost, tiles + 1, np.uint64),
            range_head=self._d2h(v.range_head, S * 256 + 1, np.uint32),
            xperm=self._d2h(v.xperm, S * v.capacity + v.cold_total, vt),
        )

    # -- checkpoint -----------------------------------------------
    def save(self, path: str) -> int:
        """Write the CSR5 state (row_ptr, tile-ordered col/val, the four format arrays) to `path`."""
        import os
        return self._lib.csr5hip_save(self._h, os.fsencode(path))

    @classmethod
    def load(cls, path: str):
        """Restore a checkpoint written by :meth:`save` -> handle already in CSR5 format (no conversion).
        The CSR arrays live in ``handle.arrays`` (an ``ingest.DeviceCsr`` owned by the handle object)."""
        import os
        from .ingest import DeviceCsr
        lib = _capi.load()
        h = C.c_void_p()
        raw = _capi.DeviceCsrStruct()
        err = lib.csr5hip_load(os.fsencode(path), C.byref(h), C.byref(raw))
        if err:
            raise RuntimeError(f"csr5hip_load -> {err}: {_capi.last_error()}")
        self = cls.__new__(cls)
        self._lib, self._h, self._vt, self._keep = lib, h, int(raw.value_type), {}
        self._m, self._n, self._nnz = int(raw.m), int(raw.n), int(raw.nnz)
        self.arrays = DeviceCsr(raw)
        return self

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.csr5hip_free(self._h)
            self._h = C.c_void_p()
        self._keep = {}
        arrays = getattr(self, "arrays", None)
        if arrays is not None:  # CSR arrays of a loaded checkpoint: released after the handle that borrowed them
            arrays.release()
            self.arrays = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MultiGpuHandle:
    """One matrix on the G GPUs of a node through the C ABI (``csr5hip_multi_*``, include/csr5hip.h): cost-balanced (nnz + 2 * rows) row
    blocks, one ordinary handle + stream per device, x replicated by ONE RCCL broadcast at ``setX``, y sharded.
    ``devices`` may repeat a device id (several shards on one GPU) -- how a 1-GPU box exercises the path."""

    def __init__(self, devices, m: int, n: int, dtype="float64"):
        self._lib = _capi.load()
        self._h = C.c_void_p()
        self.m, self.n, self.G = int(m), int(n), len(devices)
        self._np_dtype = np.float64 if _value_type(dtype) == _capi.F64 else np.float32
        devs = (C.c_int * self.G)(*[int(d) for d in devices])
        self._check(self._lib.csr5hip_multi_create(C.byref(self._h), devs, self.G, self.m, self.n, _value_type(dtype)),
                    "csr5hip_multi_create")
        self._keep = {}

    def _check(self, rc: int, what: str) -> None:
        if rc != 0:
            raise RuntimeError(f"{what} -> {rc}: {_capi.last_error()}")

    def inputCSR(self, nnz, row_ptr, col, val) -> int:
        """device arrays on devices[0]; copied into the shards (the caller's arrays stay untouched)"""
        return self._lib.csr5hip_multi_input_csr(self._h, int(nnz), _ptr(row_ptr), _ptr(col), _ptr(val))

    def setSigma(self, sigma: int) -> int:
        return self._lib.csr5hip_multi_set_sigma(self._h, int(sigma))

    def setOption(self, option: int, value: int) -> int:
        return self._lib.csr5hip_multi_set_option(self._h, int(option), int(value))

    def setRowWeight(self, weight: int) -> int:
        """cost of a row in non-zeros when the row blocks are cut (default 2; 0 = plain nnz balance); before inputCSR"""
        return self.setOption(_capi.MULTI_OPT_ROW_WEIGHT, int(weight))

    def asCSR5(self) -> int:
        return self._lib.csr5hip_multi_as_csr5(self._h)

    def setX(self, x) -> int:
        self._keep["x"] = x
        return self._lib.csr5hip_multi_set_x(self._h, _ptr(x))

    def updateValues(self, val) -> int:
        """the whole matrix' nnz values in CSR order on devices[0]; every shard takes its slice (csr5hip_multi_update_values).
        Enqueued on the shards' streams: keep ``val`` unchanged until ``synchronize()``."""
        self._keep["val"] = val
        return self._lib.csr5hip_multi_update_values(self._h, _ptr(val))

    def spmv(self, alpha=1.0) -> int:
        return self._lib.csr5hip_multi_spmv(self._h, float(alpha))

    def spmv_repeat(self, alpha, count: int) -> int:
        return self._lib.csr5hip_multi_spmv_repeat(self._h, float(alpha), int(count))

    def synchronize(self) -> int:
        return self._lib.csr5hip_multi_synchronize(self._h)

    def timer_start(self) -> int:
        return self._lib.csr5hip_multi_timer_start(self._h)

    def timer_stop(self) -> float:
        ms = C.c_double(0.0)
        self._check(self._lib.csr5hip_multi_timer_stop(self._h, C.byref(ms)), "csr5hip_multi_timer_stop")
        return ms.value

    def shard(self, g: int) -> _capi.Shard:
        s = _capi.Shard()
        self._check(self._lib.csr5hip_multi_shard(self._h, int(g), C.byref(s)), "csr5hip_multi_shard")
        return s

    def shard_info(self, g: int) -> _capi.Csr5Info:
        info = _capi.Csr5Info()
        self._check(self._lib.csr5hip_get_info(C.c_void_p(self.shard(g).handle), C.byref(info)), "csr5hip_get_info")
        return info

    def fill_y(self, byte_value: int) -> int:
        return self._lib.csr5hip_multi_fill_y(self._h, int(byte_value))

    def gather_y(self) -> np.ndarray:
        out = np.empty(self.m, dtype=self._np_dtype)
        self._check(self._lib.csr5hip_multi_gather_y(self._h, out.ctypes.data), "csr5hip_multi_gather_y")
        return out

    def destroy(self) -> int:
        return self._lib.csr5hip_multi_destroy(self._h)

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.csr5hip_multi_free(self._h)
            self._h = C.c_void_p()
        self._keep = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
