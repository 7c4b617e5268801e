"""A converted handle as a differentiable sparse operator: ``Y = spmm(A, val, X)`` with gradients for ``val`` and ``X``.

``A`` is an ``anonymouslibHandle`` in CSR5 format, ``val`` its nnz values in CSR order (the order ``inputCSR``'s value tensor
had) and ``X`` an (n, k) tensor; fp64 and fp32.  The three legs are the library's own kernels:

* forward          ``A.updateValues(val)`` unless the handle already holds exactly these values, then ``A.spmm(X, Y)`` into
                   ``torch.zeros`` (rows without entries, which the kernel leaves untouched, are 0)
* grad of ``val``  ``A.sddmm(dY, X)``: for every stored entry (i, j) the dot product of dY[i, :] and X[j, :]
* grad of ``X``    ``A.spmmT(dY, .)`` into ``torch.zeros``; ``A.buildTranspose()`` is called (once per conversion: it allocates and
                   synchronises) only when X needs a gradient and the handle has no transposed companion yet

Which values the handle holds is tracked on the handle object by (storage pointer, data pointer, ``_version``) of the tensor last
given to it; the tensor is kept referenced so that its address cannot be reused by another one.  A write that does not move
``_version`` (through ``.data``) is therefore not seen: give such values as a new tensor.  Backward gives the handle the
forward's values again when another forward has replaced them in between, so that A^T holds them (only where X needs a
gradient: ``sddmm`` does not read the values).

Aliasing (inherited from ``updateValues``): ``val`` must not share storage with the tensor given to ``inputCSR`` -- the handle
keeps that one in its own order; ``updateValues`` raises ValueError.

Stream: every call runs on torch's current stream of X's device (``setStream`` before each call); the wrapper itself never
synchronises.  Importing this module needs no GPU.
"""
from __future__ import annotations

import torch

from . import _capi

__all__ = ["spmm"]


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError(f"{what} -> {rc}: {_capi.last_error()}")


def _key(val):
    return (val.untyped_storage().data_ptr(), val.data_ptr(), val._version)


def _on_current_stream(A, device) -> None:
    _check(A.setStream(torch.cuda.current_stream(device)), "setStream")


def _give_values(A, val, key) -> None:
    """updateValues(val) unless the handle holds exactly these values"""
    if getattr(A, "_autograd_key", None) == key:
        return  # (the tensor behind the key is still referenced below, so the key cannot name another one)
    _check(A.updateValues(val), "updateValues")
    A._autograd_key, A._autograd_val = key, val


def _rows_unit_stride(t):
    """what spmm / sddmm take: stride(1) == 1 and non-overlapping rows; anything else is made contiguous"""
    if t.dim() == 2 and (t.shape[1] <= 1 or t.stride(1) == 1) and (t.shape[0] <= 1 or t.stride(0) >= t.shape[1]):
        return t
    return t.contiguous()


class _Spmm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, A, val, X):
        val = val.detach()
        if not val.is_contiguous():
            val = val.contiguous()
        Xc = _rows_unit_stride(X.detach())
        _on_current_stream(A, Xc.device)
        key = _key(val)
        _give_values(A, val, key)
        Y = torch.zeros((A._m, Xc.shape[1]), dtype=Xc.dtype, device=Xc.device)
        _check(A.spmm(Xc, Y), "spmm")
        ctx.A, ctx.key = A, key
        ctx.save_for_backward(val, Xc)
        return Y

    @staticmethod
    def backward(ctx, dY):
        A = ctx.A
        val, X = ctx.saved_tensors
        need_val, need_X = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        dY = dY.contiguous()
        _on_current_stream(A, dY.device)
        grad_val = grad_X = None
        if need_val:
            grad_val = torch.empty(val.shape[0], dtype=val.dtype, device=dY.device)
            _check(A.sddmm(dY, X, grad_val), "sddmm")
        if need_X:
            _give_values(A, val, ctx.key)  # (another forward may have given the handle other values: A^T must hold the forward's)
            if not A.info().transpose_built:
                _check(A.buildTranspose(), "buildTranspose")
            grad_X = torch.zeros((A._n, dY.shape[1]), dtype=dY.dtype, device=dY.device)
            _check(A.spmmT(dY, grad_X), "spmmT")
        return None, grad_val, grad_X


def spmm(A, val, X):
    """Y = A X (m, k) with the values ``val`` (nnz, CSR order) on the pattern of the converted handle ``A``; differentiable in
    ``val`` and ``X`` (see the module docstring)."""
    return _Spmm.apply(A, val, X)
