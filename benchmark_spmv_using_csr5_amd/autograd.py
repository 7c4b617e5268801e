"""A converted handle as a differentiable sparse operator: ``Y = spmm(A, val, X)`` with gradients for ``val`` and ``X``, the
two other links of attention on the pattern -- ``sddmm(A, U, V)`` and ``row_softmax(A, scores)`` -- and their composition
``attention(A, Q, K, V)``.

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

``row_softmax(A, scores)`` is ``A.rowSoftmax`` forward (the output p is saved) and ``A.rowSoftmaxGrad(p, g)`` backward; it reads
the handle's row_ptr only.  ``sddmm(A, U, V)`` is ``A.sddmm`` forward; backward hands the handle the incoming gradient G as its
values and takes ``grad_U = A.spmm(V)`` and ``grad_V = A.spmmT(U)``, each into ``torch.zeros`` and only where needed (the
transposed companion is built only when V needs a gradient).  After any of these calls the handle HOLDS WHATEVER VALUES THE LAST
CALL GAVE IT -- ``spmm``'s val, or a gradient G from ``sddmm``'s backward; ``spmm``'s backward gives the forward's values again
where it needs them (above), so interleaved forwards and backwards on one handle stay correct.

``fused_attention(A, Q, K, V)`` is the same function as ``attention`` with a one-launch forward: ``A.attention`` into
``torch.empty``, nothing of length nnz allocated, only Q, K and V saved, the handle's values and the record of them untouched
(the forward of inference, under ``torch.no_grad()``, where the values in the handle belong to somebody else).  Its default
backward recomputes through ``attention`` and therefore DOES leave the handle as that function's backward does (below);
``backward="fused"`` is one ``A.attentionBackward`` call instead, which leaves the handle untouched as the forward does.

``multihead_attention(A, Q, K, V)`` is ``fused_attention(..., backward="fused")`` for H heads at once on packed operands
(rows, H, width): one ``A.mha`` forward, one ``A.mhaBackward`` backward, the handle untouched by both.  With ``scale``, ``bias``
or ``slopes`` it computes ``softmax(scale Q K^T + slopes[h] bias)`` through ``A.mhaBiased`` / ``A.mhaBiasedBackward``: the bias is
nnz values in CSR order and is given to the handle as ``spmm``'s ``val`` is, so the handle then holds it.  A 2-D ``bias`` of
shape (nnz, H) -- a learned edge bias that differs per head -- takes ``A.mhaEdgeBias`` / ``A.mhaEdgeBiasBackward`` instead: the
bias stays the caller's tensor, the handle is given no values and nothing about it is recorded or checked.  With bf16 or fp16
Q, K, V (and such a 2-D bias) the forward is one ``A.mhaLowp`` -- 16-bit operands, fp32 arithmetic, whatever the handle's dtype --
and the backward on an fp32 handle is one ``A.mhaLowpBackward`` on the kept 16-bit tensors (no widened copy, no cast); on an fp64
handle it still widens what was kept and goes through ``A.mhaEdgeBiasBackward`` (a stopgap, see ``multihead_attention``).
``dropout_attention`` with bf16 or fp16 tensors is one ``A.dropoutMhaLowp`` forward and one ``A.dropoutMhaLowpBackward`` backward on
either handle dtype.

``spmm_reduce(A, val, X, reduce="max")`` is the max / min aggregator: ``A.spmmReduce`` forward (Y and the int32 argmax, one
launch), ``A.spmmReduceBackward`` backward (``dval`` by a row kernel, ``dX`` by a column kernel on the transposed companion, built
only when X needs a gradient).  With ``val`` the handle is given the values as ``spmm`` gives them; ``val=None`` aggregates
X[col(e), :] itself and neither reads nor touches the handle's values or the record of them.

Stream: every call runs on torch's current stream of X's device (``setStream`` before each call); the wrapper itself never
synchronises.  Importing this module needs no GPU.
"""
from __future__ import annotations

import torch

from . import _capi
from .handle import anonymouslibHandle

__all__ = ["spmm", "spmm_reduce", "sddmm", "row_softmax", "attention", "fused_attention", "multihead_attention", "gat_attention", "dropout_attention",
           "gat_dropout_attention"]


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError(f"{what} -> {rc}: {_capi.last_error()}")


def _key(val):
    return (val.untyped_storage().data_ptr(), val.data_ptr(), val._version)


def _on_current_stream(A, device) -> None:
    _check(A.setStream(torch.cuda.current_stream(device)), "setStream")


def _with_transpose(A) -> None:
    """the transposed companion, built (once per conversion: it allocates and synchronises) unless the handle has it"""
    if not A.info().transpose_built:
        _check(A.buildTranspose(), "buildTranspose")


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
            _with_transpose(A)
            grad_X = torch.zeros((A._n, dY.shape[1]), dtype=dY.dtype, device=dY.device)
            _check(A.spmmT(dY, grad_X), "spmmT")
        return None, grad_val, grad_X


def spmm(A, val, X):
    """Y = A X (m, k) with the values ``val`` (nnz, CSR order) on the pattern of the converted handle ``A``; differentiable in
    ``val`` and ``X`` (see the module docstring)."""
    return _Spmm.apply(A, val, X)


class _SpmmReduce(torch.autograd.Function):
    @staticmethod
    def forward(ctx, A, val, X, reduce):
        weighted = val is not None
        Xc = _rows_unit_stride(X.detach())
        _on_current_stream(A, Xc.device)
        key = None
        if weighted:
            val = val.detach()
            if not val.is_contiguous():
                val = val.contiguous()
            key = _key(val)
            _give_values(A, val, key)
        Y = torch.empty((A._m, Xc.shape[1]), dtype=Xc.dtype, device=Xc.device)  # (the kernel writes every row)
        arg = torch.empty((A._m, Xc.shape[1]), dtype=torch.int32, device=Xc.device)
        _check(A.spmmReduce(Xc, Y, reduce, arg, weighted), "spmmReduce")
        ctx.A, ctx.key, ctx.weighted = A, key, weighted
        ctx.save_for_backward(arg, Xc, *((val,) if weighted else ()))
        ctx.mark_non_differentiable(arg)
        return Y, arg

    @staticmethod
    def backward(ctx, dY, _darg):
        A, weighted = ctx.A, ctx.weighted
        arg, X = ctx.saved_tensors[:2]
        need_val, need_X = weighted and ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        grad_val = grad_X = None
        if not (need_val or need_X):
            return None, None, None, None
        dY = dY.contiguous()
        _on_current_stream(A, dY.device)
        if need_val:
            grad_val = torch.empty(A._nnz, dtype=dY.dtype, device=dY.device)
        if need_X:
            if weighted:  # (another forward may have given the handle other values: A^T must hold the forward's)
                _give_values(A, ctx.saved_tensors[2], ctx.key)
            _with_transpose(A)
            grad_X = torch.empty((A._n, dY.shape[1]), dtype=dY.dtype, device=dY.device)  # (the kernel writes every row)
        _check(A.spmmReduceBackward(X, dY, arg, grad_X, grad_val, weighted), "spmmReduceBackward")
        return None, grad_val, grad_X, None


def spmm_reduce(A, val, X, reduce="max", return_arg=False):
    """Y[i, c] = max (or, ``reduce="min"``, min) over row i's stored entries e of val[e] * X[col(e), c] on the pattern of the converted
    handle ``A``; differentiable in ``val`` (nnz, CSR order) and ``X`` (n, k).  ``val=None`` is the unweighted aggregation of
    X[col(e), c]: the handle's values are neither touched nor read, and nothing about them is recorded.  With ``val`` the handle is
    given the values as ``spmm`` gives them.  One launch forward (``A.spmmReduce`` into ``torch.empty``; a row without entries is 0);
    the int32 argmax (m, k) and X are kept.  Backward is ``A.spmmReduceBackward``: the gradient flows to the winning entry alone (ties
    go to the smaller rank); the transposed companion is built (once per conversion) only when X needs a gradient.
    ``return_arg=True`` returns (Y, arg)."""
    Y, arg = _SpmmReduce.apply(A, val, X, reduce)
    return (Y, arg) if return_arg else Y


class _Sddmm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, A, U, V):
        Uc, Vc = _rows_unit_stride(U.detach()), _rows_unit_stride(V.detach())
        _on_current_stream(A, Uc.device)
        out = torch.empty(A._nnz, dtype=Uc.dtype, device=Uc.device)
        _check(A.sddmm(Uc, Vc, out), "sddmm")
        ctx.A = A
        ctx.save_for_backward(Uc, Vc)
        return out

    @staticmethod
    def backward(ctx, G):
        A = ctx.A
        U, V = ctx.saved_tensors
        need_U, need_V = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        grad_U = grad_V = None
        if not (need_U or need_V):
            return None, None, None
        G = G.detach().contiguous()
        _on_current_stream(A, G.device)
        _give_values(A, G, _key(G))  # (the handle now holds G: see the module docstring)
        if need_U:  # dU[i, :] = sum_j G[i, j] V[j, :]
            grad_U = torch.zeros((A._m, V.shape[1]), dtype=G.dtype, device=G.device)
            _check(A.spmm(V, grad_U), "spmm")
        if need_V:  # dV[j, :] = sum_i G[i, j] U[i, :]
            _with_transpose(A)
            grad_V = torch.zeros((A._n, U.shape[1]), dtype=G.dtype, device=G.device)
            _check(A.spmmT(U, grad_V), "spmmT")
        return None, grad_U, grad_V


class _RowSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, A, scores):
        s = scores.detach().contiguous()
        _on_current_stream(A, s.device)
        p = torch.empty_like(s)
        _check(A.rowSoftmax(s, p), "rowSoftmax")
        ctx.A = A
        ctx.save_for_backward(p)
        return p

    @staticmethod
    def backward(ctx, g):
        A = ctx.A
        (p,) = ctx.saved_tensors
        if not ctx.needs_input_grad[1]:
            return None, None
        g = g.detach().contiguous()
        _on_current_stream(A, g.device)
        out = torch.empty_like(p)
        _check(A.rowSoftmaxGrad(p, g, out), "rowSoftmaxGrad")
        return None, out


def sddmm(A, U, V):
    """out[e] = dot(U[row(e), :], V[col(e), :]) for every stored element of the converted handle ``A`` (nnz values, CSR order);
    differentiable in ``U`` (m, k) and ``V`` (n, k) (see the module docstring)."""
    return _Sddmm.apply(A, U, V)


def row_softmax(A, scores):
    """softmax of ``scores`` (nnz, CSR order) over the stored entries of every row of the handle ``A``; differentiable in
    ``scores``."""
    return _RowSoftmax.apply(A, scores)


def attention(A, Q, K, V):
    """sparse attention on the pattern of the converted handle ``A``: row i attends to the columns j it stores, with weights
    softmax_j(Q[i, :] . K[j, :]).  Q (m, k), K (n, k), V (n, d); differentiable in all three.  Any scaling (1 / sqrt(k)) is
    applied by the caller to Q."""
    return spmm(A, row_softmax(A, sddmm(A, Q, K)), V)


class _FusedAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, A, Q, K, V, fused_backward=False):
        Qc, Kc, Vc = (_rows_unit_stride(t.detach()) for t in (Q, K, V))
        _on_current_stream(A, Qc.device)
        O = torch.empty((A._m, Vc.shape[1]), dtype=Vc.dtype, device=Vc.device)  # (the kernel writes every row)
        _check(A.attention(Qc, Kc, Vc, O), "attention")
        ctx.A, ctx.fused_backward = A, fused_backward
        ctx.save_for_backward(Qc, Kc, Vc)
        return O

    @staticmethod
    def backward(ctx, dO):
        need = ctx.needs_input_grad[1:4]
        if not any(need):
            return None, None, None, None, None
        if ctx.fused_backward:
            return (None,) + _fused_backward(ctx.A, ctx.saved_tensors, need, dO) + (None,)
        with torch.enable_grad():
            ops = [t.detach().requires_grad_(True) if n else t for t, n in zip(ctx.saved_tensors, need)]
            out = attention(ctx.A, *ops)
            grads = iter(torch.autograd.grad(out, [t for t, n in zip(ops, need) if n], dO))
        return (None,) + tuple(next(grads) if n else None for n in need) + (None,)


def _fused_backward(A, saved, need, dO):
    """(dQ, dK, dV), None where not needed, by ONE ``A.attentionBackward`` on the current stream"""
    Q, K, V = saved
    dO, outs, work = _backward_plumbing(A, saved, need, dO, None, dO.dtype)
    _check(A.attentionBackward(Q, K, V, dO, outs[0], outs[1], outs[2], work), "attentionBackward")
    return tuple(outs)


def fused_attention(A, Q, K, V, backward="recompute"):
    """``attention(A, Q, K, V)`` -- the same function, the same gradients -- with the forward in ONE launch (``A.attention``): no
    scores, no weights, nothing of length nnz is allocated or written, and only Q, K and V are kept for backward.  The forward
    neither reads nor changes the handle's values and does not touch the record of them, so under ``torch.no_grad()`` the
    handle is exactly what it was.  The output agrees with ``attention``'s to rounding, not bit for bit (the normalisation
    comes after the product, and the product is summed row-wise).

    ``backward="recompute"`` (the default) recomputes the weights through the existing pieces: ``attention`` on detached copies
    of exactly those operands that need a gradient, then ``torch.autograd.grad`` with the incoming gradient, so the three
    gradients are bit for bit those of ``attention`` for the same inputs.  The rules of that function therefore apply AFTER A
    BACKWARD: the handle holds whatever values the last call gave it (the recomputed weights, or a gradient from ``sddmm``'s
    backward), and the transposed companion is built (once per conversion: it allocates and synchronises) only when K or V
    needs a gradient.

    ``backward="fused"`` is ONE ``A.attentionBackward`` call (two launches) on the current stream: ``torch.empty`` outputs for
    exactly the inputs that need a gradient, a workspace of 4 m values and the transposed companion only when K or V needs one,
    nothing of length nnz, and the handle's values and the record of them untouched -- a handle whose values belong to somebody
    else can be trained through.  Its gradients agree with the other route's to rounding, not bit for bit.

    Nothing runs in backward when no input needs a gradient."""
    if backward not in ("recompute", "fused"):
        raise ValueError(f"fused_attention: backward must be 'recompute' or 'fused', not {backward!r}")
    return _FusedAttention.apply(A, Q, K, V, backward == "fused")


def _packed(t):
    """what mha takes: (rows, heads, width) with stride(2) == 1, stride(1) == width and non-overlapping rows; anything else is
    made contiguous"""
    if (t.dim() == 3 and (t.shape[2] <= 1 or t.stride(2) == 1) and (t.shape[1] <= 1 or t.stride(1) == t.shape[2])
            and (t.shape[0] <= 1 or t.stride(0) >= t.shape[1] * t.shape[2])):
        return t
    return t.contiguous()


def _backward_plumbing(A, saved, need, dO, heads, work_dtype):
    """what every backward that is one library call does first, in this order: dO made what the call takes (``heads`` None: the
    2-D call), the handle put on the current stream, a ``torch.empty`` output for exactly those of ``saved`` (Q, K, V) that
    ``need`` a gradient, and -- only when K or V needs one -- the transposed companion (``_with_transpose``) and a
    workspace of 4 m heads values of ``work_dtype``.  Returns (dO, [dQ, dK, dV] with None where not needed, work or None)."""
    dO = _backward_dO(A, dO, heads)
    return (dO,) + _backward_buffers(A, saved, need, dO.device, heads, work_dtype)


def _backward_dO(A, dO, heads):
    """the first half of ``_backward_plumbing``: dO as the call takes it, the handle on the current stream"""
    dO = (_rows_unit_stride if heads is None else _packed)(dO.detach())
    _on_current_stream(A, dO.device)
    return dO


def _backward_buffers(A, saved, need, device, heads, work_dtype):
    """the second half: the outputs, the companion and the workspace.  On their own for ``_BiasedMultiheadAttention``, which gives
    the handle its values between the two: after the stream is set, before anything is allocated"""
    outs = [torch.empty_like(t, memory_format=torch.contiguous_format) if n else None for t, n in zip(saved, need)]
    work = None
    if need[1] or need[2]:
        _with_transpose(A)
        work = torch.empty(4 * A._m * (heads or 1), dtype=work_dtype, device=device)
    return outs, work


class _MultiheadAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, A, Q, K, V):
        Qc, Kc, Vc = (_packed(t.detach()) for t in (Q, K, V))
        _on_current_stream(A, Qc.device)
        O = torch.empty((A._m,) + tuple(Vc.shape[1:]), dtype=Vc.dtype, device=Vc.device)  # (the kernel writes every row and head)
        _check(A.mha(Qc, Kc, Vc, O), "mha")
        ctx.A = A
        ctx.save_for_backward(Qc, Kc, Vc)
        return O

    @staticmethod
    def backward(ctx, dO):
        need = ctx.needs_input_grad[1:4]
        if not any(need):
            return None, None, None, None
        A, saved = ctx.A, ctx.saved_tensors
        dO, outs, work = _backward_plumbing(A, saved, need, dO, saved[0].shape[1], dO.dtype)
        _check(A.mhaBackward(saved[0], saved[1], saved[2], dO, outs[0], outs[1], outs[2], work), "mhaBackward")
        return (None,) + tuple(outs)


class _BiasedMultiheadAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, A, Q, K, V, scale, bias, slopes):
        Qc, Kc, Vc = (_packed(t.detach()) for t in (Q, K, V))
        _on_current_stream(A, Qc.device)
        val = key = None
        if bias is not None:
            val = bias.detach()
            if not val.is_contiguous():
                val = val.contiguous()
            key = _key(val)
            _give_values(A, val, key)  # (the handle now holds the bias: see the module docstring)
        else:
            key = getattr(A, "_autograd_key", None)  # (bias=None: the record of the values the handle holds now, checked in backward)
        sl = slopes.detach().contiguous() if slopes is not None else None
        O = torch.empty((A._m,) + tuple(Vc.shape[1:]), dtype=Vc.dtype, device=Vc.device)  # (the kernel writes every row and head)
        _check(A.mhaBiased(Qc, Kc, Vc, O, scale=scale, slopes=sl), "mhaBiased")
        ctx.A, ctx.scale, ctx.key = A, scale, key
        ctx.save_for_backward(Qc, Kc, Vc, val, sl)
        return O

    @staticmethod
    def backward(ctx, dO):
        need = ctx.needs_input_grad[1:4]
        Q, K, V, val, sl = ctx.saved_tensors
        need_bias = val is not None and ctx.needs_input_grad[5]
        need_slopes = sl is not None and ctx.needs_input_grad[6]
        if not (any(need) or need_bias or need_slopes):
            return (None,) * 7
        A = ctx.A
        dO = _backward_dO(A, dO, Q.shape[1])
        if val is not None:
            _give_values(A, val, ctx.key)  # (another forward may have given the handle other values: both kernels read the forward's)
        elif getattr(A, "_autograd_key", None) != ctx.key:
            raise RuntimeError("multihead_attention: the handle's values were replaced between this forward (bias=None: whatever the "
                               "handle held) and its backward; give the bias as a tensor, which backward hands to the handle again")
        outs, work = _backward_buffers(A, (Q, K, V), need, dO.device, Q.shape[1], dO.dtype)
        dS = torch.empty((A._nnz, Q.shape[1]), dtype=dO.dtype, device=dO.device) if need_bias or need_slopes else None
        _check(A.mhaBiasedBackward(Q, K, V, dO, outs[0], outs[1], outs[2], work, scale=ctx.scale, slopes=sl, dS=dS), "mhaBiasedBackward")
        grad_bias = grad_slopes = None
        if need_bias:
            grad_bias = (dS * sl).sum(1) if sl is not None else dS.sum(1)
        if need_slopes:
            grad_slopes = (dS * val[:, None]).sum(0)
        return (None,) + tuple(outs) + (None, grad_bias, grad_slopes)


def _rows_packed(t):
    """what mhaEdgeBias takes for B: (nnz, H) with stride(1) == 1 and non-overlapping rows; anything else is made contiguous"""
    if (t.shape[1] <= 1 or t.stride(1) == 1) and (t.shape[0] <= 1 or t.stride(0) >= t.shape[1]):
        return t
    return t.contiguous()


class _EdgeBiasMultiheadAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, A, Q, K, V, scale, bias):
        Qc, Kc, Vc = (_packed(t.detach()) for t in (Q, K, V))
        Bc = _rows_packed(bias.detach())
        _on_current_stream(A, Qc.device)
        O = torch.empty((A._m,) + tuple(Vc.shape[1:]), dtype=Vc.dtype, device=Vc.device)  # (the kernel writes every row and head)
        _check(A.mhaEdgeBias(Qc, Kc, Vc, O, B=Bc, scale=scale), "mhaEdgeBias")
        ctx.A, ctx.scale = A, scale
        ctx.save_for_backward(Qc, Kc, Vc, Bc)
        return O

    @staticmethod
    def backward(ctx, dO):
        need = ctx.needs_input_grad[1:4]
        need_bias = ctx.needs_input_grad[5]
        if not (any(need) or need_bias):
            return (None,) * 6
        A = ctx.A
        Q, K, V, B = ctx.saved_tensors
        dO, outs, work = _backward_plumbing(A, (Q, K, V), need, dO, Q.shape[1], dO.dtype)
        dB = torch.empty(tuple(B.shape), dtype=dO.dtype, device=dO.device) if need_bias else None  # (every element is written)
        _check(A.mhaEdgeBiasBackward(Q, K, V, dO, outs[0], outs[1], outs[2], work, B=B, scale=ctx.scale, dB=dB), "mhaEdgeBiasBackward")
        return (None,) + tuple(outs) + (None, dB)  # (dB IS the gradient of the bias: no reduction)


class _LowpMultiheadAttention(torch.autograd.Function):
    """bf16 / fp16 operands: the forward is ONE ``A.mhaLowp``.  On an fp32 handle the backward is ONE ``A.mhaLowpBackward`` on the
    kept 16-bit tensors and on dO as it arrives: 16-bit outputs for exactly the inputs that need a gradient, a float32 workspace
    only when K or V needs one, dB the bias gradient itself.  On an fp64 handle the backward stays the STOPGAP it was: the saved
    operands and dO are widened to fp64, ``A.mhaEdgeBiasBackward`` computes the gradients there, and each wanted one is cast to
    its input's dtype (moving it to the fp32 kernel would change gradient bits)."""

    @staticmethod
    def forward(ctx, A, Q, K, V, scale, bias):
        Qc, Kc, Vc = (_packed(t.detach()) for t in (Q, K, V))
        Bc = _rows_packed(bias.detach()) if bias is not None else None
        _on_current_stream(A, Qc.device)
        O = torch.empty((A._m,) + tuple(Vc.shape[1:]), dtype=Vc.dtype, device=Vc.device)  # (the kernel writes every row and head)
        _check(A.mhaLowp(Qc, Kc, Vc, O, B=Bc, scale=scale), "mhaLowp")
        ctx.A, ctx.scale, ctx.has_bias = A, scale, Bc is not None
        ctx.save_for_backward(*((Qc, Kc, Vc, Bc) if Bc is not None else (Qc, Kc, Vc)))
        return O

    @staticmethod
    def backward(ctx, dO):
        need = ctx.needs_input_grad[1:4]
        need_bias = ctx.has_bias and ctx.needs_input_grad[5]
        if not (any(need) or need_bias):
            return (None,) * 6
        A = ctx.A
        Q, K, V = ctx.saved_tensors[:3]
        B = ctx.saved_tensors[3] if ctx.has_bias else None
        low, stopgap = Q.dtype, A._vt == _capi.F64
        if stopgap:  # (a widened temporary each: what the fp32 handle's route does not make)
            Q, K, V = (t.to(torch.float64) for t in (Q, K, V))
            B = B.to(torch.float64) if B is not None else None
            dO = _packed(dO.detach()).to(torch.float64)
        dO, outs, work = _backward_plumbing(A, (Q, K, V), need, dO, Q.shape[1], torch.float64 if stopgap else torch.float32)
        dB = torch.empty(tuple(B.shape), dtype=B.dtype, device=dO.device) if need_bias else None  # (every element is written)
        if not stopgap:
            _check(A.mhaLowpBackward(Q, K, V, dO, outs[0], outs[1], outs[2], work, B=B, scale=ctx.scale, dB=dB), "mhaLowpBackward")
            return (None,) + tuple(outs) + (None, dB)  # (dB IS the gradient of the bias: no reduction, no cast)
        _check(A.mhaEdgeBiasBackward(Q, K, V, dO, outs[0], outs[1], outs[2], work, B=B, scale=ctx.scale, dB=dB), "mhaEdgeBiasBackward")
        return (None,) + tuple(o.to(low) if o is not None else None for o in outs) + (None, dB.to(low) if dB is not None else None)


def multihead_attention(A, Q, K, V, scale=None, bias=None, slopes=None):
    """``fused_attention`` for H heads in one call on packed operands: Q (m, H, k), K (n, H, k), V (n, H, d) -> (m, H, d); head h
    is, bit for bit, ``fused_attention(A, Q[:, h], K[:, h], V[:, h], backward="fused")``, in the output and in every gradient.
    Forward is ONE ``A.mha`` (one launch) into ``torch.empty``; only Q, K and V are kept.  Backward is ONE ``A.mhaBackward``
    (two launches) on the current stream: ``torch.empty`` outputs for exactly the inputs that need a gradient, a workspace of
    4 m H values and the transposed companion (``buildTranspose``, once per conversion: it allocates and synchronises) only
    when K or V needs one.  Nothing of length nnz is allocated, and the handle's values and the record of them are untouched:
    under ``torch.no_grad()`` the handle is exactly what it was.  There is no recompute route here; ``fused_attention`` keeps
    it for one head.  Nothing runs in backward when no input needs a gradient.

    With any of ``scale``, ``bias`` and ``slopes`` given (all three ``None`` is the code path above, unchanged) the weights are
    ``softmax(scale * Q K^T + slopes[h] * bias)`` over the stored entries, by ONE ``A.mhaBiased`` forward and ONE
    ``A.mhaBiasedBackward`` backward:

    * ``scale``   a Python float, ``None`` for 1.0; not differentiable.
    * ``bias``    nnz values in CSR order (edge features, a distance bias, a mask of 0 / -Inf), handed to the handle as
                  ``spmm``'s ``val`` is: ``A.updateValues`` unless the handle already holds exactly this tensor, so AFTER THE
                  CALL THE HANDLE HOLDS THE BIAS, and ``updateValues``'s aliasing rule applies.  Differentiable.  ``None``: whatever
                  values the handle holds are the bias, and nothing flows back to them.  THEY MUST STILL BE THERE IN BACKWARD:
                  nothing is kept to give again.  Where another call of this module has replaced them in between, backward
                  raises RuntimeError (the record of the handle's values differs); a direct ``A.updateValues`` between forward
                  and backward of values that this module never gave is NOT seen, and backward then differentiates the
                  function of the new values.
    * ``slopes``  H values, one per head (ALiBi), ``None`` for none; differentiable, which needs ``bias`` as a tensor (the
                  gradient is formed from it) -- ValueError otherwise.

    Backward gives the handle the forward's bias again when another forward has replaced it in between.  Only when ``bias`` or
    ``slopes`` needs a gradient an (nnz, H) tensor of score gradients dS is allocated and written; ``grad_bias`` is
    ``(dS * slopes).sum(1)`` and ``grad_slopes`` ``(dS * bias[:, None]).sum(0)``, in torch.  Single-head users pass H = 1 on a
    ``(rows, 1, width)`` view.

    A 2-D ``bias`` of shape (nnz, H), entry e in CSR order and head h at ``bias[e, h]``, is a PER-HEAD edge bias (a graph
    transformer's ``Linear(edge_attr)``): the weights are ``softmax(scale * Q K^T + bias[:, h])`` by ONE ``A.mhaEdgeBias``
    forward and ONE ``A.mhaEdgeBiasBackward`` backward.  The bias stays the caller's tensor: THE HANDLE IS GIVEN NO VALUES, its
    values are not read, and nothing about it is recorded in forward or checked in backward, so none of the caveats above
    applies.  ``grad_bias`` IS the (nnz, H) tensor dB the backward kernel writes -- allocated only when the bias needs a
    gradient, no torch reduction applied.  ``slopes`` together with a 2-D bias raises ValueError: fold them into the bias
    (``bias * slopes``).  A 1-D bias and ``bias=None`` are the code paths above, unchanged.  (Scale-only attention that does not
    read the handle's values is ``A.mhaEdgeBias(B=None)``; this function has no keyword for it.)

    A ``torch.bfloat16`` or ``torch.float16`` Q takes the 16-BIT ROUTE, whatever the handle's dtype: K, V and ``bias`` (``None`` or
    2-D (nnz, H)) have Q's dtype, forward is ONE ``A.mhaLowp`` -- fp32 arithmetic, O rounded once, the handle's values not read --
    and Q, K, V and the bias are kept.  A 1-D bias or ``slopes`` raises ValueError there: those live in the handle's values, which
    have another type.  BACKWARD ON AN fp32 HANDLE is ONE ``A.mhaLowpBackward`` (two launches) on the kept 16-bit tensors and on the
    incoming gradient as it arrives: ``torch.empty`` 16-bit outputs for exactly the inputs that need a gradient, a float32
    workspace of 4 m H values and the transposed companion only when K or V needs one, ``grad_bias`` the dB the kernel writes; no
    widened copy and no cast.  Each gradient is the fp32 route's on the widened operands rounded once, and the recomputed scores
    are the forward's bits.  ON AN fp64 HANDLE THE BACKWARD IS STILL A STOPGAP: the kept tensors and the incoming gradient are
    widened to fp64, ONE ``A.mhaEdgeBiasBackward`` runs on them, and each wanted gradient is cast to its input's dtype.  There is
    no ``torch.autocast`` integration."""
    if getattr(Q, "dtype", None) in (torch.bfloat16, torch.float16):
        if slopes is not None or (bias is not None and not (hasattr(bias, "dim") and bias.dim() == 2)):
            raise ValueError("multihead_attention: with bf16 / fp16 operands the bias is None or a 2-D (nnz, H) tensor of their dtype; a "
                             "1-D bias and slopes live in the handle's values, which have another type")
        return _LowpMultiheadAttention.apply(A, Q, K, V, 1.0 if scale is None else float(scale), bias)
    if bias is not None and hasattr(bias, "dim") and bias.dim() == 2:
        if slopes is not None:
            raise ValueError("multihead_attention: slopes cannot be combined with a 2-D (nnz, H) bias: fold them into the bias")
        return _EdgeBiasMultiheadAttention.apply(A, Q, K, V, 1.0 if scale is None else float(scale), bias)
    if scale is None and bias is None and slopes is None:
        return _MultiheadAttention.apply(A, Q, K, V)
    if slopes is not None and bias is None and slopes.requires_grad and torch.is_grad_enabled():
        raise ValueError("multihead_attention: slopes needs a gradient, which is formed from the bias: give bias as a tensor")
    return _BiasedMultiheadAttention.apply(A, Q, K, V, 1.0 if scale is None else float(scale), bias, slopes)


class _GatAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, A, Q, K, V, att, negative_slope, scale, bias):
        Qc, Kc, Vc = (_packed(t.detach()) for t in (Q, K, V))
        ac = att.detach().contiguous() if att is not None else None
        Bc = _rows_packed(bias.detach()) if bias is not None else None
        _on_current_stream(A, Qc.device)
        O = torch.empty((A._m,) + tuple(Vc.shape[1:]), dtype=Vc.dtype, device=Vc.device)  # (the kernel writes every row and head)
        _check(A.gat(Qc, Kc, Vc, O, a=ac, negative_slope=negative_slope, B=Bc, scale=scale), "gat")
        ctx.A, ctx.ns, ctx.scale = A, negative_slope, scale
        ctx.save_for_backward(Qc, Kc, Vc, ac, Bc)
        return O

    @staticmethod
    def backward(ctx, dO):
        Q, K, V, a, B = ctx.saved_tensors
        need = ctx.needs_input_grad[1:4]
        need_att = a is not None and ctx.needs_input_grad[4]
        need_bias = B is not None and ctx.needs_input_grad[7]
        if not (any(need) or need_att or need_bias):
            return (None,) * 8
        A = ctx.A
        dO, outs, work = _backward_plumbing(A, (Q, K, V), need, dO, Q.shape[1], dO.dtype)
        dB = torch.empty(tuple(B.shape), dtype=dO.dtype, device=dO.device) if need_bias else None  # (every element is written)
        dAr = torch.empty_like(Q, memory_format=torch.contiguous_format) if need_att else None  # (every row and head is written)
        _check(A.gatBackward(Q, K, V, dO, outs[0], outs[1], outs[2], work, a=a, negative_slope=ctx.ns, B=B, scale=ctx.scale, dB=dB,
                             dAr=dAr), "gatBackward")
        grad_att = dAr.sum(0) if need_att else None  # (the kernels write the rows' shares: the reduction over the rows is torch's)
        return (None,) + tuple(outs) + (grad_att, None, None, dB)


def gat_attention(A, Q, K, V, att=None, negative_slope=0.2, scale=None, bias=None):
    """additive attention on the pattern, differentiable: packed Q (m, H, k), K (n, H, k), V (n, H, d) -> (m, H, d) with the weights
    ``softmax(scale * sum_c att[h, c] LeakyReLU(Q[i, h, c] + K[j, h, c]) + bias[e, h])`` over the stored entries of row i.

    * GAT:   k = 1, ``att=None``, Q = el, K = er (the two halves of the attention vector applied to the features): the score is
             ``LeakyReLU(el[i, h] + er[j, h])``.
    * GATv2: k = the feature width, Q = W_l x, K = W_r x, ``att`` the (H, k) attention vector; ``K`` and ``V`` may be the same
             tensor (autograd adds their two gradients).

    ``negative_slope`` is the LeakyReLU's, ``scale`` a Python float (``None`` for 1.0), neither differentiable; ``bias`` ``None`` or
    a 2-D (nnz, H) tensor in CSR order as ``multihead_attention``'s per-head edge bias, differentiable.  The non-linearity sits
    INSIDE the score, so no choice of Q, K and bias turns ``multihead_attention`` into this.

    Forward is ONE ``A.gat`` (one launch) into ``torch.empty`` on torch's current stream; Q, K, V, att and bias are kept.  Backward
    is ONE ``A.gatBackward`` (two launches): ``torch.empty`` outputs for exactly what needs a gradient, a workspace of 4 m H
    values and the transposed companion (``buildTranspose``, once per conversion) only when K or V needs one.  ``grad_att`` is
    ``dAr.sum(0)`` of the (m, H, k) per-row shares the row kernel writes, allocated only when ``att`` needs a gradient;
    ``grad_bias`` IS the dB the kernel writes, allocated only when the bias needs one.  Otherwise nothing of length nnz is
    allocated; the handle is given no values and its values are not read.  Nothing runs in backward when nothing needs a
    gradient.  fp32 and fp64 handles; there is no 16-bit route."""
    if bias is not None and not (hasattr(bias, "dim") and bias.dim() == 2):
        raise ValueError("gat_attention: bias is None or a 2-D (nnz, H) tensor in CSR order")
    return _GatAttention.apply(A, Q, K, V, att, float(negative_slope), 1.0 if scale is None else float(scale), bias)


def _dropout_numbers(who, p, seed, offset):
    """(p, seed, offset) as the dropped calls take them: the handle's own check (``_dropout_args``), made before anything runs"""
    return anonymouslibHandle._dropout_args(who, p, seed, offset, 0)[:3]


class _DropoutAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, A, Q, K, V, scale, bias, p, seed, offset):
        Qc, Kc, Vc = (_packed(t.detach()) for t in (Q, K, V))
        Bc = _rows_packed(bias.detach()) if bias is not None else None
        _on_current_stream(A, Qc.device)
        O = torch.empty((A._m,) + tuple(Vc.shape[1:]), dtype=Vc.dtype, device=Vc.device)  # (the kernel writes every row and head)
        _check(A.dropoutMha(Qc, Kc, Vc, O, p, seed, offset, B=Bc, scale=scale), "dropoutMha")
        ctx.A, ctx.scale, ctx.drop = A, scale, (p, seed, offset)
        ctx.save_for_backward(Qc, Kc, Vc, Bc)
        return O

    @staticmethod
    def backward(ctx, dO):
        Q, K, V, B = ctx.saved_tensors
        need = ctx.needs_input_grad[1:4]
        need_bias = B is not None and ctx.needs_input_grad[5]
        if not (any(need) or need_bias):
            return (None,) * 9
        A = ctx.A
        dO, outs, work = _backward_plumbing(A, (Q, K, V), need, dO, Q.shape[1], dO.dtype)
        dB = torch.empty(tuple(B.shape), dtype=dO.dtype, device=dO.device) if need_bias else None  # (every element is written)
        p, seed, offset = ctx.drop
        _check(A.dropoutMhaBackward(Q, K, V, dO, p, seed, offset, dQ=outs[0], dK=outs[1], dV=outs[2], work=work, B=B, scale=ctx.scale,
                                    dB=dB), "dropoutMhaBackward")
        return (None,) + tuple(outs) + (None, dB, None, None, None)


class _LowpDropoutAttention(torch.autograd.Function):
    """bf16 / fp16 operands: the forward is ONE ``A.dropoutMhaLowp``, the backward ONE ``A.dropoutMhaLowpBackward`` on the kept
    16-bit tensors and on dO as it arrives, with the same (p, seed, offset): 16-bit outputs for exactly the inputs that need a
    gradient, a float32 workspace only when K or V needs one, dB the bias gradient itself.  On fp32 and fp64 handles alike: the
    handle's values are not read, and this route has no earlier bit pattern to keep."""

    @staticmethod
    def forward(ctx, A, Q, K, V, scale, bias, p, seed, offset):
        Qc, Kc, Vc = (_packed(t.detach()) for t in (Q, K, V))
        Bc = _rows_packed(bias.detach()) if bias is not None else None
        _on_current_stream(A, Qc.device)
        O = torch.empty((A._m,) + tuple(Vc.shape[1:]), dtype=Vc.dtype, device=Vc.device)  # (the kernel writes every row and head)
        _check(A.dropoutMhaLowp(Qc, Kc, Vc, O, p, seed, offset, B=Bc, scale=scale), "dropoutMhaLowp")
        ctx.A, ctx.scale, ctx.drop = A, scale, (p, seed, offset)
        ctx.save_for_backward(Qc, Kc, Vc, Bc)
        return O

    @staticmethod
    def backward(ctx, dO):
        Q, K, V, B = ctx.saved_tensors
        need = ctx.needs_input_grad[1:4]
        need_bias = B is not None and ctx.needs_input_grad[5]
        if not (any(need) or need_bias):
            return (None,) * 9
        A = ctx.A
        dO, outs, work = _backward_plumbing(A, (Q, K, V), need, dO, Q.shape[1], torch.float32)
        dB = torch.empty(tuple(B.shape), dtype=B.dtype, device=dO.device) if need_bias else None  # (every element is written)
        p, seed, offset = ctx.drop
        _check(A.dropoutMhaLowpBackward(Q, K, V, dO, p, seed, offset, dQ=outs[0], dK=outs[1], dV=outs[2], work=work, B=B,
                                        scale=ctx.scale, dB=dB), "dropoutMhaLowpBackward")
        return (None,) + tuple(outs) + (None, dB, None, None, None)  # (dB IS the gradient of the bias: no reduction, no cast)


def dropout_attention(A, Q, K, V, p, seed, offset=0, scale=None, bias=None, training=True):
    """``multihead_attention`` with DROPOUT ON THE ATTENTION WEIGHTS inside the fused kernels: packed Q (m, H, k), K (n, H, k),
    V (n, H, d) -> (m, H, d), the weights ``softmax(scale * Q K^T + bias[:, h])`` over the stored entries of row i, each dropped
    with probability ``p`` AFTER the softmax and the kept ones scaled by 1 / (1 - p) -- ``TransformerConv(dropout=p)``'s placement.
    ``bias`` is ``None`` or a 2-D (nnz, H) tensor in CSR order, differentiable; ``scale`` a Python float (``None`` for 1.0).

    The mask is a pure function of (p, seed, offset, entry, head) -- Philox4x32-10, written out in csr5hip_dropout.h; it makes no
    claim to match torch's generator -- so a fixed (seed, offset) makes the function deterministic, and ``A.dropoutMask``
    reproduces it.  ``seed`` and ``offset`` are Python ints below 2**64.  DRAWING FRESH ONES PER STEP IS THE CALLER'S BUSINESS; the
    idiom is one seed per layer and run and ``offset = step``::

        out = dropout_attention(A, Q, K, V, 0.6, seed=layer_seed, offset=step, training=model.training)

    ``training=False`` or ``p == 0`` is exactly ``multihead_attention(A, Q, K, V, scale=scale, bias=bias)`` -- except with a
    ``scale`` and no bias, which that function would read as "the handle's values are the bias": that case stays on the route
    below with p = 0, whose bits are ``A.mhaEdgeBias(B=None)``'s.  Otherwise forward is
    ONE ``A.dropoutMha`` (one launch) and backward ONE ``A.dropoutMhaBackward`` (two launches) with the same (p, seed, offset), which
    recompute the mask: nothing of length nnz is kept or written beside ``grad_bias`` when the bias needs one.  Buffers, the
    companion and the workspace as ``multihead_attention``'s edge-bias route; the handle is given no values.  Nothing runs in
    backward when nothing needs a gradient.  fp32 and fp64 handles.

    A ``torch.bfloat16`` or ``torch.float16`` Q takes the 16-BIT ROUTE, whatever the handle's dtype: K, V and ``bias`` (``None`` or
    2-D (nnz, H)) have Q's dtype -- ValueError otherwise --, forward is ONE ``A.dropoutMhaLowp`` and backward ONE
    ``A.dropoutMhaLowpBackward`` (two launches) on the kept 16-bit tensors and on the incoming gradient as it arrives: fp32
    arithmetic, every output rounded once, 16-bit ``torch.empty`` outputs for exactly the inputs that need a gradient, a float32
    workspace of 4 m H values and the transposed companion only when K or V needs one, ``grad_bias`` the dB the kernel writes; no
    widened copy and no cast, on fp32 and fp64 handles alike.  The mask is the one ``A.dropoutMask`` gives for the same
    (p, seed, offset).  ``training=False`` and ``p == 0`` route as above: to ``multihead_attention``'s 16-bit route, or, with a
    scale and no bias, to this one with p = 0, whose words are ``A.mhaLowp(B=None)``'s."""
    if bias is not None and not (hasattr(bias, "dim") and bias.dim() == 2):
        raise ValueError("dropout_attention: bias is None or a 2-D (nnz, H) tensor in CSR order")
    p, seed, offset = _dropout_numbers("dropout_attention", p, seed, offset)
    lowp = getattr(Q, "dtype", None) in (torch.bfloat16, torch.float16)
    if lowp:
        for name, t in (("K", K), ("V", V), ("bias", bias)):
            if t is not None and getattr(t, "dtype", None) != Q.dtype:
                raise ValueError(f"dropout_attention: with bf16 / fp16 operands K, V and the bias (None or a 2-D (nnz, H) tensor) "
                                 f"have Q's dtype {Q.dtype}; {name} has {getattr(t, 'dtype', type(t).__name__)}")
    if (not training or p == 0.0) and (bias is not None or scale is None):
        return multihead_attention(A, Q, K, V, scale=scale, bias=bias)
    if not training:
        p = 0.0  # (a scale without a bias: multihead_attention would read the handle's values as the bias; p = 0 drops nothing)
    if lowp:
        return _LowpDropoutAttention.apply(A, Q, K, V, 1.0 if scale is None else float(scale), bias, p, seed, offset)
    return _DropoutAttention.apply(A, Q, K, V, 1.0 if scale is None else float(scale), bias, p, seed, offset)


class _GatDropoutAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, A, Q, K, V, att, negative_slope, scale, bias, p, seed, offset):
        Qc, Kc, Vc = (_packed(t.detach()) for t in (Q, K, V))
        ac = att.detach().contiguous() if att is not None else None
        Bc = _rows_packed(bias.detach()) if bias is not None else None
        _on_current_stream(A, Qc.device)
        O = torch.empty((A._m,) + tuple(Vc.shape[1:]), dtype=Vc.dtype, device=Vc.device)  # (the kernel writes every row and head)
        _check(A.dropoutGat(Qc, Kc, Vc, O, p, seed, offset, a=ac, negative_slope=negative_slope, B=Bc, scale=scale), "dropoutGat")
        ctx.A, ctx.ns, ctx.scale, ctx.drop = A, negative_slope, scale, (p, seed, offset)
        ctx.save_for_backward(Qc, Kc, Vc, ac, Bc)
        return O

    @staticmethod
    def backward(ctx, dO):
        Q, K, V, a, B = ctx.saved_tensors
        need = ctx.needs_input_grad[1:4]
        need_att = a is not None and ctx.needs_input_grad[4]
        need_bias = B is not None and ctx.needs_input_grad[7]
        if not (any(need) or need_att or need_bias):
            return (None,) * 11
        A = ctx.A
        dO, outs, work = _backward_plumbing(A, (Q, K, V), need, dO, Q.shape[1], dO.dtype)
        dB = torch.empty(tuple(B.shape), dtype=dO.dtype, device=dO.device) if need_bias else None  # (every element is written)
        dAr = torch.empty_like(Q, memory_format=torch.contiguous_format) if need_att else None  # (every row and head is written)
        p, seed, offset = ctx.drop
        _check(A.dropoutGatBackward(Q, K, V, dO, p, seed, offset, dQ=outs[0], dK=outs[1], dV=outs[2], work=work, a=a,
                                    negative_slope=ctx.ns, B=B, scale=ctx.scale, dB=dB, dAr=dAr), "dropoutGatBackward")
        grad_att = dAr.sum(0) if need_att else None  # (the kernels write the rows' shares: the reduction over the rows is torch's)
        return (None,) + tuple(outs) + (grad_att, None, None, dB, None, None, None)


def gat_dropout_attention(A, Q, K, V, p, seed, offset=0, att=None, negative_slope=0.2, scale=None, bias=None, training=True):
    """``gat_attention`` with ``dropout_attention``'s dropout on the attention weights -- PyG's ``GATConv(dropout=p)`` and
    ``GATv2Conv(dropout=p)`` recipe in the fused kernels.  The score is ``gat_attention``'s; ``p``, ``seed``, ``offset`` and the
    mask are ``dropout_attention``'s (the idiom: ``offset = step``).  ``training=False`` or ``p == 0`` is exactly
    ``gat_attention(A, Q, K, V, att, negative_slope, scale, bias)``.  Otherwise forward is ONE ``A.dropoutGat`` and backward ONE
    ``A.dropoutGatBackward`` with the same (p, seed, offset); ``grad_att`` and ``grad_bias`` as ``gat_attention``'s.  Nothing runs in
    backward when nothing needs a gradient."""
    if bias is not None and not (hasattr(bias, "dim") and bias.dim() == 2):
        raise ValueError("gat_dropout_attention: bias is None or a 2-D (nnz, H) tensor in CSR order")
    p, seed, offset = _dropout_numbers("gat_dropout_attention", p, seed, offset)
    if not training or p == 0.0:
        return gat_attention(A, Q, K, V, att=att, negative_slope=negative_slope, scale=scale, bias=bias)
    return _GatDropoutAttention.apply(A, Q, K, V, att, float(negative_slope), 1.0 if scale is None else float(scale), bias, p, seed,
                                      offset)
