"""What the twelve attention wrappers of ``handle.py`` do with their arguments, as text (no GPU): one line per (handle, method,
case) on stdout, either the exception a call raised or the argument tuple that reached the stubbed ``*_ptr`` method -- ints, floats
and None as they are, tensors by their keyword name.  Deterministic: two commits whose wrappers judge alike print the same bytes.

    python scripts/attention_wrapper_transcript.py > after.txt      # and on a checkout of the other commit > before.txt
    cmp before.txt after.txt

The line count and the SHA-256 of the output go to stderr.  ``--no-pairs`` leaves the precedence cases out (a few seconds
instead of a minute or two).

A call reaches the stub without a GPU because its tensors are CPU tensors inside ``OnGpu``, a proxy that forwards every attribute
and reports a CUDA device.  Handles: (6, 4) with nnz 7, H = 2, k = 3, d = 5 (m != n, H k != H d, nnz != m), the same before
``inputCSR``, (1, 1) with nnz 1 and H = k = d = 1, and (0, 4) with nnz 0; fp64 each, fp32 with bf16 operands for the 16-bit pair.
Cases: every single mistake of ``variants`` on every tensor argument, every bad value of ``SCALARS`` on every number, every two
arguments sharing one storage, the good calls of ``good_calls``, and every pair of single mistakes on two different arguments.
The pairs are made on the first handle only, which is this program's choice: the order of two checks does not depend on the sizes,
and the other three handles are there for the clauses that one mistake alone decides (before ``inputCSR``, one row, no elements).
tests/test_attention_wrappers_host.py takes its table and its cases from here."""
import argparse
import hashlib
import itertools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from benchmark_spmv_using_csr5_amd import handle as H  # noqa: E402

_F = ("Q", "ldq", "K", "ldk", "k", "V", "ldv", "d", "O", "ldo")
_B = ("Q", "ldq", "K", "ldk", "k", "V", "ldv", "d", "dO", "lddo", "dQ", "lddq", "dK", "lddk", "dV", "lddv", "work")
_EDGE = ("heads", "scale", "B", "ldb")
_GAT = ("heads", "negative_slope", "a", "scale", "B", "ldb")
# THE table: method -> (its *_ptr method, the rank of its operands, the positional arguments of the *_ptr call).  The method's
# own keywords are the entries that are neither a size, the operand type nor a leading dimension.
METHODS = {
    "attention": ("attention_ptr", 2, _F),
    "attentionBackward": ("attention_backward_ptr", 2, _B),
    "mha": ("mha_ptr", 3, ("heads",) + _F),
    "mhaBackward": ("mha_backward_ptr", 3, ("heads",) + _B),
    "mhaBiased": ("mha_biased_ptr", 3, ("heads", "scale", "slopes") + _F),
    "mhaBiasedBackward": ("mha_biased_backward_ptr", 3, ("heads", "scale", "slopes") + _B + ("dS", "ldds")),
    "mhaEdgeBias": ("mha_edge_bias_ptr", 3, _EDGE + _F),
    "mhaEdgeBiasBackward": ("mha_edge_bias_backward_ptr", 3, _EDGE + _B + ("dB", "lddb")),
    "mhaLowp": ("mha_lowp_ptr", 3, ("type",) + _EDGE + _F),
    "mhaLowpBackward": ("mha_lowp_backward_ptr", 3, ("type",) + _EDGE + _B + ("dB", "lddb")),
    "gat": ("gat_ptr", 3, _GAT + _F),
    "gatBackward": ("gat_backward_ptr", 3, _GAT + _B + ("dB", "lddb", "dAr", "lddar")),
}
LOWP = ("mhaLowp", "mhaLowpBackward")                          # bf16 operands on an fp32 handle
INPUT_FIRST = tuple(m for m in METHODS if m not in ("attention", "attentionBackward", "mha", "mhaBackward"))
OPERANDS = {"Q": "mk", "K": "nk", "V": "nd", "O": "md", "dO": "md", "dQ": "mk", "dK": "nk", "dV": "nd", "dAr": "mk"}
ENTRY = ("B", "dB", "dS")                                      # (nnz, heads)
NUMBERS = ("scale", "negative_slope")
OPTIONAL = ("dQ", "dK", "dV", "work", "slopes", "dS", "B", "dB", "a", "dAr")
OUTPUTS = ("O", "dQ", "dK", "dV", "dS", "dB", "dAr")
# name -> (m, n, nnz or None before inputCSR, heads, k, d)
HANDLES = {"6x4": (6, 4, 7, 2, 3, 5), "6x4-before-inputCSR": (6, 4, None, 2, 3, 5), "1x1": (1, 1, 1, 1, 1, 1), "0x4": (0, 4, 0, 2, 3, 5)}
SCALARS = (("nan", float("nan")), ("inf", float("inf")), ("None", None), ("'1'", "1"), ("True", True),
           ("tensor", torch.zeros(1, dtype=torch.float64)), ("2", 2), ("-0.5", -0.5))
WRONG = {torch.float64: (torch.float32, torch.bfloat16), torch.float32: (torch.float64, torch.bfloat16),
         torch.bfloat16: (torch.float16, torch.float32)}


class OnGpu:
    """a CPU tensor that says it lives on a GPU: every other attribute is the tensor's"""

    def __init__(self, t, device="cuda:0"):
        self._t, self.device = t, torch.device(device)

    def __getattr__(self, name):
        return getattr(self._t, name)


def keywords(method):
    return tuple(a for a in METHODS[method][2] if a not in ("heads", "k", "d", "type") and not a.startswith("ld"))


def dtypes(method):
    """(the handle's, the operands')"""
    return (torch.float32, torch.bfloat16) if method in LOWP else (torch.float64, torch.float64)


def make_handle(method, name):
    m, n, nnz = HANDLES[name][:3]
    A = H.anonymouslibHandle(m, n, "float32" if method in LOWP else "float64")
    if nnz is not None:
        assert A.inputCSR(nnz, None, None, None) == 0
    reached = []
    for ptr, _, _ in METHODS.values():
        setattr(A, ptr, lambda *a, _name=ptr: reached.append((_name, a)) or 0)  # nothing may reach the library
    return A, reached


def spec(method, name, arg):
    """(shape, dtype, the axis that counts heads or None, whether the last axis is a width) of a good ``arg``"""
    m, n, nnz, heads, k, d = HANDLES[name]
    nnz = 7 if nnz is None else nnz
    rank = METHODS[method][1]
    hdt, odt = dtypes(method)
    size = dict(m=m, n=n, k=k, d=d)
    if arg in OPERANDS:
        rows, width = (size[c] for c in OPERANDS[arg])
        return ((rows, width), odt, None, True) if rank == 2 else ((rows, heads, width), odt, 1, True)
    if arg == "work":
        return (4 * m * (heads if rank == 3 else 1),), hdt, None, False
    if arg == "slopes":
        return (heads,), hdt, 0, False
    if arg == "a":
        return (heads, k), hdt, 0, True
    assert arg in ENTRY, arg
    return (nnz, heads), (hdt if arg == "dS" else odt), 1, False


def good(method, name, arg):
    shape, dt, _, _ = spec(method, name, arg)
    return OnGpu(torch.zeros(shape, dtype=dt))


def _bump(shape, axis, by):
    s = list(shape)
    s[axis] += by
    return tuple(s)


def variants(method, name, arg):
    """every single mistake on the tensor ``arg`` (and a few shapes that are no mistake on some handles): (label, value)"""
    s, dt, heads_axis, has_width = spec(method, name, arg)

    def z(shape, dtype=dt):
        return torch.zeros(shape, dtype=dtype)
    out = [("numpy", np.zeros(s)), ("dtype", OnGpu(z(s, WRONG[dt][0]))), ("dtype'", OnGpu(z(s, WRONG[dt][1]))),
           ("rank+1", OnGpu(z(s + (1,))))]
    if len(s) >= 2:
        out.append(("rank-1", OnGpu(z(s[:-2] + (s[-2] * s[-1],)))))
    out.append(("rows+1", OnGpu(z(_bump(s, 0, 1)))))
    if s[0] > 0:
        out.append(("rows-1", OnGpu(z(_bump(s, 0, -1)))))
    if heads_axis:
        out.append(("heads+1", OnGpu(z(_bump(s, heads_axis, 1)))))
    if has_width:
        out.append(("width+1", OnGpu(z(_bump(s, -1, 1)))))
    wide = s[:-1] + (2 * s[-1],)
    out.append(("stride2", OnGpu(z(wide)[..., ::2])))
    if len(s) >= 2:
        out.append(("unpacked", OnGpu(z(wide)[..., :s[-1]])))
    out.append(("overlap", OnGpu(z((1,) + s[1:]).expand(s))))
    out += [("host", z(s)), ("cuda:1", OnGpu(z(s), "cuda:1")), ("None", None)]
    return out


def shared(method, name, x, y):
    """good ``x`` and ``y`` as disjoint views of ONE storage"""
    (sx, dx, _, _), (sy, dy, _, _) = spec(method, name, x), spec(method, name, y)
    bx, by = int(np.prod(sx)) * dx.itemsize, int(np.prod(sy)) * dy.itemsize
    at = (bx + 7) // 8 * 8
    pool = torch.zeros(at + by, dtype=torch.uint8)
    return OnGpu(pool[:bx].view(dx).view(sx)), OnGpu(pool[at:at + by].view(dy).view(sy))


def base(method, name, extras=True):
    """the good call: every keyword contiguous and given; ``extras=False``: only what the method has no default for, and work"""
    kw = {}
    for a in keywords(method):
        if a in NUMBERS:
            if extras:
                kw[a] = 0.5 if a == "scale" else 0.25
        elif extras or a in OPERANDS and a != "dAr" or a == "work":
            kw[a] = good(method, name, a)
    return kw


def good_calls(method, name):
    """(label, keywords) of the calls that should reach the library"""
    m, n, nnz, heads, k, d = HANDLES[name]
    rank = METHODS[method][1]
    full = base(method, name)
    yield "good", full
    yield "good defaults", base(method, name, extras=False)
    rows, cols = {}, {}
    for a in full:
        if a in OPERANDS:                                      # a row slice of a wider tensor
            s, dt, _, _ = spec(method, name, a)
            wide = torch.zeros(_bump(s, 1, s[1] if rank == 3 else 2), dtype=dt)
            rows[a] = OnGpu(wide[:, :s[1]])
        if a in ENTRY:                                         # a column slice of a wider tensor
            s, dt, _, _ = spec(method, name, a)
            cols[a] = OnGpu(torch.zeros(_bump(s, 1, 3), dtype=dt)[:, :s[1]])
    yield "good row slices", dict(full, **rows)
    if cols:
        yield "good column slices", dict(full, **cols)
        yield "good slices", dict(full, **rows, **cols)
    outs = [a for a in full if a in OUTPUTS and a in OPTIONAL]
    for a in outs:
        yield f"good {a}=None", dict(full, **{a: None})
        yield f"good row slices {a}=None", dict(dict(full, **rows), **{a: None})
    if outs:
        yield "good outputs=None", dict(full, **{a: None for a in outs})
        yield "good outputs=None work=None", dict(full, **{a: None for a in outs}, work=None)
        yield "good dK=None dV=None work=None", dict(full, dK=None, dV=None, work=None)


def outcome(A, reached, method, kw):
    """the line's right half: the exception, or what reached the stub"""
    del reached[:]
    try:
        getattr(A, method)(**kw)
    except Exception as e:  # noqa: BLE001  (whatever a wrapper raises is what it does)
        text = f"{type(e).__name__}: {e}".replace("\n", "\\n")
        return text + (" (AFTER THE LIBRARY WAS REACHED)" if reached else "")
    assert len(reached) == 1 and reached[0][0] == METHODS[method][0], (method, reached)

    def show(v):
        if hasattr(v, "data_ptr"):
            return next((a for a, t in kw.items() if t is v), "?")
        return repr(v)
    return "-> (" + ", ".join(show(v) for v in reached[0][1]) + ")"


def single_mistakes(method, name):
    """(label, {argument: value}) of every single mistake of the method: tensors, then numbers"""
    for a in keywords(method):
        if a in NUMBERS:
            for label, value in SCALARS:
                yield a, f"{a}={label}", value
        else:
            for label, value in variants(method, name, a):
                yield a, f"{a}={label}", value


def lines(pairs=True):
    for name in HANDLES:
        for method in METHODS:
            A, reached = make_handle(method, name)
            full = base(method, name)
            for label, kw in good_calls(method, name):
                yield f"{name} {method} {label}: {outcome(A, reached, method, kw)}"
            mistakes = list(single_mistakes(method, name))
            for a, label, value in mistakes:
                yield f"{name} {method} {label}: {outcome(A, reached, method, dict(full, **{a: value}))}"
            tensors = [a for a in full if a not in NUMBERS]
            for x, y in itertools.combinations(tensors, 2):
                tx, ty = shared(method, name, x, y)
                yield f"{name} {method} {x}~{y}: {outcome(A, reached, method, dict(full, **{x: tx, y: ty}))}"
            if pairs and name == "6x4":
                for (a, la, va), (b, lb, vb) in itertools.combinations(mistakes, 2):
                    if a != b:
                        yield f"{name} {method} {la},{lb}: {outcome(A, reached, method, dict(full, **{a: va, b: vb}))}"
            A.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--no-pairs", action="store_true", help="leave the precedence cases (pairs of mistakes) out")
    args = ap.parse_args()
    sha, count = hashlib.sha256(), 0
    for line in lines(pairs=not args.no_pairs):
        data = (line + "\n").encode()
        sha.update(data)
        count += 1
        sys.stdout.buffer.write(data)
    sys.stdout.flush()
    print(f"{count} lines, sha256 {sha.hexdigest()}", file=sys.stderr)


if __name__ == "__main__":
    main()
