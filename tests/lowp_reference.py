"""bf16 / fp16 for numpy, which has no bf16: a 16-bit tensor is its ``uint16`` words.  ``to_words`` rounds float32 values ONCE to
the operand type, to nearest even -- bf16 in integer arithmetic on the float32 bit pattern, fp16 by numpy's float16 -- and
``widen`` is the exact way back.  Words are compared with NaN treated positionally (``same_words``): the payload of a NaN is not
part of csr5hip_mha_lowp's contract (one rounding routine makes 0x7FC0 of a NaN, another 0xFFFF).

``round_allowance`` is the one rounding to the operand type that the float64 comparisons of the 16-bit call add to the fp32
allowance: |ref| 2^-8 for bf16 (8 significant bits: half an ulp is at most 2^-9 |x|, and ref is not the value rounded but within
the fp32 allowance of it, which the factor 2 covers), |ref| 2^-11 + 2^-24 for fp16 (11 significant bits, half an ulp at most
2^-12 |x|; 2^-24 is the spacing of the subnormals, of which half is the rounding and half the slack).  Derived, not measured."""
import numpy as np

KINDS = ("bf16", "f16")
NAN_WORD = {"bf16": 0x7FC0, "f16": 0x7E00}
_EXP = {"bf16": 0x7F80, "f16": 0x7C00}


def to_words(x, kind):
    """float32 array -> uint16 words of the operand type, one round-to-nearest-even; NaN -> the quiet NaN NAN_WORD[kind]"""
    x = np.ascontiguousarray(x)
    assert x.dtype == np.float32, "one rounding: from float32 only"
    if kind == "f16":
        with np.errstate(over="ignore"):
            w = x.astype(np.float16).view(np.uint16).copy()
    else:
        u = x.view(np.uint32).astype(np.uint64)
        w = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)  # (the carry of a round-up runs into the exponent: that is the rule)
    w[np.isnan(x)] = NAN_WORD[kind]
    return w


def widen(w, kind):
    """uint16 words -> float32, exact"""
    w = np.ascontiguousarray(w)
    assert w.dtype == np.uint16
    if kind == "f16":
        return w.view(np.float16).astype(np.float32)
    return (w.astype(np.uint32) << 16).view(np.float32)


def is_nan(w, kind):
    return (w & 0x7FFF) > _EXP[kind]


def same_words(got, want, kind):
    """equal words, or NaN in both, everywhere"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.uint16 and want.dtype == np.uint16 and got.shape == want.shape
    return bool(((got == want) | (is_nan(got, kind) & is_nan(want, kind))).all())


def round_allowance(ref, kind):
    ref = np.abs(np.asarray(ref, dtype=np.float64))
    return ref * 2.0 ** -8 if kind == "bf16" else ref * 2.0 ** -11 + 2.0 ** -24


def f64_case(mat, kind, heads, k, d, seed=2400):
    """(B, Q, K, V) as words and the scale of tests/test_gpu_mha_lowp.py's float64 comparison: everything uniform in [-1, 1), rounded
    once to the operand type, so fp16 neither overflows nor loses more than the one rounding; scale = float32(1 / sqrt(k))"""
    rng = np.random.default_rng([seed, mat.nnz, len(kind)])
    shapes = ((mat.nnz, heads), (mat.m, heads, k), (mat.n, heads, k), (mat.n, heads, d))
    return tuple(to_words(rng.uniform(-1, 1, size=s).astype(np.float32), kind) for s in shapes), float(np.float32(1 / np.sqrt(k)))
