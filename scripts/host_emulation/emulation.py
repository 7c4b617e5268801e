"""What the attention emulations (run_*.py) share: the build of attention_driver.cpp with the units a runner names, the matrices, the
operands, the case file and its launch, the slicing of the outputs with its assertions, the argument parser and the generic checks
of a case.  A runner keeps its reference and bound, its names, its defaults and the checks that are its own.

The case file's layout is DESIGN.md's ("The attention emulation's case file"); the order of the header's fields is FIELDS here and
struct Header in attention_driver.cpp, and nowhere else."""
import argparse
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from benchmark_spmv_using_csr5_amd import matrices as M  # noqa: E402
from tests import attention_edges as E  # noqa: E402
from tests import lowp_reference as L  # noqa: E402
from tests import sddmm_reference as S  # noqa: E402
from tests import zoo  # noqa: E402

MAGIC = 0x35545441
FIELDS = ("variant", "mode", "kind", "m", "n", "nnz", "sigma", "p", "sigma_t", "p_t", "k", "d", "heads", "groups",
          "ldq", "ldk", "ldv", "ldo", "lddq", "lddk", "lddv", "ldb", "lddb", "lddar", "ldm", "want",
          "has_b", "has_a", "has_slopes", "has_values", "has_map", "head0", "offk", "offd")
PLAIN, BIASED, EDGE, LOWP, GAT, DROP, DROP_GAT, DROP_LOWP = range(8)
SIXTEEN = (LOWP, DROP_LOWP)  # the variants whose case runs twice: the 16-bit call, then the float launcher on the widened operands
FORWARD, BACKWARD, MASK = range(3)
KIND = {"float64": 0, "float32": 1, "bf16": 2, "f16": 3}
# csr5_<unit>.hip, forward and backward of the variants in their order; the all-units program links too, and takes a minute to compile
ALL_UNITS = tuple("attention" + d + v for v in ("", "_bias", "_edge", "_lowp", "_gat", "_drop", "_drop_gat", "_drop_lowp") for d in ("", "_bwd"))

CONFIGS = ((4, 16, False, 0), (7, 4, True, 1), (16, 7, False, 1))  # sigma, the companion's sigma, padded, head groups (0: the rule)
SCALE = 0.37
EDGE_NAMES = ("O", "dQ", "dK", "dV", "dB")
# what a padded configuration adds to each leading dimension
PADS = dict(ldq=3, ldk=1, ldv=2, ldo=3, lddq=1, lddk=2, lddv=1, ldb=2, lddb=3, lddar=2, ldm=2)


def build(cxx, out, units):
    """attention_driver.cpp with csr5_<unit>.hip for every unit named, under the address and undefined-behaviour sanitizers"""
    assert set(units) <= set(ALL_UNITS), units
    cmd = [cxx, "-std=c++20", "-x", "c++", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-Wno-unknown-pragmas", f"-I{HERE}/fake", f"-I{ROOT}/benchmark_spmv_using_csr5_amd/csrc", f"-I{ROOT}/include",
           *(f"-DEMU_{u.upper()}" for u in units), os.path.join(HERE, "attention_driver.cpp"), "-o", out]
    subprocess.check_call(cmd)


def transpose_with_map(mat):
    """A^T in CSR with every column's entries in A's CSR order (a stable sort by column), and that sort: position in A^T's CSR ->
    position in A's CSR, the companion's source map"""
    rows = np.repeat(np.arange(mat.m, dtype=np.int64), np.diff(mat.row_ptr))
    cols = mat.col[:mat.nnz].astype(np.int64)
    order = np.argsort(cols, kind="stable")
    rp = np.zeros(mat.n + 1, dtype=np.int32)
    rp[1:] = np.cumsum(np.bincount(cols, minlength=mat.n))
    return M.CsrMatrix(mat.n, mat.m, rp, rows[order].astype(np.int32), np.ones(mat.nnz), mat.name + "^T"), order.astype(np.uint32)


def matrices():
    """name -> matrix: tests/zoo.py's, the duplicates matrix, class-edges and dealt; NAME^T is the transpose"""
    mats = {m.name: m for m in zoo.small_zoo()}
    mats["duplicates"] = S.duplicates_matrix()
    mats["class-edges"] = E.class_edges()
    mats["dealt"] = E.dealt()
    return lambda name: transpose_with_map(mats[name[:-2]])[0] if name.endswith("^T") else mats[name]


class Patterns:
    """A matrix, its transpose with the source map, both converted by the oracle at sigma = 4, 7 and 16 (val: the values in A's CSR
    order, for the variant that reads them), and the lines without entries"""

    def __init__(self, orc, mat, val=None, companion=True):
        self.mat = mat
        self.matT, self.amap = transpose_with_map(mat)
        val = np.ones(mat.nnz) if val is None else val
        self.conv = {s: orc.convert(64, s, mat.m, mat.row_ptr, mat.col, val) for s in (4, 7, 16)}
        if companion:
            self.convT = {s: orc.convert(64, s, self.matT.m, self.matT.row_ptr, self.matT.col, val[self.amap]) for s in (4, 7, 16)}
        self.empty_r, self.empty_c = np.diff(mat.row_ptr) == 0, np.diff(self.matT.row_ptr) == 0


def wide(t, ld, fill=np.nan):
    """(rows, ...) packed into rows of ld values, EXACTLY rows ld elements, the padding `fill`"""
    w = np.full((t.shape[0], ld), fill, dtype=t.dtype)
    w[:, :int(np.prod(t.shape[1:]))] = t.reshape(t.shape[0], -1)
    return w


def wide_bias(B, ldb, fill=np.nan):
    """(nnz, H) in rows of ldb values, EXACTLY nnz ldb elements, the padding columns `fill`"""
    return wide(B, ldb, fill)


def distinct_bias(nnz, H, seed=11):
    """(nnz, H) float64: a permutation of nnz H equidistant values in [-2, 2), distinct also in fp32"""
    B = (np.random.default_rng(seed).permutation(nnz * H) / max(nnz * H, 1) * 4 - 2).reshape(nnz, H)
    assert len(np.unique(B.astype(np.float32))) == nnz * H
    return B


def distinct_a(H, k, dtype):
    """(H, k): H k equidistant values in [-1, 1) without a zero, in an order of their own"""
    v = (np.random.default_rng(13).permutation(H * k) + 0.5) / (H * k) * 2 - 1
    return v.reshape(H, k).astype(dtype)


def operands(mat, H, k, d, dtype, seed=5):
    """Q (m, H, k), K (n, H, k), V (n, H, d), dO (m, H, d)"""
    rng = np.random.default_rng(seed)
    Q = (rng.uniform(-1, 1, (mat.m, H, k)) * 2).astype(dtype)
    K = rng.uniform(-1, 1, (mat.n, H, k)).astype(dtype)
    V = rng.uniform(-1, 1, (mat.n, H, d)).astype(dtype)
    dO = rng.uniform(-1, 1, (mat.m, H, d)).astype(dtype)
    return Q, K, V, dO


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def within(g, r, a, smag, u):
    """elementwise: |g - r| inside 1e3 u (1 + smag) max(a, 1e-30) + 1e-300, a the expression on absolute values and smag the
    largest score magnitude (NaN is outside): a check of the indexing, not the accuracy test"""
    return np.abs(g - r) <= 1e3 * u * (1 + smag) * np.maximum(a, 1e-30) + 1e-300


def edge_reference(mat, B, Q, K, V, dO, B_col=None):
    """(O, dQ, dK, dV, dB) of softmax(SCALE Q K^T + B), the same expressions on absolute values, and the largest score magnitude, in
    float64.  B (nnz, H) in CSR order.  B_col: the bias the COLUMN side (dK, dV) computes its scores with, when a wrong kernel is
    modelled whose two sides disagree; None for B."""
    Q, K, V, dO, B = (t.astype(np.float64) for t in (Q, K, V, dO, B))
    rows = np.repeat(np.arange(mat.m), np.diff(mat.row_ptr))
    cols = mat.col[:mat.nnz].astype(np.int64)
    H = Q.shape[1]

    def scatter(idx, n, terms):
        out = np.zeros((n,) + terms.shape[1:])
        np.add.at(out, idx, terms)
        return out

    def side(bias):
        s = SCALE * (Q[rows] * K[cols]).sum(2) + bias                                              # (nnz, H)
        mx = np.full((mat.m, H), -np.inf)
        np.maximum.at(mx, rows, s)
        w = np.exp(s - mx[rows])
        p = w / scatter(rows, mat.m, w)[rows]
        dp, adp = (dO[rows] * V[cols]).sum(2), (np.abs(dO[rows]) * np.abs(V[cols])).sum(2)
        ds = p * (dp - scatter(rows, mat.m, p * dp)[rows])
        ads = p * (adp + scatter(rows, mat.m, p * adp)[rows])
        return p, ds, ads
    smag = float((SCALE * (np.abs(Q[rows]) * np.abs(K[cols])).sum(2) + np.abs(B)).max()) if mat.nnz else 0.0
    p, ds, ads = side(B)
    if B_col is None:
        pc, dsc, adsc = p, ds, ads
    else:  # (the workspace of the row side -- M, r, D -- with the column side's scores: modelled as that side's own softmax)
        pc, dsc, adsc = side(B_col.astype(np.float64))
    got = (scatter(rows, mat.m, p[:, :, None] * V[cols]), SCALE * scatter(rows, mat.m, ds[:, :, None] * K[cols]),
           SCALE * scatter(cols, mat.n, dsc[:, :, None] * Q[rows]), scatter(cols, mat.n, pc[:, :, None] * dO[rows]), ds)
    mag = (scatter(rows, mat.m, p[:, :, None] * np.abs(V[cols])), SCALE * scatter(rows, mat.m, ads[:, :, None] * np.abs(K[cols])),
           SCALE * scatter(cols, mat.n, adsc[:, :, None] * np.abs(Q[rows])), scatter(cols, mat.n, pc[:, :, None] * np.abs(dO[rows])), ads)
    return got, mag, smag


def round_once(x, kind):
    """float64 -> words of the operand type in ONE rounding to nearest even: through float32 rounded TO ODD, which keeps the sticky
    information the second rounding needs"""
    x = np.asarray(x, dtype=np.float64)
    f = x.astype(np.float32)
    over = np.abs(f.astype(np.float64)) > np.abs(x)
    f = np.where(over, np.nextafter(f, np.float32(0)), f)  # truncated toward zero ...
    inexact = f.astype(np.float64) != x
    f = (f.view(np.uint32) | inexact.astype(np.uint32)).view(np.float32)  # ... and the sticky bit
    return L.to_words(f, kind)


def gradients(variant):
    """the backward's outputs in file order, by their `want` bit: 1 dQ, 2 dK, 4 dV, 8 dB (biased: dS), 16 dAr"""
    return (1, 2, 4) + ((8,) if variant != PLAIN else ()) + ((16,) if variant in (GAT, DROP_GAT) else ())


def launch(exe, tmp, variant, mode, pat, sigmas, ops, pad=False, groups=0, want=None, kind=None, B=None, a=None, slopes=None, values=False,
           scalars=(1.0, 0.0, 0.0, 0, 0), head0=0, single=None, pads=PADS):
    """Write one case and run the driver on it.  ops: Q, K, V and (backward) dO as (rows, heads, width), floats or -- kind "bf16" /
    "f16" -- the words of that type; scalars: scale, negative slope, p, seed, offset; single = h: the call with heads = 1 on head
    h's slices of the same packed rows.  Every padding element is NaN.
    FORWARD: O (m, H, d).  BACKWARD: ([dQ, dK, dV, dB, dAr] as far as the variant has them, None where not wanted; the workspace
    (m, heads, 4)).  MASK: (nnz, ldm) bytes.  LOWP and DROP_LOWP: two of these, the call's own in words and the float (edge, dropped) launcher's."""
    mat = pat.mat
    Q, V = ops[0], ops[2]
    (_, H, k), d, dtype = Q.shape, V.shape[2], Q.dtype
    wk, wd = H * k, H * d
    widths = dict(ldq=wk, ldk=wk, ldv=wd, ldo=wd, lddq=wk, lddk=wk, lddv=wd, ldb=H, lddb=H, lddar=wk, ldm=H)
    h = {name: width + (pads.get(name, PADS[name]) if pad else 0) for name, width in widths.items()}
    bits = gradients(variant)
    if 8 not in bits:
        h["lddb"] = 0
    if 16 not in bits:
        h["lddar"] = 0
    column = mode == BACKWARD and variant >= EDGE
    want = sum(bits) if want is None else want
    h.update(variant=variant, mode=mode, kind=KIND[kind or dtype.name], m=mat.m, n=mat.n, nnz=mat.nnz, sigma=sigmas[0],
             p=pat.conv[sigmas[0]].p, sigma_t=sigmas[1], p_t=pat.convT[sigmas[1]].p if mode == BACKWARD else 0, k=k, d=d,
             heads=H if single is None else 1, groups=groups, want=want if mode == BACKWARD else 0, has_b=int(B is not None),
             has_a=int(a is not None), has_slopes=int(slopes is not None), has_values=int(values), has_map=int(column), head0=head0,
             offk=0 if single is None else single * k, offd=0 if single is None else single * d)
    fill = L.NAN_WORD[kind] if kind else np.nan
    case, out = os.path.join(tmp, "case.bin"), os.path.join(tmp, "out.bin")
    with open(case, "wb") as f:
        np.array([MAGIC, len(FIELDS)], dtype=np.uint32).tofile(f)
        np.array([h[name] for name in FIELDS], dtype=np.int32).tofile(f)
        np.array(scalars[:3], dtype=np.float64).tofile(f)
        np.array(scalars[3:], dtype=np.uint64).tofile(f)
        for mt, fmt in ((mat, pat.conv[sigmas[0]]),) + (((pat.matT, pat.convT[sigmas[1]]),) if mode == BACKWARD else ()):
            mt.row_ptr.astype(np.int32).tofile(f)
            fmt.col[:mt.nnz].astype(np.int32).tofile(f)
            fmt.tile_ptr.astype(np.uint32).tofile(f)
            if values:
                fmt.val[:mt.nnz].astype(dtype).tofile(f)
        if column:
            pat.amap.astype(np.uint32).tofile(f)
        for t in (a, slopes):
            if t is not None:
                np.ascontiguousarray(t, dtype=dtype).tofile(f)
        if B is not None:
            wide(B.astype(dtype), h["ldb"], fill).tofile(f)
        if mode != MASK:
            for t, ld in zip(ops[:4 if mode == BACKWARD else 3], ("ldq", "ldk", "ldv", "ldo")):
                wide(t, h[ld], fill).tofile(f)
    r = subprocess.run([exe, case, out], capture_output=True, text=True)
    if r.returncode:
        raise SystemExit(f"{mat.name} sigma {sigmas} variant {variant} mode {mode}: exit {r.returncode}\n{r.stderr[-4000:]}")
    raw = np.fromfile(out, dtype=np.uint8)
    if mode == MASK:
        return raw.reshape(mat.nnz, h["ldm"])
    at, sets = 0, []

    def take(dt, rows, ld, width, shape, wanted=True):
        nonlocal at
        g = raw[at:at + dt.itemsize * rows * ld].view(dt).reshape(rows, ld)
        at += g.nbytes
        poison = (lambda x: x == 0xFFFF) if dt == np.uint16 else np.isnan
        assert poison(g[:, width:]).all(), "written beyond the last column"
        if wanted:
            return np.ascontiguousarray(g[:, :width]).reshape(shape)
        assert poison(g).all(), "an output that was not wanted is written"
        return None
    for dt in (dtype, np.dtype(np.float32)) if variant in SIXTEEN else (dtype,):
        if mode == FORWARD:
            sets.append(take(dt, mat.m, h["ldo"], wd, (mat.m, H, d)))
            continue
        shapes = {1: (mat.m, "lddq", k), 2: (mat.n, "lddk", k), 4: (mat.n, "lddv", d), 8: (mat.nnz, "lddb", 1), 16: (mat.m, "lddar", k)}
        outs = []
        for b in bits:
            rows, ld, width = shapes[b]
            outs.append(take(dt, rows, h[ld], H * width, (rows, H) + ((width,) if b != 8 else ()), want & b))
        work = take(np.dtype(np.float32) if variant in SIXTEEN else dt, 4 * mat.m * h["heads"], 1, 1, (mat.m, h["heads"], 4), want & 6)
        sets.append((outs, work))
    assert at == raw.size
    return sets if variant in SIXTEEN else sets[0]


def arguments(matrices, heads=None, kd=None, kinds="dtypes", extra=()):
    """the runners' command line: --matrices, --cxx and, as far as the runner has them, --dtypes f64,f32 or --types bf16,f16, --heads,
    --kd KxD,...; extra: (flag, keywords) of the runner's own"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrices", default=matrices)
    if kinds:
        ap.add_argument("--" + kinds, default="f64,f32" if kinds == "dtypes" else ",".join(L.KINDS))
    if heads:
        ap.add_argument("--heads", default=",".join(str(h) for h in heads))
    if kd:
        ap.add_argument("--kd", default=",".join(f"{k}x{d}" for k, d in kd), help="a subset lets the slow cases run side by side")
    for flag, keywords in extra:
        ap.add_argument(flag, **keywords)
    ap.add_argument("--cxx", default="/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else "clang++")
    args = ap.parse_args()
    args.matrices = args.matrices.split(",")
    args.dtypes = [{"f64": np.float64, "f32": np.float32}[t] for t in getattr(args, "dtypes", "f64,f32").split(",")]
    args.types = getattr(args, "types", "").split(",")
    args.heads = [int(h) for h in args.heads.split(",")] if heads else None
    args.kd = [tuple(int(v) for v in s.split("x")) for s in args.kd.split(",")] if kd else None
    return args


def check_configs(both, names, empties, where, judge=None, isnan=np.isnan, configs=CONFIGS):
    """The checks every runner makes of one case.  both(sigma, sigma_t, padded, groups) -> the outputs in the order of `names` (None:
    the case has no such output).  Per configuration: nothing unwritten or poisoned, every output inside the runner's bound
    (judge(i, g) -> (elementwise ok, the worst |error|)), lines without entries (empties[i]; None: no such lines) exactly +0, and
    equal bits across the configurations.  Returns the first configuration's outputs and the worst |error|."""
    first, worst = None, 0.0
    for sigma, sigma_t, pad, groups in configs:
        got = both(sigma, sigma_t, pad, groups)
        for i, (g, e, what) in enumerate(zip(got, empties, names)):
            if g is None:
                continue
            assert not isnan(g).any(), where + (sigma, what, "unwritten or poisoned")
            if judge:
                ok, err = judge(i, g)
                assert ok.all(), where + (sigma, what, err)
                worst = max(worst, err)
            if e is not None:
                assert not np.ascontiguousarray(g[e]).view(np.uint8).any(), f"{what}: a line without entries is not +0"
        first = got if first is None else first
        check_same(got, first, names, where + (sigma,), "bits")
    return first, worst


def check_same(got, expected, names, where, why):
    """equal bits of every output that `got` has: a null optional operand against its neutral value, a subset of the outputs alone
    against the full call, one configuration against another"""
    for g, g0, what in zip(got, expected, names):
        assert g is None or same(g, g0), where + (what, why)


def worst_of(g, r):
    return float(np.abs(g - r).max()) if g.size else 0.0
