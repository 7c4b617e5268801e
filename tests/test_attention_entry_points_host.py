"""The twelve attention entry points of the C ABI judge their arguments alike (no GPU): ONE table of the calls and their argument
lists, and every mistake -- a null handle, a negative size, a non-finite scale or slope, a leading dimension too small, a null
operand, the missing companion, the CSR and the unknown format -- made in every call that has the argument, with the same code
expected everywhere.  The per-call tests (test_attention_host.py, test_attention_backward_host.py, test_mha_host.py,
test_mha_bias_host.py, test_mha_edge_bias_host.py, test_mha_lowp_host.py, test_mha_lowp_backward_host.py, test_gat_host.py) pin each
call's order on its own; this one pins that the calls agree (tests/test_attention_wrappers_host.py does the same for the Python
wrappers).  Handles as
test_mha_edge_bias_host.py makes them: csr5hip_create, then csr5hip_input_csr with null arrays, and fake non-null pointers --
nothing is launched, csr5hip_get_info is the same bytes before and after."""
import ctypes as C

import pytest

from benchmark_spmv_using_csr5_amd import _capi

M, N, NNZ = 10, 12, 100
K, D, HEADS = 4, 5, 3
FAKE = C.c_void_p(64)
INV, CSR, UNK, TYPE = _capi.INVALID_ARGUMENT, _capi.UNSUPPORTED_CSR_SPMV, _capi.UNKOWN_FORMAT, _capi.UNSUPPORTED_VALUE_TYPE

_FWD = ("Q", "ldq", "K", "ldk", "k", "V", "ldv", "d", "O", "ldo")
_BWD = ("Q", "ldq", "K", "ldk", "k", "V", "ldv", "d", "dO", "lddo", "dQ", "lddq", "dK", "lddk", "dV", "lddv", "work")
# the arguments of every entry point in the order of its declaration; "dS" / "ldds" stand for the edge call's dB / lddb as well
ENTRIES = {
    "csr5hip_attention": ("handle",) + _FWD,
    "csr5hip_attention_backward": ("handle",) + _BWD,
    "csr5hip_mha": ("handle", "heads") + _FWD,
    "csr5hip_mha_backward": ("handle", "heads") + _BWD,
    "csr5hip_mha_biased": ("handle", "heads", "scale", "slopes") + _FWD,
    "csr5hip_mha_biased_backward": ("handle", "heads", "scale", "slopes") + _BWD + ("dS", "ldds"),
    "csr5hip_mha_edge_bias": ("handle", "heads", "scale", "B", "ldb") + _FWD,
    "csr5hip_mha_lowp": ("handle", "type", "heads", "scale", "B", "ldb") + _FWD,
    "csr5hip_mha_edge_bias_backward": ("handle", "heads", "scale", "B", "ldb") + _BWD + ("dS", "ldds"),
    "csr5hip_mha_lowp_backward": ("handle", "type", "heads", "scale", "B", "ldb") + _BWD + ("dS", "ldds"),
    "csr5hip_gat": ("handle", "heads", "negative_slope", "a", "scale", "B", "ldb") + _FWD,
    "csr5hip_gat_backward": ("handle", "heads", "negative_slope", "a", "scale", "B", "ldb") + _BWD + ("dS", "ldds", "dAr", "lddar"),
}
BACKWARD = [name for name in ENTRIES if name.endswith("_backward")]
# leading dimension -> (what it is a multiple of, the pointer it is judged with or None for always)
LEADING = {"ldq": ("k", None), "ldk": ("k", None), "lddq": ("k", None), "lddk": ("k", None), "ldv": ("d", None), "ldo": ("d", None),
           "lddo": ("d", None), "lddv": ("d", None), "ldb": (None, "B"), "ldds": (None, "dS"), "lddar": ("k", "dAr")}


class Entry:
    """one entry point on one handle: call(**changes) makes the good call with these arguments changed"""

    def __init__(self, lib, handle, name):
        self.fn, self.name, self.args = getattr(lib, name), name, ENTRIES[name]
        self.heads = HEADS if "heads" in self.args else 1
        self.good = dict(handle=handle, type=_capi.BF16, heads=self.heads, scale=0.5, slopes=FAKE, B=FAKE, ldb=self.heads, Q=FAKE, K=FAKE,
                         V=FAKE, O=FAKE, dO=FAKE, k=K, d=D, dQ=FAKE, dK=None, dV=None, work=None, dS=None, ldds=self.heads,
                         negative_slope=0.2, a=FAKE, dAr=None)
        for ld, (width, _) in LEADING.items():
            if width:
                self.good[ld] = self.heads * self.good[width]

    def has(self, *args):
        return all(a in self.args for a in args)

    def call(self, **changes):
        unknown = set(changes) - set(self.args)
        assert not unknown, (self.name, unknown)
        values = dict(self.good, **changes)
        return self.fn(*(values[a] for a in self.args))


@pytest.fixture()
def entries():
    lib = _capi.load()
    h = C.c_void_p()
    assert lib.csr5hip_create(C.byref(h), M, N, _capi.F64) == 0
    yield lib, h, [Entry(lib, h, name) for name in ENTRIES]
    assert lib.csr5hip_free(h) == 0


def _info_bytes(lib, h):
    info = _capi.Csr5Info()
    assert lib.csr5hip_get_info(h, C.byref(info)) == 0
    return bytes(info)


def _argument_mistakes(e, fmt):
    """every mistake that is judged before the format, on a handle whose good call returns `fmt`"""
    assert e.call() == fmt, e.name
    assert e.call(handle=None) == INV, e.name
    if e.has("type"):  # after the handle, before everything else
        for bad in (_capi.F64, _capi.F32, 7, -1):
            assert e.call(type=bad) == TYPE and e.call(type=bad, heads=-1, ldq=0, Q=None) == TYPE, (e.name, bad)
        assert e.call(type=_capi.F16) == fmt and e.call(type=7, handle=None) == INV, e.name
    for size in ("heads", "k", "d"):
        if e.has(size):
            assert e.call(**{size: -1}) == INV, (e.name, size)
    if e.has("scale"):
        for bad in (float("nan"), float("inf"), -float("inf")):
            assert e.call(scale=bad) == INV, (e.name, bad)
        assert e.call(scale=0.0) == fmt and e.call(scale=-3.0) == fmt, e.name
    if e.has("negative_slope"):
        for bad in (float("nan"), float("inf"), -float("inf")):
            assert e.call(negative_slope=bad) == INV, (e.name, bad)
        assert e.call(negative_slope=0.0) == fmt and e.call(negative_slope=-3.0) == fmt, e.name
    for ld, (_, pointer) in LEADING.items():
        if not e.has(ld):
            continue
        given = {pointer: FAKE} if pointer else {}
        assert e.call(**{ld: e.good[ld] - 1}, **given) == INV, (e.name, ld)
        assert e.call(**{ld: e.good[ld] + 3}, **given) == fmt, (e.name, ld)
        # before the null operands and before the companion
        assert e.call(**{ld: e.good[ld] - 1}, **given, Q=None) == INV, (e.name, ld)
        if pointer:  # judged only with its pointer given
            assert e.call(**{ld: 0, pointer: None}) == fmt, (e.name, ld)
    # the output of the forward is judged whatever the format: the handle has rows
    if e.has("O"):
        assert e.call(O=None) == INV, e.name
    # the trivial cases return only after the format
    assert e.call(d=0, ldv=0, V=None) == fmt, e.name
    assert e.call(k=0, ldq=0, ldk=0, Q=None, K=None) == fmt, e.name
    if e.has("heads"):
        assert e.call(heads=0, ldq=0, ldk=0, ldv=0, Q=None, K=None, V=None) == fmt, e.name
        if e.has("O"):
            assert e.call(heads=0, O=None) == fmt and e.call(d=0, O=None) == fmt, e.name


def _missing_companion(e, other, **changes):
    """the call asks for dK or dV on a handle without the companion: INVALID with the call's OWN name in last_error()"""
    assert other.call(dK=FAKE, work=FAKE) == INV and other.name + ":" in _capi.last_error()  # (another call's name first)
    assert e.call(**changes) == INV, e.name
    text = _capi.last_error()
    return text.startswith(e.name + ":") and "csr5hip_build_transpose" in text


def test_every_entry_point_is_in_the_table():
    lists = (_capi.SYMBOLS + _capi.SYMBOLS_BIASED + _capi.SYMBOLS_EDGE_BIAS + _capi.SYMBOLS_LOWP + _capi.SYMBOLS_LOWP_BACKWARD
             + _capi.SYMBOLS_GAT)
    bound = [name for name, _, _ in lists if name.startswith(("csr5hip_attention", "csr5hip_mha", "csr5hip_gat"))]
    assert sorted(bound) == sorted(ENTRIES) and len(ENTRIES) == 12
    for name, _, argtypes in lists:
        if name in ENTRIES:
            assert len(argtypes) == len(ENTRIES[name]), name
            for arg, ctype in zip(ENTRIES[name], argtypes):
                integer = arg in ("type", "heads", "k", "d") or arg.startswith("ld")
                assert ctype is (C.c_double if arg in ("scale", "negative_slope") else C.c_int if integer else C.c_void_p), (name, arg)


def test_the_same_mistake_gets_the_same_code_before_input(entries):
    """the unknown format: a handle that holds no matrix (m = 10 rows, no entries)"""
    lib, h, table = entries
    before = _info_bytes(lib, h)
    for e in table:
        _argument_mistakes(e, UNK)
        assert e.call(Q=None, K=None, V=None) == UNK, e.name  # no entries: the operands are not judged
    for i, name in enumerate(BACKWARD):
        e, other = Entry(lib, h, name), Entry(lib, h, BACKWARD[(i + 1) % len(BACKWARD)])
        assert _missing_companion(e, other, dK=FAKE, work=FAKE) and _missing_companion(e, other, dV=FAKE, work=FAKE)  # before the format
        assert e.call(dK=FAKE, dV=FAKE) == INV                 # (no entries: the workspace is not judged, the companion is)
    assert _info_bytes(lib, h) == before


def test_the_same_mistake_gets_the_same_code_in_csr_format(entries):
    """the CSR format with entries: csr5hip_input_csr with null arrays"""
    lib, h, table = entries
    assert lib.csr5hip_input_csr(h, NNZ, None, None, None) == 0
    before = _info_bytes(lib, h)
    for e in table:
        _argument_mistakes(e, CSR)
        for operand in ("Q", "K", "V", "O", "dO"):
            if e.has(operand):
                assert e.call(**{operand: None}) == INV, (e.name, operand)
        if e.has("slopes"):
            assert e.call(slopes=None) == CSR, e.name         # optional
        if e.has("B"):
            assert e.call(B=None) == CSR, e.name              # optional
        if e.has("a"):
            assert e.call(a=None) == CSR, e.name              # optional: a = 1
    for i, name in enumerate(BACKWARD):
        e, other = Entry(lib, h, name), Entry(lib, h, BACKWARD[(i + 1) % len(BACKWARD)])
        assert _missing_companion(e, other, dK=FAKE, work=FAKE) and _missing_companion(e, other, dV=FAKE, work=FAKE)
        assert _missing_companion(e, other, dQ=None, dK=FAKE, dV=FAKE, work=FAKE)
        if e.has("heads"):
            assert _missing_companion(e, other, heads=0, dK=FAKE)  # (no heads: nothing else is judged, the companion is)
        # the null operands and the workspace come before the companion: the other call's text stays
        for changes in (dict(dK=FAKE), dict(dV=FAKE), dict(dK=FAKE, work=FAKE, Q=None), dict(dV=FAKE, work=FAKE, dO=None)):
            assert other.call(dK=FAKE, work=FAKE) == INV
            text = _capi.last_error()
            assert e.call(**changes) == INV and _capi.last_error() == text and e.name + ":" not in text, (e.name, changes)
        # nothing wanted: nothing judged but the arguments' signs, the leading dimensions and the format
        assert e.call(dQ=None, Q=None, K=None, V=None, dO=None) == CSR, e.name
        assert e.call(dQ=None, k=-1) == INV and e.call(dQ=None, ldq=e.good["ldq"] - 1) == INV, e.name
        if e.has("dS"):  # dS / dB alone is a wanted output
            assert e.call(dQ=None, dS=FAKE) == CSR and e.call(dQ=None, dS=FAKE, Q=None) == INV, e.name
        if e.has("dAr"):  # and so is dAr
            assert e.call(dQ=None, dAr=FAKE) == CSR and e.call(dQ=None, dAr=FAKE, Q=None) == INV, e.name
    assert _info_bytes(lib, h) == before
