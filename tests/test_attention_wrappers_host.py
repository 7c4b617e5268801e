"""The twelve attention wrappers of handle.py judge their arguments alike (no GPU): the Python twin of
test_attention_entry_points_host.py.  ONE table -- ``METHODS`` of scripts/attention_wrapper_transcript.py, whose cases these are: the
method, its ``*_ptr`` method and that call's positional arguments, from which the method's own keywords follow -- and every single
mistake (not a tensor, dtype, rank, rows, heads, width, inner stride, packing, overlapping rows, a host tensor, the other device,
None; nan, inf, None, a string, a bool, a tensor for a number) made in every method that has the argument.  ``legal`` says, from the
argument's shape alone, which of the cases is no mistake; every other one must raise ValueError with nothing reaching a ``*_ptr``
method, and its message must be the same text in all twelve wrappers up to the method's name.  Where the wrappers differ on purpose
the tables below say so and nothing else is forgiven: ``WORDING`` (what the 2-D and the 16-bit wrappers word differently),
``DIFFERENT`` (the few cases whose text is another one, with that text), ``INPUT_FIRST`` (where "call inputCSR first" stands in the
order), ``ENTRY_SPELLING`` (the two spellings of a shared storage) and ``NEVER_COMPARED`` (``slopes``).  The per-call tests
(test_attention_host.py ... test_gat_host.py) pin each wrapper on its own; this one pins that they agree and that a good call
reaches the library with the expected arguments.  Tensors are CPU tensors that report a CUDA device (``OnGpu``), handles as the
transcript makes them."""
import inspect
import itertools
import re

import pytest

torch = pytest.importorskip("torch")

from benchmark_spmv_using_csr5_amd import _capi  # noqa: E402
from benchmark_spmv_using_csr5_amd import handle as H  # noqa: E402
from scripts import attention_wrapper_transcript as T  # noqa: E402

METHODS = T.METHODS
# what the wrappers word differently on purpose, taken out of a message before it is compared: (pattern, what stands for it)
WORDING = (
    (r", not .*$", ", not <what it got>"),                                   # the tensor's own shape, strides, device; the value
    (r"\((\d+), (heads, )?(k|d)\)", r"(\1, [heads, ]\3)"),                   # 2-D operands have no heads ...
    (r"must be row-major with stride\(1\) == 1|must have stride\(2\) == 1", "must have a unit inner stride"),
    (r"< (heads \* )?(k|d) = \d+\)", r"< [heads * ]\2)"),                      # ... so a row is one width wide
    (r"has (\d+) columns", r"has width \1"),                                 # and the width is called columns
    (r"work must have shape \(\d+,\)", "work must have shape (4 m heads,)"),
    (r"(the handle holds|Q has) torch\.\w+$", "<whose dtype counts>"),        # 16-bit: the operands follow Q, not the handle
    (r"has dtype torch\.\w+", "has dtype <the wrong one>"),
)
# the cases whose text is another one in some wrappers: (which wrappers, the case) -> the text after the method's name
_NO_16 = "Q must be a torch.bfloat16 or torch.float16 tensor, not "
DIFFERENT = {
    (T.LOWP, "Q=numpy"): _NO_16 + "float64",                 # the 16-bit pair reads the operand type off Q before anything else
    (T.LOWP, "Q=None"): _NO_16 + "NoneType",
    (T.LOWP, "Q=dtype'"): _NO_16 + "torch.float32",
    (T.LOWP, "Q=dtype"): "K has dtype torch.bfloat16, Q has torch.float16",  # (fp16 is a legal Q: the others then miss it)
    (("mhaLowpBackward",), "work=dtype"): "work has dtype torch.float64, it must be torch.float32 whatever the operands' dtype",
    (("mhaLowpBackward",), "work=dtype'"): "work has dtype torch.bfloat16, it must be torch.float32 whatever the operands' dtype",
}
# a V that is wider than the rest is told the first tensor that disagrees: O in a forward, dO in a backward
FIRST_AFTER_V = {"V=width+1": (r", dO (\d+)$", r", O \1")}
# "call inputCSR first" is said before anything else by the methods with a scale (their first group of checks begins with it),
# after the shapes and before the aliasing and the devices by the four plain ones
INPUT_FIRST = T.INPUT_FIRST
# an output among the operands "shares storage with X (aliased)"; a per-entry output is judged earlier and differently
OPERAND_SPELLING = "{who}: {out} shares storage with {other} (aliased)"
ENTRY_SPELLING = "{who}: {out} shares a storage with {other} (views of one storage are rejected, disjoint or not)"
# slopes is compared with nothing: mhaBiased takes an O and mhaBiasedBackward a dS in slopes' storage, and slopes on another GPU
# than Q's (dS as well).  Kept as found: the wrappers' behaviour is not this file's to change
NEVER_COMPARED = ("slopes",)
LD = {"ldq": "Q", "ldk": "K", "ldv": "V", "ldo": "O", "lddo": "dO", "lddq": "dQ", "lddk": "dK", "lddv": "dV", "lddar": "dAr",
      "ldb": "B", "lddb": "dB", "ldds": "dS"}


def _who(method, text):
    assert text.startswith(f"ValueError: {method}: "), (method, text)
    return "{who}: " + text[len(f"ValueError: {method}: "):]


def legal(method, name, arg, label):
    """whether the case ``arg=label`` of T.single_mistakes is NO mistake in the call that has Q, K, V, the outputs and work and
    nothing else: decided from the argument's shape, not from what a wrapper does"""
    label = label.split("=", 1)[1]
    if arg in T.NUMBERS:
        return label in ("2", "-0.5") and T.HANDLES[name][2] is not None
    if T.HANDLES[name][2] is None:
        return False                                           # before inputCSR nothing is legal
    shape = T.spec(method, name, arg)[0]
    empty = 0 in shape                                         # a tensor without elements has no strides to judge
    if label == "None":
        return arg in T.OPTIONAL and arg != "work"             # (the call wants dK and dV, so it wants work)
    if label == "cuda:1":
        return arg in NEVER_COMPARED or arg == "dS"            # (only that they live on SOME GPU is judged)
    if label == "rows+1":
        return arg == "work"                                   # "or longer"
    if label == "stride2":
        return empty or shape[-1] <= 1                         # a stride of a dimension of one element is nobody's business
    if label == "overlap":
        return empty or shape[0] <= 1
    if label == "unpacked":                                    # a slice [..., :w] of a tensor twice as wide
        if arg in T.ENTRY or (arg in T.OPERANDS and METHODS[method][1] == 2):
            return True                                        # 2-D: the row stride is free
        return empty or shape[-2] <= 1                         # packed operands and a: the dimension before the last
    return False


def _one_mistake(name, method, arg, value, label=None):
    """the method called with its required arguments, ``work`` and ``arg=value``: what it raised, or '-> (...)' where the call
    reached the ``*_ptr`` method; with ``label``, judged by ``legal``"""
    A, reached = T.make_handle(method, name)
    text = T.outcome(A, reached, method, dict(T.base(method, name, extras=False), **{arg: value}))
    A.close()
    assert "AFTER THE LIBRARY" not in text, (name, method, arg, text)
    if label is not None and legal(method, name, arg, label):
        assert text.startswith("-> (") and len(reached) == 1, (name, method, label, text)
    elif label is not None:
        assert text.startswith(f"ValueError: {method}: ") and reached == [], (name, method, label, text)
    return text


def test_the_table_names_every_wrapper_and_its_arguments():
    assert len(METHODS) == 12
    public = [n for n, f in vars(H.anonymouslibHandle).items() if n.endswith("_ptr") and n.startswith(("attention", "mha", "gat"))]
    assert sorted(public) == sorted(ptr for ptr, _, _ in METHODS.values())
    for method, (ptr, rank, layout) in METHODS.items():
        own = list(inspect.signature(getattr(H.anonymouslibHandle, method)).parameters)[1:]
        assert sorted(own) == sorted(T.keywords(method)), method
        raw = list(inspect.signature(getattr(H.anonymouslibHandle, ptr)).parameters)[1:]
        assert raw == ["operand_type" if a == "type" else a for a in layout], method
        assert ("heads" in layout) == (rank == 3), method
        assert all(ld in layout for ld, t in LD.items() if t in layout) and all(LD[a] in layout for a in layout if a in LD), method


@pytest.mark.parametrize("name", list(T.HANDLES))
def test_the_same_mistake_gets_the_same_message_in_every_wrapper(name):
    """per argument and case: accepted where ``legal`` says so, else ValueError before the library, and ONE text in all twelve
    wrappers once ``WORDING`` is taken out (before inputCSR: one text among those that judge it at the same place).  The list of
    devices that the other-device message prints is the wrapper's own list of tensors, so it is compared as such."""
    seen, texts = {}, {}
    for method in METHODS:
        given = [a for a in T.base(method, name, extras=False)]
        for arg, label, value in T.single_mistakes(method, name):
            text = _one_mistake(name, method, arg, value, label)
            if text.startswith("-> ("):
                continue
            text = _who(method, text)
            other = [t for (who, case), t in DIFFERENT.items() if method in who and case == label]
            if other and (T.HANDLES[name][2] is not None or other[0].startswith(_NO_16)):  # (that one comes before inputCSR too)
                assert text == "{who}: " + other[0], (name, method, label, text)
                continue
            if re.search(r" on cuda:\d, ", text):  # every tensor of the call and where it lives, in the order of the call
                on = [a for a in dict.fromkeys(given + [arg]) if a in T.OPERANDS] + [a for a in given if a == "work"]
                if arg not in on:                  # (a tensor beside the operands is compared with Q alone)
                    assert text == f"{{who}}: {arg} on cuda:1, Q on cuda:0", (method, label, text)
                else:
                    assert text == "{who}: " + ", ".join(f"{a} on cuda:{int(a == arg)}" for a in on), (method, label, text)
                text = "devices"
            for pattern, stands in WORDING + ((FIRST_AFTER_V[label],) if label in FIRST_AFTER_V else ()):
                text = re.sub(pattern, stands, text)
            texts[method, label] = text
            # (before inputCSR: among those that judge it at the same place, and what would be legal after it apart from the rest)
            group = (method in INPUT_FIRST, legal(method, "6x4", arg, label)) if T.HANDLES[name][2] is None else None
            first = seen.setdefault((group, label), (method, text))
            assert text == first[1], (name, label, method, text, first)
    assert len(seen) > 130
    for (method, label), text in texts.items():  # dAr is judged as dQ is
        if label.startswith("dAr="):
            assert text.replace("dAr", "dQ") == texts[method, "dQ=" + label[4:]], (name, label, text)


def test_the_place_of_inputCSR_in_the_order():
    """the quirk that is kept on purpose: the methods of INPUT_FIRST say "call inputCSR first" whatever else is wrong (the 16-bit
    pair after judging Q's dtype); the four plain ones judge the shapes and ``work`` first, the aliasing and the devices after"""
    name = "6x4-before-inputCSR"
    for method in METHODS:
        want = f"ValueError: {method}: call inputCSR first"
        mistakes = {label: (arg, value) for arg, label, value in T.single_mistakes(method, name)}
        if method in INPUT_FIRST:
            for label, (arg, value) in mistakes.items():
                text = _one_mistake(name, method, arg, value)
                assert text == want or (method in T.LOWP and arg == "Q" and "Q must be a torch.bfloat16 or torch.float16" in text), label
        else:
            assert _one_mistake(name, method, *mistakes["K=rows+1"]).startswith(f"ValueError: {method}: K must have shape")
            assert "V has" in _one_mistake(name, method, *mistakes["V=width+1"])
            if "work" in T.keywords(method):
                assert "work must have shape" in _one_mistake(name, method, *mistakes["work=rows-1"])
            assert _one_mistake(name, method, *mistakes["Q=host"]) == want       # the devices are judged after it
            assert _one_mistake(name, method, *mistakes["K=cuda:1"]) == want
        A, reached = T.make_handle(method, name)  # and so is the aliasing, in all twelve
        x, y = T.shared(method, name, "Q", "O" if "O" in T.keywords(method) else "dQ")
        both = {"Q": x, ("O" if "O" in T.keywords(method) else "dQ"): y}
        assert T.outcome(A, reached, method, dict(T.base(method, name), **both)) == want and not reached, method
        A.close()


def test_the_two_spellings_of_a_shared_storage():
    """every two tensor arguments of a call as views of one storage: inputs (``work`` among them) may share among themselves; an
    output among the operands is rejected in ``OPERAND_SPELLING`` naming the argument that comes earlier in the call; a per-entry
    output (dS, dB) is judged before the operands, against everything, in ``ENTRY_SPELLING``"""
    name = "6x4"
    for method in METHODS:
        A, reached = T.make_handle(method, name)
        full = T.base(method, name)
        order = [a for a in full if a not in T.NUMBERS]
        # the order of judgement among the operands: inputs, then outputs in the order of the call, then work, then B and a
        rank = {a: i for i, a in enumerate([a for a in order if a in T.OPERANDS] + ["work", "B", "a", "slopes"])}
        for x, y in itertools.combinations(order, 2):
            tx, ty = T.shared(method, name, x, y)
            text = T.outcome(A, reached, method, dict(full, **{x: tx, y: ty}))
            entry = [a for a in (x, y) if a in ("dS", "dB") and not set((x, y)) & set(NEVER_COMPARED)]
            outs = [a for a in (x, y) if a in T.OUTPUTS and not set((x, y)) & set(NEVER_COMPARED)]
            if entry:
                other = y if entry[0] == x else x
                assert text == "ValueError: " + ENTRY_SPELLING.format(who=method, out=entry[0], other=other), (method, x, y, text)
            elif outs:
                out = max(outs, key=rank.get) if len(outs) == 2 else outs[0]
                other = y if out == x else x
                assert text == "ValueError: " + OPERAND_SPELLING.format(who=method, out=out, other=other), (method, x, y, text)
            else:
                assert text.startswith("-> ("), (method, x, y, text)
            assert text.startswith("-> (") or not reached, (method, x, y)
        A.close()


def _expected(method, name, kw):
    """the positional arguments the ``*_ptr`` method should get for the good call ``kw``, from the table and the tensors' strides"""
    m, n, nnz, heads, k, d = T.HANDLES[name]
    heads = heads if METHODS[method][1] == 3 else 1
    out = []
    for a in METHODS[method][2]:
        if a in LD:
            t = kw.get(LD[a])
            row = heads if LD[a] in T.ENTRY else heads * (k if T.OPERANDS[LD[a]][1] == "k" else d)
            out.append(max(t.stride(0), row) if t is not None and t.shape[0] > 1 and row else row)
        elif a in T.NUMBERS:
            out.append(float(kw.get(a, 1.0 if a == "scale" else 0.2)))
        else:
            out.append({"heads": heads, "k": k, "d": d, "type": _capi.BF16}[a] if a in ("heads", "k", "d", "type") else kw.get(a))
    return out


@pytest.mark.parametrize("name", list(T.HANDLES))
def test_a_good_call_reaches_the_library_with_the_expected_arguments(name):
    """contiguous tensors, row slices of wider operands, column slices of wider (nnz, H) tensors, each output None in turn and all
    of them: the tensors as given, the sizes, the numbers as floats, and for every tensor its leading dimension -- stride(0) where
    it has more than one row, the packed width otherwise and for an output that is None"""
    for method in METHODS:
        A, reached = T.make_handle(method, name)
        count = 0
        for label, kw in T.good_calls(method, name):
            text = T.outcome(A, reached, method, kw)
            if T.HANDLES[name][2] is None:
                assert text == f"ValueError: {method}: call inputCSR first" and not reached, (method, label, text)
                continue
            assert text.startswith("-> ("), (method, label, text)
            got, want = list(reached[0][1]), _expected(method, name, kw)
            assert len(got) == len(want), (method, label)
            for a, g, w in zip(METHODS[method][2], got, want):
                assert (g is w) if hasattr(w, "data_ptr") else (type(g) is type(w) and g == w), (name, method, label, a, g, w)
            count += 1
        assert count >= 3 or T.HANDLES[name][2] is None
        A.close()
    if name == "6x4":  # the figures of the padded gatBackward call: a [:, :2] slice of a (6, 4, 3) tensor, a [:, :2] of a (7, 5) one
        A, reached = T.make_handle("gatBackward", name)
        kw = dict(T.good_calls("gatBackward", name))["good slices"]
        T.outcome(A, reached, "gatBackward", dict(kw, dK=None))
        got = dict(zip(METHODS["gatBackward"][2], reached[0][1]))
        assert (got["lddq"], got["ldb"], got["lddb"], got["lddk"], got["ldv"], got["lddar"]) == (12, 5, 5, 6, 20, 12)
        A.close()
