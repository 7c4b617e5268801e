"""The cut rule of the range kernel (csrc/csr5_range_cut.h) without a GPU: scripts/host_emulation/range_cut_main.cpp -- plain host code, its own
main -- is compiled with g++ -fsanitize=address,undefined and run as a stand-alone program on the cases below; every line it prints is compared
with cuts computed HERE, from the rule as the header's comment states it (linear scans over Python integers, no bisection, no 64-bit limits):

  E[i] = cost of tiles 0 .. i-1.  Workgroup boundary g = 0 .. 32 is the first tile i with E[i] >= ceil(g W / 32); inside the span [b_g, b_g+1)
  of cost V, wavefront boundary j is the first tile i of the span with E[i] - E[b_g] >= ceil(V cum_j / cum_8); the first boundary of a span is
  its first tile, the last its end; so the first of a slab is 0 and the last is n.  Every case runs a second time with the workgroups' spans
  cut by tile count (boundary g = tile ceil(g n / 32): the rule with every tile costing 1), which is what the library uses.

Uniform costs are also held against the formula the kernel used before the table (equal tile counts per workgroup, 1085 / 915 per mille inside
it), restated below.  For n = 0, 1, 255, 256, 257 every boundary lies within one tile of it: the workgroup boundaries g q + min(g, n % 32) and
ceil(g n / 32) coincide for these n, and inside a span the rule rounds sz cum / 8000 up where the formula rounded down.  For other n the formula
gave its n % 32 spare tiles to the FIRST workgroups and the rule spreads them, so positions drift by up to n % 32 - ceil(.) < 32 tiles while a
range's SIZE -- (q or q + 1) x share, rounded either way in both -- stays within two tiles (less than 1 + 1 + 0.136)."""
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_SLOTS = [1085] * 4 + [915] * 4
WGS, WAVES = 32, 8


def ceil_div(a, b):
    return -((-a) // b)


def rule_cuts(costs, slots, by_count=False):
    n = len(costs)
    E = [0]
    for c in costs:
        E.append(E[-1] + c)
    W = E[n]

    def first(lo, hi, level):
        for i in range(lo, hi + 1):
            if E[i] >= level:
                return i
        return hi

    wg = [0] + [ceil_div(g * n, WGS) if by_count else first(0, n, ceil_div(g * W, WGS)) for g in range(1, WGS)] + [n]
    total = sum(slots)
    cuts = []
    for g in range(WGS):
        b0, b1 = wg[g], wg[g + 1]
        V = E[b1] - E[b0]
        cuts.append(b0)
        for j in range(1, WAVES):
            share = ceil_div(V * sum(slots[:j]), total) if total else 0
            cuts.append(first(b0, b1, E[b0] + share))
    return cuts + [n]


def formula_before_the_table(n, rho):
    """hot_range_begin of the parent commit, skew 85 per mille"""
    wg, j = divmod(rho, WAVES)
    if wg >= WGS:
        return n
    q, rem = divmod(n, WGS)
    wb, sz = wg * q + min(wg, rem), q + (1 if wg < rem else 0)
    cum = j * 1085 if j <= 4 else 4 * 1085 + (j - 4) * 915
    return wb + sz * cum // 8000


def build_cases():
    rnd = random.Random(7)
    cases = {}
    for n in (0, 1, 255, 256, 257):
        cases[f"uniform/n{n}"] = (0, DEFAULT_SLOTS, [1000] * n)
        cases[f"uniform_cost1/n{n}"] = (0, DEFAULT_SLOTS, [1] * n)
    for n in (528, 4099, 32781):
        cases[f"uniform/n{n}"] = (0, DEFAULT_SLOTS, [1537] * n)
    for n, at in ((1, 0), (257, 100), (257, 256), (1000, 0), (1000, 999)):
        cases[f"one_tile/n{n}_at{at}"] = (0, DEFAULT_SLOTS, [10 ** 6 if t == at else 0 for t in range(n)])
    for n in (255, 256, 1000):
        cases[f"first_half/n{n}"] = (0, DEFAULT_SLOTS, [1000 if t < n // 2 else 0 for t in range(n)])
    cases["all_zero/n300"] = (0, DEFAULT_SLOTS, [0] * 300)
    cases["beyond_2^32/n600"] = (0, DEFAULT_SLOTS, [rnd.randrange(1 << 24, 1 << 26) for _ in range(600)])
    cases["beyond_2^32/base_2^40"] = (1 << 40, DEFAULT_SLOTS, [rnd.randrange(1 << 24, 1 << 26) for _ in range(3000)])
    cases["beyond_2^32/n40000_tile_costs"] = (123456789012, DEFAULT_SLOTS, [1000 + 5 * rnd.randrange(0, 513) + 2 * rnd.randrange(0, 513) + (1 << 20) for _ in range(40000)])
    cases["zero_slot/second"] = (0, [1085, 0, 1085, 1085, 915, 915, 915, 2000], [rnd.randrange(900, 4000) for _ in range(5000)])
    cases["zero_slot/first_and_last"] = (0, [0, 1000, 1000, 1000, 1000, 1000, 1000, 0], [rnd.randrange(900, 4000) for _ in range(700)])
    cases["zero_slot/all"] = (0, [0] * 8, [rnd.randrange(900, 4000) for _ in range(700)])
    cases["random/default_slots"] = (99, DEFAULT_SLOTS, [1000 + 5 * rnd.randrange(0, 513) + rnd.randrange(0, 513) for _ in range(20000)])
    cases["random/skewed"] = (0, DEFAULT_SLOTS, [rnd.choice((1000, 1000, 1000, 3560, 1000 + 5 * 512 + 2 * 512)) for _ in range(3001)])
    cases["random/fewer_tiles_than_ranges"] = (0, DEFAULT_SLOTS, [rnd.randrange(1000, 4000) for _ in range(77)])
    return cases


CASES = build_cases()


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("range_cut") / "range_cut")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           f"-I{ROOT}/benchmark_spmv_using_csr5_amd/csrc", f"-I{ROOT}/include",
           os.path.join(ROOT, "scripts", "host_emulation", "range_cut_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = "".join(f"{pre}{name} {by_count} {base} {' '.join(map(str, slots))} {len(costs)} {' '.join(map(str, costs))}\n"
                   for pre, by_count in (("", 0), ("by_count/", 1)) for name, (base, slots, costs) in CASES.items())
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr  # (the sanitizers abort on a finding)
    return dict(line.split(": ", 1) for line in r.stdout.splitlines())


def test_every_case_is_printed(printed):
    assert [k for k in printed if k != "constants" and not k.startswith("cost/")] == list(CASES) + ["by_count/" + k for k in CASES]


@pytest.mark.parametrize("by_count", (False, True), ids=("spans_by_cost", "spans_by_count"))
@pytest.mark.parametrize("name", list(CASES))
def test_cuts_follow_the_rule(printed, name, by_count):
    base, slots, costs = CASES[name]
    got = [int(w) for w in printed[("by_count/" if by_count else "") + name].split()]
    assert len(got) == WGS * WAVES + 1
    assert got[0] == 0 and got[-1] == len(costs)
    assert all(a <= b for a, b in zip(got, got[1:]))
    assert got == rule_cuts(costs, slots, by_count)


@pytest.mark.parametrize("n", (0, 1, 255, 256, 257))
@pytest.mark.parametrize("kind", ("uniform", "uniform_cost1", "by_count/uniform"))
def test_uniform_cost_lands_within_one_tile_of_the_formula_before(printed, kind, n):
    got = [int(w) for w in printed[f"{kind}/n{n}"].split()]
    for rho, b in enumerate(got):
        assert abs(b - formula_before_the_table(n, rho)) <= 1, (rho, b)


@pytest.mark.parametrize("n", (528, 4099, 32781))
def test_uniform_cost_keeps_the_range_sizes_of_the_formula_before(printed, n):
    got = [int(w) for w in printed[f"uniform/n{n}"].split()]
    for rho in range(WGS * WAVES):
        before = formula_before_the_table(n, rho + 1) - formula_before_the_table(n, rho)
        assert abs((got[rho + 1] - got[rho]) - before) <= 2, rho


def test_where_the_cost_is_decides_where_the_ranges_are(printed):
    """all cost in one tile: that tile is a range of its own end, everything behind it goes to the last range; cost in the first half only: no
    range but the last holds a tile of the second half"""
    got = [int(w) for w in printed["one_tile/n257_at100"].split()]
    assert got[1] == 101 and got[-2] == 101  # the first boundary that must reach any cost lies behind tile 100
    for n in (255, 256, 1000):
        got = [int(w) for w in printed[f"first_half/n{n}"].split()]
        assert got[-2] <= n // 2 and got[-1] == n
    assert set(int(w) for w in printed["all_zero/n300"].split()[:-1]) == {0}


def test_a_zero_factor_gives_an_empty_range(printed):
    got = [int(w) for w in printed["zero_slot/second"].split()]
    assert all(got[8 * g + 1] == got[8 * g + 2] for g in range(WGS))
    got = [int(w) for w in printed["zero_slot/first_and_last"].split()]
    assert all(got[8 * g] == got[8 * g + 1] for g in range(WGS))


def test_constants_and_tile_cost(printed):
    """the default slot factors are the skew the kernel had before (1085 x 4, 915 x 4); a tile of T elements costs A T + B min(cold, T / 2) +
    C starts, and that is positive whatever the tile holds (B may be negative: profiles/r07_range_cost.md)"""
    words = [int(w) for w in printed["constants"].split()]
    A, B, C = words[1:4]
    assert words[0] == 1 and words[4:] == DEFAULT_SLOTS
    assert A > 0 and C >= 0 and 2 * A + B > 0
    probes = [k for k in printed if k.startswith("cost/")]
    assert len(probes) == 8
    for k in probes:
        T, cold, starts = (int(w) for w in k[5:].split("_"))
        assert int(printed[k]) == A * T + B * min(cold, T // 2) + C * starts > 0, k


def test_the_cut_header_needs_no_hip():
    with open(os.path.join(ROOT, "benchmark_spmv_using_csr5_amd", "csrc", "csr5_range_cut.h")) as f:
        includes = [line.split()[1] for line in f if line.startswith("#include")]
    assert includes == ["<cstdint>"]
