"""The decisions of the column-slab build (csrc/csr5_slab_plan.h) without a GPU: scripts/host_emulation/slab_plan_main.cpp -- plain host code, its
own main -- is compiled with g++ -fsanitize=address,undefined, run as a stand-alone program, and every line it prints is compared with a literal.

Where the literals come from: they were recorded from the function bodies the rules had BEFORE they moved into csr5_slab_plan.h -- slab_count_for,
slab_count_without_table and the blocks of build_slabs_impl in csr5_capi.hip, lifted verbatim into a throw-away program that ran the same case
table -- so they pin the behaviour the library had before the split, not what the new header happens to give.

The cases: every gate of the auto rule with its neighbour; the size classes of x for fp64 and fp32, before and after the halving loop; the count
without the table; what rules the table out beforehand; the rule after the column sample, with ADVICE.md's coverage cliff (28 % of 100 M non-zeros
covered and no structure at all: pinned as it is, the finding is still open); the sample's stride and threshold; the layout of the temporaries'
arena; the memory estimate against its cap; the dealing of slabs onto XCDs."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EXPECTED = """\
gate/base: by_x=8 count=8
gate/child: by_x=8 count=0
gate/request0: by_x=8 count=0
gate/p1_forced: by_x=8 count=0
gate/p2_forced: by_x=8 count=2
gate/nnz0_forced: by_x=8 count=0
gate/nnz1_forced: by_x=8 count=2
gate/x_under_4MiB_f64: by_x=8 count=0
gate/x_4MiB_f64: by_x=8 count=8
gate/x_one_byte_under_4MiB: by_x=8 count=0
gate/x_4MiB_bytes: by_x=8 count=8
gate/p511: by_x=8 count=0
gate/p512: by_x=8 count=8
gate/window50: by_x=8 count=0
gate/window49: by_x=8 count=8
size/f64_x8MB: by_x=8 count=8
size/f64_x33MB: by_x=8 count=8
size/f64_x134MB: by_x=16 count=16
size/f64_x268MB: by_x=32 count=32
size/f64_x536MB: by_x=32 count=32
size/f32_x8MB: by_x=8 count=8
size/f32_x33MB: by_x=8 count=8
size/f32_x134MB: by_x=16 count=16
size/f32_x268MB: by_x=32 count=32
size/f32_x536MB: by_x=32 count=32
size/halves_twice: by_x=32 count=8
size/stops_at_8: by_x=16 count=8
size/halves_once: by_x=32 count=16
plain/x1MiB: S=2
plain/x4MiB: S=2
plain/x8MiB: S=4
plain/x32MiB: S=16
plain/x64MiB: S=16
table/base_auto: S=8 S_plain=4 S_alloc=8 bits_s=3 bits_alloc=3 auto=1 hot=1 hot_sigma=8 hot_T=512 hot_p=32768 capacity=16384 stride=4 min_count=4
table/forced8: S=8 S_plain=8 S_alloc=8 bits_s=3 bits_alloc=3 auto=0 hot=1 hot_sigma=8 hot_T=512 hot_p=32768 capacity=16384 stride=4 min_count=4
table/S4_not_multiple_of_8: S=4 S_plain=4 S_alloc=4 bits_s=2 bits_alloc=2 auto=0 hot=0 hot_sigma=8 hot_T=512 hot_p=32768 capacity=0 stride=1 min_count=0
table/mode0_auto: S=4 S_plain=4 S_alloc=4 bits_s=3 bits_alloc=2 auto=1 hot=0 hot_sigma=8 hot_T=512 hot_p=32768 capacity=0 stride=1 min_count=0
table/mode0_forced16: S=16 S_plain=16 S_alloc=16 bits_s=4 bits_alloc=4 auto=0 hot=0 hot_sigma=8 hot_T=512 hot_p=32768 capacity=0 stride=1 min_count=0
table/hot_request0: S=4 S_plain=4 S_alloc=4 bits_s=3 bits_alloc=2 auto=1 hot=0 hot_sigma=8 hot_T=512 hot_p=32768 capacity=0 stride=1 min_count=0
table/hot_p1: S=8 S_plain=8 S_alloc=8 bits_s=3 bits_alloc=3 auto=0 hot=0 hot_sigma=8 hot_T=512 hot_p=1 capacity=0 stride=1 min_count=0
table/hot_p2: S=8 S_plain=8 S_alloc=8 bits_s=3 bits_alloc=3 auto=0 hot=1 hot_sigma=8 hot_T=512 hot_p=2 capacity=16384 stride=1 min_count=16
table/lds_1023_slots: S=4 S_plain=4 S_alloc=4 bits_s=3 bits_alloc=2 auto=1 hot=0 hot_sigma=8 hot_T=512 hot_p=32768 capacity=0 stride=1 min_count=0
table/lds_1024_slots: S=8 S_plain=4 S_alloc=8 bits_s=3 bits_alloc=3 auto=1 hot=1 hot_sigma=8 hot_T=512 hot_p=32768 capacity=1024 stride=4 min_count=4
table/lds_64KiB: S=8 S_plain=4 S_alloc=8 bits_s=3 bits_alloc=3 auto=1 hot=1 hot_sigma=8 hot_T=512 hot_p=32768 capacity=4096 stride=4 min_count=4
table/f32: S=8 S_plain=2 S_alloc=8 bits_s=3 bits_alloc=3 auto=1 hot=1 hot_sigma=16 hot_T=1024 hot_p=16384 capacity=32768 stride=4 min_count=4
table/local_columns_over_2^22: S=8 S_plain=8 S_alloc=8 bits_s=3 bits_alloc=3 auto=0 hot=0 hot_sigma=16 hot_T=1024 hot_p=16384 capacity=0 stride=1 min_count=0
table/local_columns_2^22: S=8 S_plain=8 S_alloc=8 bits_s=3 bits_alloc=3 auto=0 hot=1 hot_sigma=16 hot_T=1024 hot_p=16384 capacity=32768 stride=4 min_count=4
table/x_over_2GiB: S=8 S_plain=8 S_alloc=8 bits_s=3 bits_alloc=3 auto=0 hot=0 hot_sigma=8 hot_T=512 hot_p=32768 capacity=0 stride=1 min_count=0
table/rmat24_auto: S=16 S_plain=16 S_alloc=16 bits_s=4 bits_alloc=4 auto=1 hot=1 hot_sigma=8 hot_T=512 hot_p=524288 capacity=16384 stride=64 min_count=2
sample/100M_cover24: planned S=16 hot=1 cover=24 -> no_table S=16 bits=4
sample/100M_cover25: planned S=16 hot=1 cover=25 -> none S=0 bits=0
sample/100M_cover28: planned S=16 hot=1 cover=28 -> none S=0 bits=0
sample/100M_cover29: planned S=16 hot=1 cover=29 -> none S=0 bits=0
sample/100M_cover30: planned S=16 hot=1 cover=30 -> table S=16 bits=4
sample/25M_cover54: planned S=8 hot=1 cover=54 -> table S=8 bits=3
sample/25M_cover44: planned S=8 hot=1 cover=44 -> none S=0 bits=0
sample/25M_cover10_forced_table: planned S=8 hot=1 cover=10 -> table S=8 bits=3
sample/25M_cover10_forced_count: planned S=8 hot=1 cover=10 -> no_table S=8 bits=3
sample/25M_cover28_forced_count: planned S=8 hot=1 cover=28 -> no_table S=8 bits=3
sample/25M_cover54_forced_count: planned S=8 hot=1 cover=54 -> table S=8 bits=3
sample/25M_no_candidate: planned S=8 hot=0 cover=0 -> no_table S=8 bits=3
stride/nnz1000000: S=8 S_plain=8 S_alloc=8 bits_s=3 bits_alloc=3 auto=0 hot=1 hot_sigma=8 hot_T=512 hot_p=1954 capacity=16384 stride=1 min_count=16
stride/nnz4194304: S=8 S_plain=8 S_alloc=8 bits_s=3 bits_alloc=3 auto=0 hot=1 hot_sigma=8 hot_T=512 hot_p=8192 capacity=16384 stride=1 min_count=16
stride/nnz8388608: S=8 S_plain=8 S_alloc=8 bits_s=3 bits_alloc=3 auto=0 hot=1 hot_sigma=8 hot_T=512 hot_p=16384 capacity=16384 stride=2 min_count=8
stride/nnz67108864: S=8 S_plain=8 S_alloc=8 bits_s=3 bits_alloc=3 auto=0 hot=1 hot_sigma=8 hot_T=512 hot_p=131072 capacity=16384 stride=16 min_count=2
stride/nnz2147483647: S=8 S_plain=8 S_alloc=8 bits_s=3 bits_alloc=3 auto=0 hot=1 hot_sigma=8 hot_T=512 hot_p=4194304 capacity=16384 stride=64 min_count=2
cover/rmat24: stride=64 covered=3000000 -> 71 covered=5000000 -> 100
arena/table: hot=1 off 0+524288 524288+1031 525568+67108864 67634432+16 67634688+70001 67704832+4194304 71899136+144256 72043520+32768 72076288+64 72076544+1048576 73125120+4194304 77319424+4194304 81513728+4194304 85708032+4194304 89902336+12345 total=89914880 aligned=1 disjoint=1 covered_in_count=1 cold_empty=0
memory/table: hot=1 need=475291800 cap=454 fits=1 cap=453 fits=0
memory/table_narrow: hot=1 need=542400664 cap=518 fits=1 cap=517 fits=0
arena/no_table: hot=0 off 0+262144 262144+1031 263424+67108864 67372288+16 67372544+70001 67442688+4194304 71636992+72256 71709440+16384 71725824+32 71726080+0 71726080+0 71726080+0 71726080+0 71726080+0 71726080+0 total=71726080 aligned=1 disjoint=1 covered_in_count=1 cold_empty=1
memory/no_table: hot=0 need=332887672 cap=318 fits=1 cap=317 fits=0
arena/odd_f32: hot=1 off 0+187520 187648+1031 188928+12000068 12189184+16 12189440+70001 12259584+4000012 16259840+288256 16548096+65536 16613632+128 16613888+1000192 17614080+4000768 21614848+4000768 25615616+4000768 29616384+4000768 33617152+12345 total=33629696 aligned=1 disjoint=1 covered_in_count=1 cold_empty=0
memory/odd_f32: hot=1 need=107863072 cap=103 fits=1 cap=102 fits=0
deal/S8: order 2 4 6 0 5 1 7 3 permutation=1 per_xcd=1
deal/S16_rmat24: order 0 6 13 12 3 4 9 14 7 8 15 10 1 2 11 5 permutation=1 per_xcd=2
deal/S64_ties: order 3 35 2 34 1 33 0 32 7 39 6 38 5 37 4 36 11 43 10 42 9 41 8 40 15 47 14 46 13 45 12 44 19 51 18 50 17 49 16 48 23 55 22 54 21 53 20 52 27 59 26 58 25 57 24 56 31 63 30 62 29 61 28 60 permutation=1 per_xcd=8
"""


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("slab_plan") / "slab_plan")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           f"-I{ROOT}/benchmark_spmv_using_csr5_amd/csrc", f"-I{ROOT}/include",
           os.path.join(ROOT, "scripts", "host_emulation", "slab_plan_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr  # (the sanitizers abort on a finding)
    return dict(line.split(": ", 1) for line in r.stdout.splitlines())


CASES = dict(line.split(": ", 1) for line in EXPECTED.splitlines())


def test_the_program_prints_exactly_the_recorded_cases(printed):
    assert list(printed) == list(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_slab_plan_case(printed, name):
    assert printed[name] == CASES[name]


def test_the_plan_header_needs_no_hip():
    """csr5_slab_plan.h is plain C++: no HIP header, directly or through what it includes."""
    with open(os.path.join(ROOT, "benchmark_spmv_using_csr5_amd", "csrc", "csr5_slab_plan.h")) as f:
        includes = [line.split()[1] for line in f if line.startswith("#include")]
    assert includes == ["<algorithm>", "<cstddef>", "<cstdint>", "<vector>", '"csr5hip.h"']
    with open(os.path.join(ROOT, "include", "csr5hip.h")) as f:
        assert "hip/" not in "".join(line for line in f if line.startswith("#include"))


def test_properties_the_literals_must_have():
    """What the issue of the split asks of the table, read off the literals themselves."""
    field = lambda name, key: CASES[name].split(key + "=")[1].split()[0]
    for gate in ("child", "request0", "p1_forced", "nnz0_forced", "x_under_4MiB_f64", "x_one_byte_under_4MiB", "p511", "window50"):
        assert field("gate/" + gate, "count") == "0", gate
    for neighbour in ("base", "p2_forced", "nnz1_forced", "x_4MiB_f64", "x_4MiB_bytes", "p512", "window49"):
        assert field("gate/" + neighbour, "count") != "0", neighbour
    assert CASES["plain/x8MiB"] == "S=4"  # the webbase case
    assert CASES["sample/100M_cover28"].endswith("-> none S=0 bits=0")  # ADVICE.md's cliff, still open
    for name in CASES:
        if name.startswith("arena/"):
            assert "aligned=1 disjoint=1 covered_in_count=1" in CASES[name]
            assert field(name, "cold_empty") == ("0" if field(name, "hot") == "1" else "1")
        if name.startswith("memory/"):
            assert CASES[name].count("fits=1") == 1 and CASES[name].endswith("fits=0")
        if name.startswith("deal/"):
            assert "permutation=1" in CASES[name]
            S = int(name.split("/S")[1].split("_")[0])
            assert field(name, "per_xcd") == str(S // 8)
