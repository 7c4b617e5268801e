// range_cut_main.cpp -- the cut rule of the range kernel (csrc/csr5_range_cut.h) as a stand-alone host program: plain g++, no HIP,
// its own main (tests/test_range_cut_host.py compiles it with -fsanitize=address,undefined and compares every line it prints with
// cuts the test computes itself from the rule).
//
// stdin, one case per line:   name by_count base s0 .. s7 n c0 .. c(n-1)
//   by_count = 1: the workgroups' spans are cut by tile count (what the library does), 0: by cost like the ranges inside them,
//   base = cost in front of the slab (the prefix array the library passes is one array for all slabs), s = slot factors,
//   n = tiles of the slab, c = their costs.
// stdout:  "constants: by_count A B C s0 .. s7", "cost/<T>_<cold>_<starts>: <cost>" for a few tiles, then per case "name: b0 .. b256".
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "csr5_range_cut.h"

int main()
{
    using namespace csr5;
    std::printf("constants: %d %d %d %d", RANGE_SPANS_BY_COUNT ? 1 : 0, RANGE_COST_A, RANGE_COST_B, RANGE_COST_C);
    for (int w = 0; w < CUT_WAVES; w++)
        std::printf(" %d", RANGE_SLOTS_DEFAULT.permil[w]);
    std::printf("\n");
    const int probe[][3] = {{512, 0, 0}, {512, 512, 0}, {512, 0, 512}, {512, 256, 3}, {512, 257, 3}, {1024, 1024, 1024}, {1024, 137, 41}, {1024, 512, 0}};
    for (const auto &pr : probe)
        std::printf("cost/%d_%d_%d: %llu\n", pr[0], pr[1], pr[2], (unsigned long long)range_tile_cost(pr[0], pr[1], pr[2]));
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty())
            continue;
        std::istringstream in(line);
        std::string name;
        unsigned long long base = 0;
        RangeSlots slots{};
        int n = 0, by_count = 0;
        in >> name >> by_count >> base;
        for (int w = 0; w < CUT_WAVES; w++)
            in >> slots.permil[w];
        in >> n;
        // exactly n + 1 words: a read past either end is the sanitizer's finding
        std::vector<uint64_t> E((size_t)n + 1);
        E[0] = base;
        for (int t = 0; t < n; t++) {
            unsigned long long c = 0;
            in >> c;
            E[(size_t)t + 1] = E[(size_t)t] + c;
        }
        if (!in) {
            std::fprintf(stderr, "bad case line: %s\n", name.c_str());
            return 2;
        }
        std::printf("%s:", name.c_str());
        for (int rho = 0; rho <= CUT_RANGES; rho++)
            std::printf(" %d", range_cut_begin(E.data(), n, rho, slots, by_count != 0));
        std::printf("\n");
    }
    return 0;
}
