// moment_core_check.cpp — csrc/sp_moment_core.h over csrc/sp_exact_sum.h with the host compiler alone, for the sanitizers
// (tests/test_moments_cpu.py builds this with -fsanitize=address,undefined).  Lines on stdin:
//     column <order> <count> <bits> ...          the `count` values of a column as hexadecimal bit patterns
//     sparse <order> <count> <row> <bits> ...    a column of `count` rows that is +0.0 but for the (row, bits) pairs that follow
// and per line on stdout the order + 1 moments as hexadecimal bit patterns, or "refused".  The weights are the rows 0 .. count - 1.
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "sp_moment_core.h"

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string kind;
        int order = 0;
        unsigned long long count = 0;
        in >> kind >> order >> count;
        if (!in || (kind != "column" && kind != "sparse") || count > (1ull << 24)) {
            std::fprintf(stderr, "bad line: %.60s\n", line.c_str());
            return 2;
        }
        std::vector<uint64_t> bits((size_t)count, 0);
        in >> std::hex;
        if (kind == "column") {
            for (auto &b : bits) in >> b;
        } else {
            unsigned long long row;
            uint64_t b;
            while (in >> std::dec >> row >> std::hex >> b) {
                if (row >= count) {
                    std::fprintf(stderr, "row %llu beyond the column\n", row);
                    return 2;
                }
                bits[(size_t)row] = b;
            }
            in.clear();
        }
        if (in.fail()) {
            std::fprintf(stderr, "short line: %.60s\n", line.c_str());
            return 2;
        }
        uint64_t out[spm::kMaxOrder + 1] = {};
        if (!spm::moment_sum_bits(bits.data(), bits.size(), order, out)) {
            std::puts("refused");
            continue;
        }
        for (int k = 0; k <= order; k++) std::printf("%s%016" PRIx64, k ? " " : "", out[k]);
        std::puts("");

        // the pieces themselves, on every value: they put (m * w) << s back together, and weight 1 gives spx::decompose's pieces
        for (size_t r = 0; r < bits.size(); r++) {
            if (!bits[r]) continue;
            int c3, c4;
            uint32_t p3[3], p4[4];
            const int k3 = spx::decompose(bits[r], c3, p3), k4 = spm::decompose_weighted(bits[r], 1, c4, p4);
            if (k3 != k4 || c3 != c4 || p3[0] != p4[0] || p3[1] != p4[1] || p3[2] != p4[2] || p4[3] != 0) {
                std::fprintf(stderr, "weight 1 differs from decompose at row %zu\n", r);
                return 3;
            }
            if (k4 != spx::kFinite) continue;
            const uint64_t w = spm::weight(r, 2);
            spm::decompose_weighted(bits[r], w, c4, p4);
            const uint32_t e = (uint32_t)(bits[r] >> 52) & 0x7ffu;
            const uint64_t m = e ? (bits[r] & 0x000fffffffffffffull) | (1ull << 52) : bits[r] & 0x000fffffffffffffull;
            const unsigned __int128 want = ((unsigned __int128)m * w) << ((e ? e - 1 : 0) & 31u);
            const unsigned __int128 got = ((unsigned __int128)p4[3] << 96) | ((unsigned __int128)p4[2] << 64) | ((unsigned __int128)p4[1] << 32) | p4[0];
            if (want != got || c4 != (int)((e ? e - 1 : 0) >> 5)) {
                std::fprintf(stderr, "pieces differ from the product at row %zu\n", r);
                return 3;
            }
        }
    }
    return 0;
}
