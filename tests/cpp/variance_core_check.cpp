// variance_core_check.cpp — csrc/sp_variance_core.h over csrc/sp_exact_sum.h with the host compiler alone, for the sanitizers
// (tests/test_variance_cpu.py builds this with -fsanitize=address,undefined).  Lines on stdin:
//     row <count> <bits> ...          the `count` values of a row over its frames as hexadecimal bit patterns
// and per line on stdout the three results as hexadecimal bit patterns, or "refused".  Every row is also added in the reverse order and
// split across two accumulators that are merged cell by cell: integer adds commute, so the bits must be the same - exit status 3
// where they are not, or where a value's five pieces do not put its 128-bit square back together.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "sp_variance_core.h"

static bool same(const uint64_t a[3], const uint64_t b[3]) { return std::memcmp(a, b, 3 * sizeof(uint64_t)) == 0; }

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string kind;
        unsigned long long count = 0;
        in >> kind >> count;
        if (!in || kind != "row" || count > (1ull << 24)) {
            std::fprintf(stderr, "bad line: %.60s\n", line.c_str());
            return 2;
        }
        std::vector<uint64_t> bits((size_t)count, 0);
        in >> std::hex;
        for (auto &b : bits) in >> b;
        if (in.fail()) {
            std::fprintf(stderr, "short line: %.60s\n", line.c_str());
            return 2;
        }
        uint64_t out[3] = {};
        if (!spv::variance_sums_bits(bits.data(), bits.size(), out)) {
            std::puts("refused");
            continue;
        }
        std::printf("%016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", out[0], out[1], out[2]);

        // the reverse order, and two accumulators - the even and the odd frames, then the first third and the rest - merged cell-wise
        uint64_t other[3];
        spv::Accumulator back;
        for (size_t k = bits.size(); k-- > 0;) back.add(bits[k]);
        back.finish(other);
        if (!same(out, other)) {
            std::fprintf(stderr, "the reverse order differs: %.60s\n", line.c_str());
            return 3;
        }
        for (int split = 0; split < 2; split++) {
            spv::Accumulator a, b;
            for (size_t k = 0; k < bits.size(); k++) ((split ? k < bits.size() / 3 : (k & 1) == 0) ? a : b).add(bits[k]);
            b.merge(a);
            b.finish(other);
            if (!same(out, other)) {
                std::fprintf(stderr, "two accumulators differ (split %d): %.60s\n", split, line.c_str());
                return 3;
            }
        }

        // the pieces themselves, on every value: they put m^2 << (2 e1 % 32) back together in the cell (2 e1) / 32
        for (size_t k = 0; k < bits.size(); k++) {
            int cell;
            uint32_t p[5];
            if (spv::decompose_squared(bits[k], cell, p) != spx::kFinite) continue;
            const uint32_t e = (uint32_t)(bits[k] >> 52) & 0x7ffu;
            const uint64_t m = e ? (bits[k] & 0x000fffffffffffffull) | (1ull << 52) : bits[k] & 0x000fffffffffffffull;
            const uint32_t e2 = 2 * (e ? e - 1 : 0), s = e2 & 31u;
            const unsigned __int128 sq = (unsigned __int128)m * m;
            const unsigned __int128 low = sq << s;                               // the low 128 bits of the 136
            const uint64_t high = s ? (uint64_t)(sq >> (128 - s)) : 0;           // ... and what passes them
            const unsigned __int128 got = ((unsigned __int128)p[3] << 96) | ((unsigned __int128)p[2] << 64) | ((unsigned __int128)p[1] << 32) | p[0];
            if (low != got || high != p[4] || cell != (int)(e2 >> 5) || cell + 4 >= spv::kSquareCells) {
                std::fprintf(stderr, "pieces differ from the square at frame %zu\n", k);
                return 3;
            }
        }
    }
    return 0;
}
