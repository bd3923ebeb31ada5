// lagcov_core_check.cpp — csrc/sp_lagcov_core.h over csrc/sp_variance_core.h and csrc/sp_exact_sum.h with the host compiler alone, for
// the sanitizers (tests/test_lagcov_cpu.py builds this with -fsanitize=address,undefined).  Lines on stdin:
//     pair <width> <lags> <bits of a> ... <bits of b> ...        two series of `width` values as hexadecimal bit patterns
// and per line on stdout the 3 * lags results as hexadecimal bit patterns, out[0][..], out[1][..], out[2][..], or "refused".  Every lag
// is also accumulated with its terms in the reverse order and split across two accumulators that are merged cell by cell: integer adds
// commute, so the bits must be the same - exit status 3 where they are not, or where a term's five pieces do not put its 128-bit
// product and shift back together.  (Negative and zero differences pass through the finish with the lines the test sends.)
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "sp_lagcov_core.h"

static uint64_t mantissa(uint64_t bits, uint32_t &e1)
{
    const uint32_t e = (uint32_t)(bits >> 52) & 0x7ffu;
    e1 = e ? e - 1 : 0;
    return e ? (bits & 0x000fffffffffffffull) | (1ull << 52) : bits & 0x000fffffffffffffull;
}

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string kind;
        long long width = -1, lags = 0;
        in >> kind >> width >> lags;
        if (!in || kind != "pair" || width < 0 || width > (1 << 20) || lags < -1 || lags > (1 << 20)) {
            std::fprintf(stderr, "bad line: %.60s\n", line.c_str());
            return 2;
        }
        std::vector<uint64_t> a((size_t)width, 0), b((size_t)width, 0);
        in >> std::hex;
        for (auto &v : a) in >> v;
        for (auto &v : b) in >> v;
        if (in.fail()) {
            std::fprintf(stderr, "short line: %.60s\n", line.c_str());
            return 2;
        }
        std::vector<uint64_t> out(lags > 0 ? 3 * (size_t)lags : 0, 0);
        if (!spl::lagcov_bits(a.data(), b.data(), width, lags, out.data())) {
            std::puts("refused");
            continue;
        }
        for (size_t k = 0; k < out.size(); k++) std::printf("%016" PRIx64 "%c", out[k], k + 1 == out.size() ? '\n' : ' ');

        const long long n = spl::terms(width, lags);
        for (long long l = 0; l < lags; l++) {
            const uint64_t want[3] = {out[(size_t)l], out[(size_t)(lags + l)], out[(size_t)(2 * lags + l)]};
            uint64_t other[3];
            // the reverse order, and two accumulators - the even and the odd terms, then the first third and the rest - merged cell-wise
            spl::Accumulator back;
            for (long long x = n; x-- > 0;) back.add(a[(size_t)x], b[(size_t)(x + l)]);
            back.finish(other);
            if (std::memcmp(want, other, sizeof want) != 0) {
                std::fprintf(stderr, "the reverse order differs at lag %lld: %.60s\n", l, line.c_str());
                return 3;
            }
            for (int split = 0; split < 2; split++) {
                spl::Accumulator p, q;
                for (long long x = 0; x < n; x++) ((split ? x < n / 3 : (x & 1) == 0) ? p : q).add(a[(size_t)x], b[(size_t)(x + l)]);
                q.merge(p);
                q.finish(other);
                if (std::memcmp(want, other, sizeof want) != 0) {
                    std::fprintf(stderr, "two accumulators differ (split %d) at lag %lld: %.60s\n", split, l, line.c_str());
                    return 3;
                }
            }
            // the pieces themselves, on every term: they put ma * mb << ((ea1 + eb1) % 32) back together in the cell (ea1 + eb1) / 32
            for (long long x = 0; x < n; x++) {
                int cell;
                uint32_t p[5];
                if (spl::decompose_product(a[(size_t)x], b[(size_t)(x + l)], cell, p) != spx::kFinite) continue;
                uint32_t ea1, eb1;
                const uint64_t ma = mantissa(a[(size_t)x], ea1), mb = mantissa(b[(size_t)(x + l)], eb1);
                const uint32_t e2 = ea1 + eb1, s = e2 & 31u;
                const unsigned __int128 prod = (unsigned __int128)ma * mb;
                const unsigned __int128 low = prod << s;                               // the low 128 bits of the 137
                const uint64_t high = s ? (uint64_t)(prod >> (128 - s)) : 0;           // ... and what passes them
                const unsigned __int128 got =
                    ((unsigned __int128)p[3] << 96) | ((unsigned __int128)p[2] << 64) | ((unsigned __int128)p[1] << 32) | p[0];
                if (low != got || high != p[4] || cell != (int)(e2 >> 5) || cell + 4 >= spv::kSquareCells) {
                    std::fprintf(stderr, "pieces differ from the product at term %lld, lag %lld\n", x, l);
                    return 3;
                }
            }
        }
    }
    return 0;
}
