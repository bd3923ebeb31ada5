// occupancy_core_check.cpp — the decision of the occupancy counts (csrc/sp_occupancy_core.h) alone, under the host compiler:
// tests/test_occupancy_cpu.py builds this with -fsanitize=address,undefined and compares what it prints with tests/occref.py.
// stdin, one frame per line:   <y0> <y1> <n> <v0> ... <v(n-1)> <t0> ... <t(n-1)>   (bit patterns of doubles, 16 hexadecimal digits each)
// stdout, per line:            <the hits among the rows [y0, y1)>
// The frame is counted twice - ascending, as sp_debug_occupancy does, and as the kernel does: the rows 64 at a time from row `first`
// on (the start of a tile), a lane past the end re-reading the last row and masked, the group's hits as one 64-bit ballot, and the
// band's share of it the popcount under spo::band_mask - for the band itself and for its two halves - and the counts must agree.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "sp_occupancy_core.h"

static uint32_t as_the_wave_does(const uint64_t *values, const uint64_t *thresholds, int32_t n, int32_t first, int32_t y0, int32_t y1)
{
    uint32_t count = 0;
    const int32_t last = n - 1;
    for (int32_t g = first; g < n; g += 64) {
        uint64_t ballot = 0;
        for (int32_t lane = 0; lane < 64; lane++) {
            const int32_t y = g + lane <= last ? g + lane : last;
            const uint64_t tkey = g + lane <= last ? spo::threshold_key(thresholds[y]) : spo::kNoHitKey;
            if (spo::hit(values[y], tkey)) ballot |= 1ull << lane;
        }
        count += spo::popcount(ballot & spo::band_mask(y0, y1, g));
    }
    return count;
}

int main()
{
    std::string line;
    for (int c = getchar();; c = getchar()) {
        if (c != '\n' && c != EOF) {
            line.push_back((char)c);
            continue;
        }
        if (c == EOF && line.empty()) break;
        char *end = nullptr;
        const int32_t y0 = (int32_t)strtol(line.c_str(), &end, 10);
        const int32_t y1 = (int32_t)strtol(end, &end, 10);
        const long n = strtol(end, &end, 10);
        std::vector<uint64_t> values, thresholds;   // exactly n each on the heap: a read past them is the sanitizer's to find
        for (long k = 0; k < n; k++) values.push_back((uint64_t)strtoull(end, &end, 16));
        for (long k = 0; k < n; k++) thresholds.push_back((uint64_t)strtoull(end, &end, 16));
        const uint32_t a = spo::band_count(values.data(), thresholds.data(), y0, y1);
        const int32_t mid = y0 + (y1 - y0) / 2;
        bool same = true;
        // (a tile that starts at row 0, and one that starts below the band at a row that is no multiple of 64: the rows in front of
        // it belong to another workgroup, so only a band that starts at or behind it is counted whole)
        for (const int32_t first : {0, y0 - y0 % 7}) {
            const uint32_t whole = as_the_wave_does(values.data(), thresholds.data(), (int32_t)n, first, y0, y1);
            const uint32_t halves = as_the_wave_does(values.data(), thresholds.data(), (int32_t)n, first, y0, mid) +
                                    as_the_wave_does(values.data(), thresholds.data(), (int32_t)n, first, mid, y1);
            same = same && whole == a && halves == a;
        }
        if (!same) printf("orders disagree: ");
        printf("%" PRIu32 "\n", a);
        line.clear();
        if (c == EOF) break;
    }
    return 0;
}
