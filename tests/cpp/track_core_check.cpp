// track_core_check.cpp — the comparison of the peak track (csrc/sp_track_core.h) alone, under the host compiler: tests/test_track_cpu.py
// builds this with -fsanitize=address,undefined and compares what it prints with tests/trackref.py.
// stdin, one frame per line:   <y0> <y1> <n> <v0> <v1> ...    (n bit patterns of doubles, 16 hexadecimal digits each)
// stdout, per line:            <row> <the peak's bit pattern, 16 hexadecimal digits>
// The frame is folded twice - ascending, as sp_debug_band_peak does, and as the kernel does: 64 running bests, lane l over the rows
// y0 + l, y0 + l + 64, ..., merged as a butterfly - and the two must agree.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "sp_track_core.h"

static spt::Best as_the_wave_does(const uint64_t *bits, int32_t y0, int32_t y1)
{
    spt::Best lane[64];
    for (int l = 0; l < 64; l++)
        for (int64_t y = (int64_t)y0 + l; y < y1; y += 64) spt::fold(lane[l], spt::key_of(bits[y]), (int32_t)y);
    for (int step = 1; step < 64; step *= 2) {
        spt::Best next[64];
        for (int l = 0; l < 64; l++) {
            next[l] = lane[l];
            spt::merge(next[l], lane[l ^ step].key, lane[l ^ step].row);
        }
        for (int l = 0; l < 64; l++) lane[l] = next[l];
    }
    for (int l = 1; l < 64; l++)
        if (lane[l].key != lane[0].key || lane[l].row != lane[0].row) return spt::Best{~0ull, -2};   // (the lanes disagree)
    return lane[0];
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
        std::vector<uint64_t> bits;   // exactly n values on the heap: a read past them is the sanitizer's to find
        for (long k = 0; k < n; k++) bits.push_back((uint64_t)strtoull(end, &end, 16));
        const spt::Best a = spt::band_peak(bits.data(), y0, y1), b = as_the_wave_does(bits.data(), y0, y1);
        if (a.key != b.key || a.row != b.row) printf("orders disagree: ");
        printf("%d %016" PRIx64 "\n", (int)spt::row_of(a), spt::peak_bits_of(a));
        line.clear();
        if (c == EOF) break;
    }
    return 0;
}
