// blockmean_core_check.cpp — the split of the averaged spectrogram (csrc/sp_blockmean_core.h) and the exact-sum core
// (csrc/sp_exact_sum.h) alone, under the host compiler: tests/test_blockmean_cpu.py builds this with -fsanitize=address,undefined and
// compares what it prints with tests/blockmeanref.py.  It walks a plane as the device does: runs of random lengths, in order; every run
// split into head, body and tail; the columns of a direct body through an Accumulator per row of their own, as k_blockmean's LDS cells
// are; everything carried through ONE persistent Accumulator per row, cleared where a column begins and finished where it ends, as the
// context's workspace is.
// stdin: per plane one line "n width group direct_max seed" and one line of width * n hexadecimal 64-bit patterns, frame-major.
// stdout: per plane one line of columns * n patterns, frame-major; "mismatch" in place of it where the walk and the plain loop - an
// Accumulator per column and row, frame by frame - disagree; "broken split" where the parts of a run do not add up.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sp_blockmean_core.h"
#include "sp_exact_sum.h"

namespace {

uint64_t quotient(uint64_t sum_bits, int64_t count)
{
    double s;
    memcpy(&s, &sum_bits, sizeof s);
    const double q = s / (double)count;
    uint64_t r;
    memcpy(&r, &q, sizeof r);
    return r;
}

struct Walk {
    int64_t n, width, group, direct_max;
    const std::vector<uint64_t> &plane;
    std::vector<uint64_t> out;
    std::vector<spx::Accumulator> carried;   // one per row: the workspace
    bool broken = false;

    Walk(int64_t n_, int64_t width_, int64_t group_, int64_t direct_max_, const std::vector<uint64_t> &plane_)
        : n(n_), width(width_), group(group_), direct_max(direct_max_), plane(plane_), out((size_t)(spbm::columns(width_, group_) * n_), 0),
          carried((size_t)n_)
    {
    }

    // frames [x0, x0 + frames) of one column, carried
    void carry(int64_t x0, int64_t frames)
    {
        const int64_t c = x0 / group, first = c * group, end = first + group < width ? first + group : width;
        if (x0 + frames > end) broken = true;
        if (x0 == first)
            for (auto &a : carried) a = spx::Accumulator();
        for (int64_t x = x0; x < x0 + frames; x++)
            for (int64_t y = 0; y < n; y++) carried[(size_t)y].add(plane[(size_t)(x * n + y)]);
        if (x0 + frames == end)
            for (int64_t y = 0; y < n; y++) out[(size_t)(c * n + y)] = quotient(carried[(size_t)y].finish(), end - first);
    }

    void run(int64_t x_base, int64_t frames)
    {
        const spbm::Split s = spbm::split(x_base, frames, width, group, direct_max);
        if (s.head < 0 || s.body < 0 || s.tail < 0 || s.head + s.body + s.tail != frames) broken = true;
        if (broken) return;
        if (s.head) carry(x_base, s.head);
        const int64_t body_x = x_base + s.head;
        if (s.body && (body_x % group != 0 || s.body_column != body_x / group)) broken = true;
        for (int64_t k = 0; k < s.body_columns && !broken; k++) {
            const int64_t at = k * group, count = s.body - at < group ? s.body - at : group;
            if (count < 1) {
                broken = true;
            } else if (s.direct) {
                const int64_t c = s.body_column + k;
                for (int64_t y = 0; y < n; y++) {
                    spx::Accumulator cells;
                    for (int64_t x = body_x + at; x < body_x + at + count; x++) cells.add(plane[(size_t)(x * n + y)]);
                    out[(size_t)(c * n + y)] = quotient(cells.finish(), count);
                }
            } else {
                carry(body_x + at, count);
            }
        }
        if (s.tail && !broken) carry(body_x + s.body, s.tail);
    }
};

}  // namespace

int main()
{
    long long n, width, group, direct_max;
    unsigned long long seed;
    while (scanf("%lld %lld %lld %lld %llu", &n, &width, &group, &direct_max, &seed) == 5) {
        if (n < 1 || width < 0 || group < 1) return 2;
        std::vector<uint64_t> plane((size_t)(width * n));
        for (auto &v : plane)
            if (scanf("%" SCNx64, &v) != 1) return 2;

        Walk w(n, width, group, direct_max, plane);
        uint64_t state = seed * 6364136223846793005ull + 1442695040888963407ull;
        for (int64_t x = 0; x < width && !w.broken;) {
            state = state * 6364136223846793005ull + 1442695040888963407ull;
            int64_t frames = 1 + (int64_t)((state >> 33) % 17);
            if (frames > width - x) frames = width - x;
            w.run(x, frames);
            x += frames;
        }
        if (w.broken) {
            printf("broken split\n");
            continue;
        }
        // the plain loop
        bool same = true;
        const int64_t columns = spbm::columns(width, group);
        for (int64_t c = 0; c < columns && same; c++) {
            const int64_t first = c * group, end = first + group < width ? first + group : width;
            for (int64_t y = 0; y < n && same; y++) {
                spx::Accumulator a;
                for (int64_t x = first; x < end; x++) a.add(plane[(size_t)(x * n + y)]);
                same = quotient(a.finish(), end - first) == w.out[(size_t)(c * n + y)];
            }
        }
        if (!same) {
            printf("mismatch\n");
            continue;
        }
        for (size_t k = 0; k < w.out.size(); k++) printf("%s%016" PRIx64, k ? " " : "", w.out[k]);
        printf("\n");
    }
    return 0;
}
