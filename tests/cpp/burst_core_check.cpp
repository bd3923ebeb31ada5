// burst_core_check.cpp — csrc/sp_burst_core.h alone under the host compiler and its sanitizers (tests/test_bursts_cpu.py).  Every line of
// stdin is one series: "<hi bits> <lo bits> <max_bursts> <width> <value bits> ...", all in hex but the two numbers.  The series is
// scanned by the host loop (spb::scan) and, for segments of 64, 128 and SP_BURST_SEGMENT_FRAMES frames, as the kernels scan it: SET and
// RESET masks of 64-frame words, a Summary per segment, the exclusive combine scan 64 summaries a step by doubling as a wave's shuffles
// do it, and the emit with popcounts and the true carry.  All four must agree; the answer goes to stdout as "<count> <edges ...>".
// Before the first line combine() is checked for associativity, and against the masks' own scan, on all triples of small summaries.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>
#include <iostream>

#include "../../include/spectroplot_hip.h"
#include "sp_burst_core.h"

namespace {

[[noreturn]] void die(const char *what, size_t line)
{
    fprintf(stderr, "burst_core_check: %s (line %zu)\n", what, line);
    exit(1);
}

bool same(const spb::Summary &a, const spb::Summary &b) { return a.first == b.first && a.last == b.last && a.rises == b.rises; }

// a run of `len` <= 21 frames as base-3 digits of `code` (0 HOLD, 1 SET, 2 RESET) -> its masks
void masks_of(uint32_t code, int len, uint64_t &set, uint64_t &reset)
{
    set = reset = 0;
    for (int i = 0; i < len; i++, code /= 3) {
        if (code % 3 == spb::kSet) set |= 1ull << i;
        if (code % 3 == spb::kReset) reset |= 1ull << i;
    }
}

void check_algebra()
{
    // every run of 0 .. 3 frames: 1 + 3 + 9 + 27 = 40 summaries; all 64000 triples
    std::vector<spb::Summary> sums;
    std::vector<std::pair<uint32_t, int>> runs;
    for (int len = 0, pow = 1; len <= 3; len++, pow *= 3)
        for (uint32_t code = 0; code < (uint32_t)pow; code++) {
            uint64_t s, r;
            masks_of(code, len, s, r);
            sums.push_back(spb::word_summary(s, r));
            runs.push_back({code, len});
        }
    for (size_t a = 0; a < sums.size(); a++)
        for (size_t b = 0; b < sums.size(); b++) {
            const spb::Summary ab = spb::combine(sums[a], sums[b]);
            // against the masks of the run a followed by the run b
            uint64_t sa, ra, sb, rb;
            masks_of(runs[a].first, runs[a].second, sa, ra);
            masks_of(runs[b].first, runs[b].second, sb, rb);
            const spb::Summary direct = spb::word_summary(sa | sb << runs[a].second, ra | rb << runs[a].second);
            if (!same(ab, direct)) die("combine(a, b) is not the summary of a followed by b", a * 100 + b);
            for (uint32_t carry = 0; carry < 2; carry++) {
                const spb::Step st = spb::step(sa, ra, carry);
                const int len = runs[a].second;
                const uint32_t after = len ? (uint32_t)(st.on >> (len - 1) & 1) : carry;
                if (spb::rises_after(sums[a], carry) != spo::popcount(st.rises)) die("rises_after", a);
                if (spb::state_after(sums[a], carry) != after) die("state_after", a);
            }
            for (size_t c = 0; c < sums.size(); c++)
                if (!same(spb::combine(ab, sums[c]), spb::combine(sums[a], spb::combine(sums[b], sums[c])))) die("combine is not associative", c);
        }
    for (const spb::Summary &s : sums)
        if (!same(spb::unpack(spb::pack(s)), s)) die("pack", 0);
}

// as the three kernels do it, in segments of `seg` frames (a multiple of 64)
uint32_t scan_as_kernels(const std::vector<uint64_t> &bits, int32_t width, uint64_t hi_key, uint64_t lo_key, int32_t max_bursts, int32_t seg,
                         std::vector<int32_t> &edges)
{
    edges.assign(2 * (size_t)max_bursts, -1);
    const int32_t words = (width + 63) / 64, per = seg / 64, segments = (width + seg - 1) / seg;
    std::vector<uint64_t> set((size_t)words), reset((size_t)words);
    for (int32_t w = 0; w < words; w++)
        for (int lane = 0; lane < 64; lane++) {
            const int32_t x = w * 64 + lane;
            const int32_t at = x < width ? x : width - 1;          // a lane past the end re-reads the last frame and is masked
            const uint32_t c = spb::classify(bits[(size_t)at], hi_key, lo_key);
            if (x < width && c == spb::kSet) set[(size_t)w] |= 1ull << lane;
            if (x < width && c == spb::kReset) reset[(size_t)w] |= 1ull << lane;
        }
    auto word = [&](int32_t w, uint64_t &s, uint64_t &r) { s = w < words ? set[(size_t)w] : 0, r = w < words ? reset[(size_t)w] : 0; };
    // k_burst_summary
    std::vector<uint64_t> summaries((size_t)segments), carries((size_t)segments);
    for (int32_t g = 0; g < segments; g++) {
        spb::Summary sum;
        for (int32_t w = g * per; w < (g + 1) * per; w++) {
            uint64_t s, r;
            word(w, s, r);
            sum = spb::combine(sum, spb::word_summary(s, r));
        }
        summaries[(size_t)g] = spb::pack(sum);
    }
    // k_burst_carry
    spb::Summary run;
    for (int32_t g0 = 0; g0 < segments; g0 += 64) {
        spb::Summary incl[64];
        for (int lane = 0; lane < 64; lane++) incl[lane] = spb::unpack(g0 + lane < segments ? summaries[(size_t)(g0 + lane)] : 0ull);
        for (int d = 1; d < 64; d *= 2) {
            spb::Summary next[64];
            for (int lane = 0; lane < 64; lane++) next[lane] = lane >= d ? spb::combine(incl[lane - d], incl[lane]) : incl[lane];
            memcpy(incl, next, sizeof incl);
        }
        for (int lane = 0; lane < 64 && g0 + lane < segments; lane++) {
            const spb::Summary excl = lane == 0 ? run : spb::combine(run, incl[lane - 1]);
            carries[(size_t)(g0 + lane)] = (uint64_t)excl.rises | (uint64_t)spb::state_after(excl, 0) << 32;
        }
        run = spb::combine(run, incl[63]);
    }
    if (spb::state_after(run, 0) != 0 && run.rises - 1 < (uint32_t)max_bursts) edges[2 * (size_t)(run.rises - 1) + 1] = width;
    // k_burst_emit
    for (int32_t g = 0; g < segments && max_bursts > 0; g++) {
        uint32_t base = (uint32_t)carries[(size_t)g], state = (uint32_t)(carries[(size_t)g] >> 32) & 1u;
        for (int32_t w = g * per; w < (g + 1) * per; w++) {
            uint64_t s, r;
            word(w, s, r);
            const spb::Step st = spb::step(s, r, state);
            for (int lane = 0; lane < 64; lane++) {
                const uint32_t started = base + spo::popcount(st.rises & ((1ull << lane) - 1));
                const int32_t x = w * 64 + lane;
                if ((st.rises >> lane & 1) != 0 && started < (uint32_t)max_bursts) {
                    if (edges[2 * (size_t)started] != -1) die("a start slot has two writers", (size_t)x);
                    edges[2 * (size_t)started] = x;
                }
                if ((st.falls >> lane & 1) != 0 && started - 1 < (uint32_t)max_bursts) {
                    if (edges[2 * (size_t)(started - 1) + 1] != -1) die("an end slot has two writers", (size_t)x);
                    edges[2 * (size_t)(started - 1) + 1] = x;
                }
            }
            base += spo::popcount(st.rises);
            state = st.carry;
        }
    }
    return run.rises;
}

}  // namespace

int main()
{
    check_algebra();
    std::string text;
    size_t line = 0;
    while (std::getline(std::cin, text)) {
        line++;
        std::istringstream in(text);
        uint64_t hi_bits, lo_bits;
        int32_t max_bursts, width;
        in >> std::hex >> hi_bits >> lo_bits >> std::dec >> max_bursts >> width >> std::hex;
        if (!in || width < 0 || max_bursts < 0) die("bad line", line);
        std::vector<uint64_t> bits((size_t)width);
        for (int32_t x = 0; x < width; x++)
            if (!(in >> bits[(size_t)x])) die("short line", line);
        const uint64_t hi_key = spo::threshold_key(hi_bits), lo_key = spo::threshold_key(lo_bits);
        if (hi_key == spo::kNoHitKey || lo_key > hi_key) die("bad thresholds", line);
        std::vector<int32_t> want(2 * (size_t)max_bursts), got;
        const uint32_t total = spb::scan(bits.data(), width, hi_key, lo_key, max_bursts, want.data());
        for (int32_t seg : {64, 128, SP_BURST_SEGMENT_FRAMES}) {
            if (scan_as_kernels(bits, width, hi_key, lo_key, max_bursts, seg, got) != total) die("the kernels' count differs", line);
            if (got != want) die("the kernels' edges differ", line);
        }
        printf("%" PRIu32, total);
        for (int32_t e : want) printf(" %d", e);
        printf("\n");
    }
    return 0;
}
