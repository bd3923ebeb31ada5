// pulse_core_check.cpp — csrc/sp_pulse_core.h alone under the host compiler and its sanitizers (tests/test_pulses_cpu.py).  Every line of
// stdin is one series: "<hi bits> <lo bits> <max_bursts> <width> <value bits> ...", all in hex but the two numbers.  The series is
// measured by the host loop (spp::measure) and, for segments of 64, 128 and SP_BURST_SEGMENT_FRAMES frames, as the kernels measure it:
// SET and RESET masks of 64-frame words, the carry of every segment, then the SEGMENTS IN A SHUFFLED ORDER - every ON frame's burst index
// from the popcount of the rises, its pieces into the head's or the tail's column of the segment or into the burst's cells, the columns'
// non-zero partial cells added to the workspace in that shuffled order, the unsigned maximum of the keys; a second shuffled pass for the
// unsigned minimum of the frames that hold the peak key; a finish per listed burst that stores with one writer per slot.  All must agree
// word for word; the answer goes to stdout as "<count> <edges ...> <energy bits ...> <peak bits ...> <peak_at ...>".
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/spectroplot_hip.h"
#include "sp_pulse_core.h"

namespace {

[[noreturn]] void die(const char *what, size_t line)
{
    fprintf(stderr, "pulse_core_check: %s (line %zu)\n", what, line);
    exit(1);
}

constexpr uint32_t kNoBurst = 0xffffffffu;

struct Reply {
    std::vector<uint64_t> energy, peak;
    std::vector<int32_t> peak_at;
};

// the segments 0 .. segments - 1 in an order that depends on `salt`
std::vector<int32_t> shuffled(int32_t segments, uint32_t salt)
{
    std::vector<int32_t> order((size_t)segments);
    for (int32_t g = 0; g < segments; g++) order[(size_t)g] = g;
    uint32_t state = 12345u + salt * 2654435761u;
    for (int32_t g = segments - 1; g > 0; g--) {
        state = state * 1664525u + 1013904223u;
        std::swap(order[(size_t)g], order[(size_t)((state >> 8) % (uint32_t)(g + 1))]);
    }
    return order;
}

// as the kernels do it, in segments of `seg` frames (a multiple of 64); `total` is the burst kernels' count
void measure_as_kernels(const std::vector<uint64_t> &bits, int32_t width, uint64_t hi_key, uint64_t lo_key, int32_t max_bursts, int32_t seg,
                        uint32_t total, Reply &out, size_t line)
{
    const size_t m = (size_t)max_bursts;
    out.energy.assign(m, ~0ull);
    out.peak.assign(m, ~0ull);
    out.peak_at.assign(m, -1);
    if (width == 0 || max_bursts == 0) return;
    const int32_t words = (width + 63) / 64, per = seg / 64, segments = (width + seg - 1) / seg;
    std::vector<uint64_t> set((size_t)words), reset((size_t)words);
    for (int32_t w = 0; w < words; w++)
        for (int lane = 0; lane < 64; lane++) {
            const int32_t x = w * 64 + lane;
            const uint32_t c = spb::classify(bits[(size_t)(x < width ? x : width - 1)], hi_key, lo_key);
            if (x < width && c == spb::kSet) set[(size_t)w] |= 1ull << lane;
            if (x < width && c == spb::kReset) reset[(size_t)w] |= 1ull << lane;
        }
    auto word = [&](int32_t w, uint64_t &s, uint64_t &r) { s = w < words ? set[(size_t)w] : 0, r = w < words ? reset[(size_t)w] : 0; };
    // the carries (k_burst_carry) and every segment's own rises
    std::vector<uint32_t> base_of((size_t)segments), state_of((size_t)segments), tail_of((size_t)segments);
    {
        uint32_t base = 0, state = 0;
        for (int32_t g = 0; g < segments; g++) {
            base_of[(size_t)g] = base, state_of[(size_t)g] = state;
            spb::Summary sum;
            for (int32_t w = g * per; w < (g + 1) * per; w++) {
                uint64_t s, r;
                word(w, s, r);
                sum = spb::combine(sum, spb::word_summary(s, r));
            }
            const uint32_t rises = spb::rises_after(sum, state);
            tail_of[(size_t)g] = rises ? base + rises - 1 : kNoBurst;
            base += rises;
            state = spb::state_after(sum, state);
        }
        if (base != total) die("the carries' count differs", line);
    }
    std::vector<uint64_t> cells(m * spx::kSlots, 0), peak_key(m, 0);
    std::vector<uint32_t> at(m, 0xffffffffu);   // the int32 array's words, filled with -1

    // one pass over a segment's ON frames of listed bursts: f(frame, burst, where) with where 0 the head, 1 the tail, 2 neither
    auto frames_of = [&](int32_t g, auto &&f) {
        const uint32_t head = state_of[(size_t)g] ? base_of[(size_t)g] - 1 : kNoBurst, tail = tail_of[(size_t)g];
        uint32_t base = base_of[(size_t)g], state = state_of[(size_t)g];
        for (int32_t w = g * per; w < (g + 1) * per; w++) {
            uint64_t s, r;
            word(w, s, r);
            const spb::Step st = spb::step(s, r, state);
            for (int lane = 0; lane < 64; lane++) {
                const int32_t x = w * 64 + lane;
                const uint32_t idx = base + spo::popcount(st.rises & ((2ull << lane) - 1)) - 1;
                if (x < width && (st.on >> lane & 1) != 0 && idx < (uint32_t)max_bursts) f(x, idx, idx == head ? 0 : idx == tail ? 1 : 2, st, lane);
            }
            base += spo::popcount(st.rises);
            state = st.carry;
        }
        return std::pair<uint32_t, uint32_t>(head, tail);
    };

    // k_pulse_accumulate
    for (int32_t g : shuffled(segments, (uint32_t)seg)) {
        uint64_t col[2][spx::kSlots] = {}, col_key[2] = {0, 0};
        const auto ends = frames_of(g, [&](int32_t x, uint32_t idx, int where, const spb::Step &, int) {
            const uint64_t v = bits[(size_t)x];
            const spp::Pieces a = spp::pieces_of(v);
            for (int j = 0; j < 3; j++) {
                if (!a.p[j]) continue;
                if (a.slot + j >= spx::kSlots) die("a non-zero piece points past the slots", line);
                uint64_t &cell = where < 2 ? col[where][a.slot + j] : cells[(size_t)idx * spx::kSlots + (size_t)(a.slot + j)];
                cell += a.p[j];
                if (cell >> 63) die("a cell reaches 2^63", line);
            }
            if (spp::is_candidate(v)) {
                uint64_t &key = where < 2 ? col_key[where] : peak_key[idx];
                if (spt::key_of(v) > key) key = spt::key_of(v);
            }
        });
        for (int c = 0; c < 2; c++) {
            const uint32_t idx = c == 0 ? ends.first : ends.second;
            if (idx >= (uint32_t)max_bursts) {
                for (int k = 0; k < spx::kSlots; k++)
                    if (col[c][k]) die("a column without a listed burst is not zero", line);
                continue;
            }
            for (int k = 0; k < spx::kSlots; k++)
                if (col[c][k]) cells[(size_t)idx * spx::kSlots + (size_t)k] += col[c][k];
            if (col_key[c] > peak_key[idx]) peak_key[idx] = col_key[c];
        }
    }
    // k_pulse_peak_frame
    for (int32_t g : shuffled(segments, (uint32_t)seg + 7u)) {
        uint32_t col_at[2] = {0xffffffffu, 0xffffffffu};
        uint64_t match_word = 0;   // the lanes of the current word that hold their burst's peak
        int32_t match_of = -1;
        const auto ends = frames_of(g, [&](int32_t x, uint32_t idx, int where, const spb::Step &st, int lane) {
            if (spt::key_of(bits[(size_t)x]) != peak_key[idx]) return;
            if (match_of != x / 64) match_of = x / 64, match_word = 0;
            // the first lane of its burst in this word only: no lane of the same burst in front of it matched
            const uint64_t started = st.rises & ((2ull << lane) - 1);
            int rise = -1;
            for (int k = 63; k >= 0 && rise < 0; k--)
                if (started >> k & 1) rise = k;
            const uint64_t from = rise >= 0 ? (1ull << rise) - 1 : 0ull;
            const bool earliest = (match_word & ((1ull << lane) - 1) & ~from) == 0;
            match_word |= 1ull << lane;
            if (!earliest) return;
            uint32_t &slot = where < 2 ? col_at[where] : at[idx];
            if ((uint32_t)x < slot) slot = (uint32_t)x;
        });
        for (int c = 0; c < 2; c++) {
            const uint32_t idx = c == 0 ? ends.first : ends.second;
            if (idx < (uint32_t)max_bursts && col_at[c] < at[idx]) at[idx] = col_at[c];
        }
    }
    // k_pulse_finish: a thread per slot, those behind the listed bursts leave
    std::vector<int> writers(m, 0);
    const uint32_t listed = total < (uint32_t)max_bursts ? total : (uint32_t)max_bursts;
    for (uint32_t i = 0; i < (uint32_t)max_bursts; i++) {
        if (i >= listed) {
            for (int k = 0; k < spx::kSlots; k++)
                if (cells[(size_t)i * spx::kSlots + (size_t)k]) die("a burst behind the list has cells", line);
            continue;
        }
        out.energy[i] = spp::energy_of(&cells[(size_t)i * spx::kSlots]);
        out.peak[i] = peak_key[i];
        if (++writers[i] != 1) die("a slot has two writers", line);
    }
    for (size_t i = 0; i < m; i++) out.peak_at[i] = (int32_t)at[i];
}

}  // namespace

int main()
{
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
        const size_t m = (size_t)max_bursts;
        std::vector<int32_t> edges(2 * m), peak_at(m);
        std::vector<uint64_t> energy(m), peak(m);
        const uint32_t total = spp::measure(bits.data(), width, hi_key, lo_key, max_bursts, edges.data(), energy.data(), peak.data(), peak_at.data());
        for (int32_t seg : {64, 128, SP_BURST_SEGMENT_FRAMES}) {
            Reply got;
            measure_as_kernels(bits, width, hi_key, lo_key, max_bursts, seg, total, got, line);
            if (got.energy != energy) die("the kernels' energy differs", line);
            if (got.peak != peak) die("the kernels' peak differs", line);
            if (got.peak_at != peak_at) die("the kernels' peak_at differs", line);
        }
        printf("%" PRIu32, total);
        for (int32_t e : edges) printf(" %d", e);
        for (uint64_t e : energy) printf(" %" PRIx64, e);
        for (uint64_t e : peak) printf(" %" PRIx64, e);
        for (int32_t e : peak_at) printf(" %d", e);
        printf("\n");
    }
    return 0;
}
