// sp_burst_core.h — the one decision of the burst lists (include/spectroplot_hip.h, sp_plan_execute_bursts): a Schmitt trigger along
// the frames of a band's power series.  Plain integer C++, no HIP, in the manner of sp_occupancy_core.h, whose keys and whose hit()
// these are: the host compiler takes it alone (sp_debug_bursts, tests/cpp/burst_core_check.cpp), and under hipcc the same functions are
// the device's (sp_kernel_burst.h).  No floating-point compare.
//
// A frame is one of three things (classify): SET, its value reaches `hi`; RESET, its value is below `lo`; HOLD, anything else - a value
// between the two and every NaN.  With lo_key <= hi_key no frame is both.  The state behind a frame is ON where the last frame at or
// before it that is not HOLD is a SET, and OFF where it is a RESET or there is none: the machine starts OFF.
//
// 64 frames are one step (step): with the SET frames and the RESET frames as two 64-bit masks, bit i the i-th frame, the state in front
// of every frame is the carry chain of ONE ADDITION.  Adding ~reset and set, a SET frame is 1 + 1 (a carry goes out whatever comes in),
// a HOLD frame is 1 + 0 (the carry passes) and a RESET frame is 0 + 0 (no carry goes out): the carry into bit i is the state in front
// of frame i, and a sum's carries are sum ^ a ^ b.
//
// A run of frames is known to what follows it by a Summary: the class of its first frame that is not HOLD, that of its last, and the
// bursts that start in it when the state in front of it is OFF.  Were the state ON, the count is the same less one where the first
// event is a SET (that SET then continues a burst); the state behind the run is its last event's, or the state in front where it has no
// event.  combine(a, b) is the summary of a followed by b.  It is associative, so summaries may be folded in any grouping - over the
// words of a wave, the waves of a workgroup, the segments of a band - as long as the order stands: the reply does not depend on how
// the series is cut.
#pragma once

#include <cstdint>

#include "sp_occupancy_core.h"

namespace spb {

constexpr uint32_t kHold = 0, kSet = 1, kReset = 2;

// `hi_key`, `lo_key`: spo::threshold_key of the thresholds, neither of them a NaN's, lo_key <= hi_key
SP_TRACK_FN uint32_t classify(uint64_t value_bits, uint64_t hi_key, uint64_t lo_key)
{
    const uint64_t key = spt::key_of(value_bits);
    if (spo::hit(value_bits, hi_key)) return kSet;
    return ((key <= spt::kInfKey) & (key < lo_key)) ? kReset : kHold;
}

struct Step {
    uint64_t on;      // bit i: the state behind frame i
    uint64_t rises;   // bit i: frame i is the first of a burst
    uint64_t falls;   // bit i: frame i is the first behind a burst, its `end`
    uint32_t carry;   // the state behind frame 63
};

// 64 frames at once; `carry` is the state in front of frame 0 (0 or 1), set & reset == 0.  A frame that does not exist is a HOLD.
SP_TRACK_FN Step step(uint64_t set, uint64_t reset, uint32_t carry)
{
    const uint64_t a = ~reset, sum = a + set + (uint64_t)carry;   // (wraps: the carry out of bit 63 is `on`'s top bit)
    const uint64_t before = sum ^ a ^ set;                        // bit i: the state in front of frame i
    Step s;
    s.on = set | (a & before);
    s.rises = s.on & ~before;
    s.falls = before & ~s.on;
    s.carry = (uint32_t)(s.on >> 63);
    return s;
}

struct Summary {
    uint32_t first = kHold;   // the class of the first frame that is not HOLD, kHold where there is none
    uint32_t last = kHold;    // the class of the last one
    uint32_t rises = 0;       // the bursts that start in the run when the state in front of it is OFF
};

SP_TRACK_FN Summary word_summary(uint64_t set, uint64_t reset)
{
    const uint64_t events = set | reset;
    Summary s;
    if (events != 0) {
        s.first = (set & (events & (0 - events))) != 0 ? kSet : kReset;   // (the lowest event)
        s.last = set > reset ? kSet : kReset;                              // (disjoint masks: the larger one holds the highest event)
        s.rises = spo::popcount(step(set, reset, 0).rises);
    }
    return s;
}

// the bursts that start in the run, and the state behind it, when the state in front of it is `carry`
SP_TRACK_FN uint32_t rises_after(const Summary &s, uint32_t carry) { return s.rises - (((carry != 0) & (s.first == kSet)) ? 1u : 0u); }
SP_TRACK_FN uint32_t state_after(const Summary &s, uint32_t carry) { return s.last == kHold ? carry : (s.last == kSet ? 1u : 0u); }

// a followed by b
SP_TRACK_FN Summary combine(const Summary &a, const Summary &b)
{
    Summary s;
    s.first = a.first != kHold ? a.first : b.first;
    s.last = b.last != kHold ? b.last : a.last;
    s.rises = a.rises + rises_after(b, state_after(a, 0));
    return s;
}

// a summary as one word, for a shuffle and for the workspace
SP_TRACK_FN uint64_t pack(const Summary &s) { return (uint64_t)s.rises | (uint64_t)s.first << 32 | (uint64_t)s.last << 34; }
SP_TRACK_FN Summary unpack(uint64_t w)
{
    Summary s;
    s.rises = (uint32_t)w;
    s.first = (uint32_t)(w >> 32) & 3u;
    s.last = (uint32_t)(w >> 34) & 3u;
    return s;
}

// The bursts of one series of `width` values (bit patterns), frame by frame: the total, and into edges[2 * max_bursts] (may be null)
// the start and the end of the first max_bursts of them, every other slot -1.  The host side of what the kernels do, and the whole of
// sp_debug_bursts.
SP_TRACK_FN uint32_t scan(const uint64_t *series_bits, int32_t width, uint64_t hi_key, uint64_t lo_key, int32_t max_bursts, int32_t *edges)
{
    if (edges)
        for (int64_t i = 0; i < 2 * (int64_t)max_bursts; i++) edges[i] = -1;
    uint32_t total = 0;
    bool on = false;
    for (int32_t x = 0; x < width; x++) {
        const uint32_t c = classify(series_bits[x], hi_key, lo_key);
        if (c == kSet && !on) {
            if (edges && total < (uint32_t)max_bursts) edges[2 * (size_t)total] = x;
            total++;
            on = true;
        } else if (c == kReset && on) {
            if (edges && total - 1 < (uint32_t)max_bursts) edges[2 * (size_t)(total - 1) + 1] = x;
            on = false;
        }
    }
    if (on && edges && total - 1 < (uint32_t)max_bursts) edges[2 * (size_t)(total - 1) + 1] = width;
    return total;
}

}  // namespace spb
