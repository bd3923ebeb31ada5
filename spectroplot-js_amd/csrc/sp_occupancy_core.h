// sp_occupancy_core.h — the one decision of the occupancy counts (include/spectroplot_hip.h, sp_plan_execute_occupancy): does a value of
// a power plane reach its row's threshold.  Plain integer C++, no HIP, in the manner of sp_track_core.h, whose keys these are: the host
// compiler takes it alone (sp_debug_occupancy, tests/cpp/occupancy_core_check.cpp), and under hipcc the same functions are the device's
// (sp_kernel_occupancy.h).
//
// hit(x, y) is numpy's power[x][y] >= threshold[y] for a plane whose values are not negative.  Non-negative doubles and +inf order as
// their keys do as unsigned integers, so the compare is one of keys - once the threshold has been made a key that says the same:
//   a NaN threshold (key above kInfKey)            all ones: no value's key reaches it, and nothing compares >= a NaN;
//   a negative threshold, -inf included            0: every value that is not a NaN reaches it;
//   anything else (+0.0, -0.0, denormals, +inf)    its key; -0.0 is key 0, as +0.0 is.
// A NaN value is no hit whatever the threshold.  So there is no floating-point compare here, as there is none in sp_track_core.h.
//
// A count is a sum of hits, and integer adds commute: the counts do not depend on the order of the rows or frames, on the grid or on
// how the plane is cut into blocks.  The kernel counts a band's rows 64 at a time: the hits of rows g .. g + 63 are one 64-bit word
// (bit i: row g + i), and a band's share of them is the popcount of that word under band_mask().
#pragma once

#include <cstdint>

#include "sp_track_core.h"

namespace spo {

constexpr uint64_t kNoHitKey = ~0ull;   // the key of a NaN threshold: above every key

SP_TRACK_FN uint64_t threshold_key(uint64_t bits)
{
    const uint64_t key = spt::key_of(bits);
    if (spt::is_nan_key(key)) return kNoHitKey;
    return (bits & spt::kSignBit) != 0 && key != 0 ? 0 : key;
}

SP_TRACK_FN bool hit(uint64_t value_bits, uint64_t tkey)
{
    const uint64_t key = spt::key_of(value_bits);
    return (key <= spt::kInfKey) & (key >= tkey);
}

// The bits of the rows [y0, y1) in the hit word of the rows g .. g + 63: bit i is row g + i.  (y0 <= y1; every shift is below 64.)
SP_TRACK_FN uint64_t band_mask(int32_t y0, int32_t y1, int32_t g)
{
    const int32_t lo = y0 - g < 0 ? 0 : (y0 - g > 64 ? 64 : y0 - g);
    const int32_t hi = y1 - g < 0 ? 0 : (y1 - g > 64 ? 64 : y1 - g);
    return hi > lo ? (~0ull >> (64 - (hi - lo))) << lo : 0;
}

SP_TRACK_FN uint32_t popcount(uint64_t word)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__popcll(word);
#else
    return (uint32_t)__builtin_popcountll(word);
#endif
}

// The hits among the rows [y0, y1) of one frame's values against the rows' thresholds (bit patterns both), ascending: the host side
// of what the kernel does, and the whole of sp_debug_occupancy.
SP_TRACK_FN uint32_t band_count(const uint64_t *values, const uint64_t *thresholds, int32_t y0, int32_t y1)
{
    uint32_t count = 0;
    for (int32_t y = y0; y < y1; y++) count += hit(values[y], threshold_key(thresholds[y])) ? 1u : 0u;
    return count;
}

}  // namespace spo
