// sp_pulse_core.h — the one decision of the burst measurements (include/spectroplot_hip.h, sp_plan_execute_pulses): what a frame adds
// to the energy of its burst and which frame of a burst is its peak.  Plain integer C++, no HIP, in the manner of sp_burst_core.h: the
// host compiler takes it alone (sp_debug_pulses, tests/cpp/pulse_core_check.cpp), and under hipcc the same functions are the device's
// (sp_kernel_pulse.h).  The bursts are spb's, the sum is spx's and the order of powers is spt's; none of them is restated here.
//
// ENERGY.  A frame's value goes, by its key (the sign bit is not looked at), through spx::decompose into at most three pieces for three
// neighbouring cells of its burst's accumulator, u64[spx::kSlots]; a NaN adds one to the NaN slot and +inf one to the inf slot.  A
// piece is one integer add: integer adds commute, so the cells of a burst do not depend on the order of its frames, and sums of
// pieces made elsewhere first (a wave's, a workgroup's) add to the same total.  energy_of() pushes the cells through ONE spx::Finisher
// and applies spx::apply_specials: RN(exact sum), rounded once.
//
// PEAK.  A candidate is (key, frame).  The larger key wins and of equal keys the SMALLER FRAME; a NaN key is no candidate.  That is
// spt::better with a frame where the track has a row: a strict total order on candidates with distinct frames, so any fold order gives
// the same best.  The kernels fold it in two passes that commute each: an unsigned maximum of the keys, then an unsigned minimum of
// the frames that hold that key.
#pragma once

#include <cstdint>

#include "sp_burst_core.h"
#include "sp_exact_sum.h"

namespace spp {

// What one frame adds to its burst's slots: p[j] into slot + j.  A zero piece adds nothing, and only a zero piece may point past the
// slots (slot + j <= 65 wherever p[j] != 0: spx::decompose; a special's one piece is p[0]).
struct Pieces {
    int slot;
    uint32_t p[3];
};

SP_TRACK_FN Pieces pieces_of(uint64_t value_bits)
{
    Pieces a;
    const int kind = spx::decompose(spt::key_of(value_bits), a.slot, a.p);
    if (kind != spx::kFinite) {
        a.slot = kind == spx::kNan ? spx::kNanSlot : spx::kInfSlot;
        a.p[0] = 1;
    }
    return a;
}

// RN(exact sum) of a burst from its slots, with the rule of the specials
SP_TRACK_FN uint64_t energy_of(const uint64_t *slots)
{
    spx::Finisher f;
    for (int k = 0; k < spx::kCells; k++) f.push(slots[k]);
    return spx::apply_specials(f.result(), slots[spx::kNanSlot], slots[spx::kInfSlot]);
}

// a frame of a burst is a candidate for its peak
SP_TRACK_FN bool is_candidate(uint64_t value_bits) { return !spt::is_nan_key(spt::key_of(value_bits)); }

// The measurements of one series of `width` values (bit patterns): spb::scan's bursts, and for burst i < min(total, max_bursts) its
// energy, its peak (both as bit patterns) and the frame of its peak; every other slot all-ones.  Each array may be null.  The host
// side of what the kernels do, and the whole of sp_debug_pulses.  `edges`: 2 * max_bursts words of the caller's, filled here (spb::scan).
inline uint32_t measure(const uint64_t *series_bits, int32_t width, uint64_t hi_key, uint64_t lo_key, int32_t max_bursts, int32_t *edges,
                        uint64_t *energy, uint64_t *peak, int32_t *peak_at)
{
    const uint32_t total = spb::scan(series_bits, width, hi_key, lo_key, max_bursts, edges);
    for (int32_t i = 0; i < max_bursts; i++) {
        if (energy) energy[i] = ~0ull;
        if (peak) peak[i] = ~0ull;
        if (peak_at) peak_at[i] = -1;
    }
    const int32_t listed = total < (uint32_t)max_bursts ? (int32_t)total : max_bursts;
    for (int32_t i = 0; i < listed; i++) {
        uint64_t slots[spx::kSlots] = {};
        spt::Best best;
        for (int32_t x = edges[2 * (size_t)i]; x < edges[2 * (size_t)i + 1]; x++) {
            const Pieces a = pieces_of(series_bits[x]);
            for (int j = 0; j < 3; j++)
                if (a.p[j]) slots[a.slot + j] += a.p[j];
            spt::fold(best, spt::key_of(series_bits[x]), x);
        }
        if (energy) energy[i] = energy_of(slots);
        if (peak) peak[i] = spt::peak_bits_of(best);
        if (peak_at) peak_at[i] = spt::row_of(best);
    }
    return total;
}

}  // namespace spp
