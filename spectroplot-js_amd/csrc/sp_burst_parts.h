// sp_burst_parts.h — what the kernels along a band's series share (sp_kernel_burst.h, sp_kernel_pulse.h): the shape of a segment, the
// thresholds of a launch and a wave's words and summary.  No kernel is defined here, so every device unit may include it.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/spectroplot_hip.h"   // SP_BURST_SEGMENT_FRAMES
#include "sp_band_list.h"                    // kBandMax
#include "sp_burst_core.h"

namespace spk {

constexpr int kBurstUnroll = 8;                          // loads of 64 frames a wave has in flight
constexpr int kBurstWaveFrames = 64 * kBurstUnroll;      // frames of a wave: 4 KiB of its band's series
constexpr int kBurstSegment = SP_BURST_SEGMENT_FRAMES;   // frames of a workgroup's segment (measured: DESIGN.md section 21)
constexpr int kBurstWaves = kBurstSegment / kBurstWaveFrames;
constexpr int kBurstThreads = 64 * kBurstWaves;
static_assert(kBurstSegment % kBurstWaveFrames == 0 && kBurstWaves >= 1 && kBurstWaves <= 16, "a segment is 1 .. 16 waves of 512 frames");

// The thresholds of a launch as a kernel argument, 1 KiB: spo::threshold_key of hi[b] and lo[b], checked by the host.
struct BurstKeys {
    unsigned long long hi[kBandMax], lo[kBandMax];
};

// The SET and RESET masks of the wave's kBurstUnroll words, frames x0 + 64 u + lane of the series `s` of `width` > 0 frames.  Every
// load is issued: a lane past the end re-reads the last frame and is masked behind the load (sp_kernel_occupancy.h).  All of the wave
// may lie past the end: its masks are 0 then, frames that HOLD.
__device__ inline void burst_words(const unsigned long long *__restrict__ s, const int width, const long long x0, const int lane,
                                   const uint64_t hi_key, const uint64_t lo_key, uint64_t (&set)[kBurstUnroll], uint64_t (&reset)[kBurstUnroll])
{
    const long long last = (long long)width - 1;
    unsigned long long v[kBurstUnroll];
#pragma unroll
    for (int u = 0; u < kBurstUnroll; u++) {
        const long long x = x0 + 64 * u + lane;
        v[u] = s[x <= last ? x : last];
    }
#pragma unroll
    for (int u = 0; u < kBurstUnroll; u++) {
        const bool live = x0 + 64 * u + lane <= last;
        const uint32_t c = spb::classify(v[u], hi_key, lo_key);
        set[u] = __ballot(live && c == spb::kSet);
        reset[u] = __ballot(live && c == spb::kReset);
    }
}

__device__ inline spb::Summary burst_wave_summary(const uint64_t (&set)[kBurstUnroll], const uint64_t (&reset)[kBurstUnroll])
{
    spb::Summary sum;
#pragma unroll
    for (int u = 0; u < kBurstUnroll; u++) sum = spb::combine(sum, spb::word_summary(set[u], reset[u]));
    return sum;
}
}  // namespace spk
