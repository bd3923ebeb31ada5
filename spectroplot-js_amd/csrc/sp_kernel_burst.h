// sp_kernel_burst.h — the burst lists (include/spectroplot_hip.h, sp_plan_execute_bursts): a Schmitt trigger along the frames of every
// band's power series f64[count][width], its bursts [start, end) counted and listed.  The decision is sp_burst_core.h's and nothing
// else's: keys compared as unsigned integers, 64 frames a step, runs of frames known to what follows them by a Summary that combines
// associatively.  The reply therefore does not depend on the segment size, the grid or the order in which workgroups run.
//
// A recurrence along time in three launches, none of which waits for another workgroup:
//   k_burst_summary   a workgroup per segment of kBurstSegment frames and band: the segment's Summary into the workspace
//   k_burst_carry     a wave per band: the exclusive scan of the band's summaries - the state in front of every segment and the bursts
//                     started before it - the band's total, and the end of a burst that is open behind the last frame
//   k_burst_emit      the first kernel's grid: the segment read again, its words made with the true carry, the edges stored
// Every slot of `edges` has one writer at the most (a burst starts once and ends once), so the stores are plain; the host fills the
// array with -1 in front.  Integer work only: no floating-point compare or add.
#pragma once

#include <hip/hip_runtime.h>

#include "sp_burst_parts.h"   // the segment's shape, BurstKeys, burst_words, burst_wave_summary

namespace spk {

// summaries[b * segments + g] = the packed Summary of the frames [g * kBurstSegment, (g + 1) * kBurstSegment) of band b's series at
// series + b * stride.  grid = (segments, bands), kBurstThreads threads; width > 0.
__global__ __launch_bounds__(kBurstThreads) void k_burst_summary(const unsigned long long *__restrict__ series, const long long stride,
                                                                 const int width, const BurstKeys keys,
                                                                 unsigned long long *__restrict__ summaries)
{
    __shared__ unsigned long long s_sum[kBurstWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.y;
    const long long x0 = (long long)blockIdx.x * kBurstSegment + (long long)wave * kBurstWaveFrames;
    uint64_t set[kBurstUnroll], reset[kBurstUnroll];
    burst_words(series + (size_t)b * (size_t)stride, width, x0, lane, keys.hi[b], keys.lo[b], set, reset);
    const spb::Summary mine = burst_wave_summary(set, reset);   // (uniform: made of ballots)
    if (lane == 0) s_sum[wave] = spb::pack(mine);
    __syncthreads();
    if (tid == 0) {
        spb::Summary sum;
#pragma unroll
        for (int w = 0; w < kBurstWaves; w++) sum = spb::combine(sum, spb::unpack(s_sum[w]));
        summaries[(size_t)b * gridDim.x + blockIdx.x] = spb::pack(sum);
    }
}

// One wave per band b = blockIdx.x: carries[b * segments + g] = the bursts started before segment g in its low word and the state in
// front of it in bit 32; counts[b] = the band's total (counts may be null); and where the last burst is open behind the last frame
// and listed, its end = width (edges may be null).  64 summaries a step: an inclusive shuffle scan with combine, behind the running
// summary of the steps before.  segments == 0 (a series of no frames) writes the total 0 and nothing else.
__global__ __launch_bounds__(64) void k_burst_carry(const unsigned long long *__restrict__ summaries, const int segments, const int width,
                                                    const int max_bursts, unsigned long long *__restrict__ carries,
                                                    uint32_t *__restrict__ counts, int32_t *__restrict__ edges)
{
    const int lane = threadIdx.x, b = blockIdx.x;
    const unsigned long long *const in = summaries + (size_t)b * (size_t)segments;
    unsigned long long *const out = carries + (size_t)b * (size_t)segments;
    spb::Summary run;   // of the segments in front of this step
    for (int g0 = 0; g0 < segments; g0 += 64) {   // (uniform)
        const int g = g0 + lane;
        const unsigned long long w = in[g < segments ? g : segments - 1];
        spb::Summary incl = spb::unpack(g < segments ? w : 0ull);   // (a segment that does not exist: the summary of no frames)
#pragma unroll
        for (int d = 1; d < 64; d *= 2) {
            const spb::Summary left = spb::unpack(__shfl_up(spb::pack(incl), d, 64));
            if (lane >= d) incl = spb::combine(left, incl);
        }
        const unsigned long long before = __shfl_up(spb::pack(incl), 1, 64);
        const spb::Summary excl = lane == 0 ? run : spb::combine(run, spb::unpack(before));
        if (g < segments) out[g] = (unsigned long long)excl.rises | (unsigned long long)spb::state_after(excl, 0) << 32;
        run = spb::combine(run, spb::unpack(__shfl(spb::pack(incl), 63, 64)));
    }
    if (lane == 0) {
        if (counts) counts[b] = run.rises;
        if (edges && spb::state_after(run, 0) != 0 && run.rises - 1 < (uint32_t)max_bursts)
            edges[(size_t)b * 2 * (size_t)max_bursts + 2 * (size_t)(run.rises - 1) + 1] = width;
    }
}

// edges[b][2 i] = the start and edges[b][2 i + 1] = the end of burst i < max_bursts of band b, for the starts and the ends that lie in
// this workgroup's segment.  grid = (segments, bands), kBurstThreads threads; width > 0, max_bursts > 0.  A wave makes its words as
// k_burst_summary does, the waves exchange their summaries through LDS, and a wave's carry is the segment's (k_burst_carry) followed by
// the waves in front of it.  Then word by word: the lane of a rise stores its frame at the slot of the bursts started before it, the
// lane of a fall at the end of the last burst started.
__global__ __launch_bounds__(kBurstThreads) void k_burst_emit(const unsigned long long *__restrict__ series, const long long stride,
                                                              const int width, const BurstKeys keys,
                                                              const unsigned long long *__restrict__ carries, const int max_bursts,
                                                              int32_t *__restrict__ edges)
{
    __shared__ unsigned long long s_sum[kBurstWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.y;
    const long long x0 = (long long)blockIdx.x * kBurstSegment + (long long)wave * kBurstWaveFrames;
    uint64_t set[kBurstUnroll], reset[kBurstUnroll];
    burst_words(series + (size_t)b * (size_t)stride, width, x0, lane, keys.hi[b], keys.lo[b], set, reset);
    const unsigned long long carry = carries[(size_t)b * gridDim.x + blockIdx.x];
    if (kBurstWaves > 1) {
        const spb::Summary mine = burst_wave_summary(set, reset);
        if (lane == 0) s_sum[wave] = spb::pack(mine);
        __syncthreads();
    }
    uint32_t base = (uint32_t)carry, state = (uint32_t)(carry >> 32) & 1u;
    for (int w = 0; w < wave; w++) {   // (uniform)
        const spb::Summary front = spb::unpack(s_sum[w]);
        base += spb::rises_after(front, state);
        state = spb::state_after(front, state);
    }
    int32_t *const row = edges + (size_t)b * 2 * (size_t)max_bursts;
    const uint64_t below = (1ull << lane) - 1;
#pragma unroll
    for (int u = 0; u < kBurstUnroll; u++) {
        const spb::Step st = spb::step(set[u], reset[u], state);
        const uint32_t started = base + spo::popcount(st.rises & below);   // the bursts started in front of this lane's frame
        const int32_t x = (int32_t)(x0 + 64 * u + lane);
        if ((st.rises >> lane & 1) != 0 && started < (uint32_t)max_bursts) row[2 * (size_t)started] = x;
        if ((st.falls >> lane & 1) != 0 && started - 1 < (uint32_t)max_bursts) row[2 * (size_t)(started - 1) + 1] = x;
        base += spo::popcount(st.rises);
        state = st.carry;
    }
}

}  // namespace spk
