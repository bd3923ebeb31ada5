// sp_kernel_pulse.h — the burst measurements (include/spectroplot_hip.h, sp_plan_execute_pulses): for every listed burst of every
// band's power series its exact energy, its peak and the frame of its peak.  The bursts are the burst kernels' (sp_kernel_burst.h, run
// in front, unchanged), what a frame adds and which frame is the peak is sp_pulse_core.h's.  A segmented reduction along time over
// segments whose lengths only the device knows - a burst is one frame or a million - on the burst kernels' grid, which the host knows
// without a synchronisation:
//   k_pulse_accumulate   a workgroup per segment of kBurstSegment frames and band: every ON frame's pieces into its burst's cells
//                        u64[count][max_bursts][spx::kSlots] and its key into peak_key[count][max_bursts], with integer atomic adds and
//                        an unsigned 64-bit atomic max whose return values are not used.  Both commute: the words do not depend on order.
//   k_pulse_peak_frame   the same grid, the segment read again: where a frame's key equals its burst's peak_key, an atomic UNSIGNED min of
//                        the frame into peak_at - the -1 the host filled is the largest unsigned word, so every frame beats it.
//   k_pulse_finish       a thread per listed burst: its cells through one spx::Finisher, energy and peak stored with plain stores
// No workgroup waits for another: no flags, no look-back, no cooperative launch.
//
// A long burst spans hundreds of workgroups that would all hit the same few cells.  So a workgroup gathers two bursts in LDS and
// flushes their non-zero cells once at its end: the HEAD, the burst that is ON at the segment's first frame, and the TAIL, the last
// burst that starts in the segment.  Every other burst of the segment lies wholly inside it: one workgroup, no contention.  In front
// of the atomics a wave folds its 64 frames: by burst for the key, by (burst, slot) for the pieces, a round per group as sp_kernel_band.h's
// band_fold does by cell, at most kPulseRounds rounds; what is left then - words of many short bursts - goes lane by lane.
#pragma once

#include <hip/hip_runtime.h>

#include "sp_burst_parts.h"   // the segment's shape, BurstKeys, burst_wave_summary
#include "sp_pulse_core.h"
#include "sp_wave_sum.h"

namespace spk {

constexpr int kPulseRounds = 6;                // fold rounds of a word; a word of more bursts than this is not folded at all
constexpr uint32_t kNoBurst = 0xffffffffu;     // the index of "no such burst": above every index (max_bursts < 2^30)
constexpr int kPulseHead = 0, kPulseTail = 1, kPulseGlobal = 2;   // where a burst's accumulators are: LDS column 0 or 1, or the workspace

// The sum of x over the wave's 64 lanes, exactly (sp_wave_sum.h).  16 bits at a time, so that a half's total stays below 2^22 and is
// a 32-bit word.  Every lane of the wave must be here.
__device__ inline unsigned long long pulse_wave_sum(uint32_t x)
{
    return (unsigned long long)wave_rows_total<uint32_t>(wave_row_sums(x & 0xffffu)) +
           ((unsigned long long)wave_rows_total<uint32_t>(wave_row_sums(x >> 16)) << 16);
}

// the largest k of the wave's 64 lanes, in every lane
__device__ inline unsigned long long pulse_wave_max(unsigned long long k)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(k, d, 64);
        k = o > k ? o : k;
    }
    return k;
}

// The values of the wave's kBurstUnroll words and their SET and RESET masks: burst_words (sp_kernel_burst.h) with the values kept.
// Every load is issued: a lane past the end re-reads the last frame and is masked behind the load.
__device__ inline void pulse_words(const unsigned long long *__restrict__ s, const int width, const long long x0, const int lane,
                                   const uint64_t hi_key, const uint64_t lo_key, unsigned long long (&v)[kBurstUnroll],
                                   uint64_t (&set)[kBurstUnroll], uint64_t (&reset)[kBurstUnroll])
{
    const long long last = (long long)width - 1;
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

// What a wave knows of its segment once the waves have exchanged their summaries through s_sum (a barrier inside): the bursts started
// in front of the wave's first frame and the state there, and the segment's head and tail bursts (kNoBurst where there is none).
struct PulseWave {
    uint32_t base, state, head, tail;
};

__device__ inline PulseWave pulse_wave(unsigned long long *s_sum, const int wave, const int lane, const unsigned long long carry,
                                       const uint64_t (&set)[kBurstUnroll], const uint64_t (&reset)[kBurstUnroll])
{
    const spb::Summary mine = burst_wave_summary(set, reset);
    if (lane == 0) s_sum[wave] = spb::pack(mine);
    __syncthreads();
    PulseWave w;
    uint32_t base = (uint32_t)carry, state = (uint32_t)(carry >> 32) & 1u;
    w.head = state ? base - 1 : kNoBurst;   // (ON in front of the segment: a burst has started before it)
    w.base = base, w.state = state;
#pragma unroll
    for (int k = 0; k < kBurstWaves; k++) {   // (uniform)
        if (k == wave) w.base = base, w.state = state;
        const spb::Summary front = spb::unpack(s_sum[k]);
        base += spb::rises_after(front, state);
        state = spb::state_after(front, state);
    }
    w.tail = base != (uint32_t)carry ? base - 1 : kNoBurst;
    return w;
}

// The burst of a lane's frame in a word: the bursts started at or before it, less one (meaningless where the frame is not ON).
__device__ inline uint32_t pulse_index(const spb::Step &st, const uint32_t base, const int lane)
{
    return base + spo::popcount(st.rises & ((2ull << lane) - 1)) - 1;
}

__device__ inline int pulse_where(const PulseWave &w, const uint32_t idx) { return idx == w.head ? kPulseHead : idx == w.tail ? kPulseTail : kPulseGlobal; }

// cells[(b * max_bursts + i) * kSlots + k] += the pieces and peak_key[b * max_bursts + i] = max of the keys of the frames of burst
// i < max_bursts of band b that lie in this workgroup's segment.  grid = (segments, bands), kBurstThreads threads; width > 0,
// max_bursts > 0; the host has zeroed both arrays.  A frame of a burst behind the list is dropped.
__global__ __launch_bounds__(kBurstThreads) void k_pulse_accumulate(const unsigned long long *__restrict__ series, const long long stride,
                                                                    const int width, const BurstKeys keys,
                                                                    const unsigned long long *__restrict__ carries, const int max_bursts,
                                                                    unsigned long long *__restrict__ cells,
                                                                    unsigned long long *__restrict__ peak_key)
{
    __shared__ unsigned long long s_sum[kBurstWaves];
    __shared__ unsigned long long s_cells[2][spx::kSlots];
    __shared__ unsigned long long s_key[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.y;
    for (int k = tid; k < 2 * spx::kSlots; k += kBurstThreads) (&s_cells[0][0])[k] = 0;
    if (tid < 2) s_key[tid] = 0;
    const long long x0 = (long long)blockIdx.x * kBurstSegment + (long long)wave * kBurstWaveFrames;
    unsigned long long v[kBurstUnroll];
    uint64_t set[kBurstUnroll], reset[kBurstUnroll];
    pulse_words(series + (size_t)b * (size_t)stride, width, x0, lane, keys.hi[b], keys.lo[b], v, set, reset);
    const unsigned long long carry = carries[(size_t)b * gridDim.x + blockIdx.x];
    const PulseWave w = pulse_wave(s_sum, wave, lane, carry, set, reset);   // (its barrier stands behind the zeroing, too)

    unsigned long long *const g_cells = cells + (size_t)b * (size_t)max_bursts * spx::kSlots;
    unsigned long long *const g_key = peak_key + (size_t)b * (size_t)max_bursts;
    // one add, one max: into the LDS column of the head or the tail, or into the workspace (idx < max_bursts, slot < kSlots)
    auto add = [&](const int where, const uint32_t idx, const int slot, const unsigned long long value) {
        if (where != kPulseGlobal) atomicAdd(&s_cells[where][slot], value);
        else atomicAdd(&g_cells[(size_t)idx * spx::kSlots + slot], value);
    };
    auto key_max = [&](const int where, const uint32_t idx, const unsigned long long key) {
        if (where != kPulseGlobal) atomicMax(&s_key[where], key);
        else atomicMax(&g_key[idx], key);
    };

    uint32_t base = w.base, state = w.state;
#pragma unroll
    for (int u = 0; u < kBurstUnroll; u++) {
        const spb::Step st = spb::step(set[u], reset[u], state);
        const uint32_t idx = pulse_index(st, base, lane);
        const bool inside = x0 + 64 * u + lane < (long long)width;   // (a frame that does not exist is a HOLD: ON behind an open burst)
        const bool live = inside && (st.on >> lane & 1) != 0 && idx < (uint32_t)max_bursts;
        const int where = pulse_where(w, idx);
        const bool folds = spo::popcount(st.rises) < (uint32_t)kPulseRounds;   // (uniform)
        base += spo::popcount(st.rises);
        state = st.carry;
        if (__ballot(live) == 0) continue;   // (uniform)

        // the key: a round per burst, its first lane adds for all
        bool cand = live && spp::is_candidate(v[u]);
        const unsigned long long key = spt::key_of(v[u]);
        unsigned long long left = __ballot(cand);
        for (int r = 0; folds && r < kPulseRounds && left; r++) {   // (uniform)
            const int first = __ffsll((long long)left) - 1;
            const uint32_t bi = (uint32_t)__builtin_amdgcn_readlane((int)idx, first);
            const bool take = cand && idx == bi;
            const unsigned long long m = pulse_wave_max(take ? key : 0ull);
            if (lane == first) key_max(where, idx, m);
            cand = cand && !take;
            left &= ~__ballot(take);
        }
        if (cand) key_max(where, idx, key);

        // the pieces: a round per (burst, slot), lanes 0 .. 2 add the three sums where the first lane's burst is
        const spp::Pieces a = spp::pieces_of(v[u]);
        bool mine = live && (a.p[0] | a.p[1] | a.p[2]) != 0;
        left = __ballot(mine);
        for (int r = 0; folds && r < kPulseRounds && left; r++) {   // (uniform)
            const int first = __ffsll((long long)left) - 1;
            const uint32_t bi = (uint32_t)__builtin_amdgcn_readlane((int)idx, first);
            const int c = __builtin_amdgcn_readlane(a.slot, first);
            const int wh = __builtin_amdgcn_readlane(where, first);
            const bool take = mine && idx == bi && a.slot == c;
            const unsigned long long s0 = pulse_wave_sum(take ? a.p[0] : 0u), s1 = pulse_wave_sum(take ? a.p[1] : 0u),
                                     s2 = pulse_wave_sum(take ? a.p[2] : 0u);
            const unsigned long long s = lane == 0 ? s0 : lane == 1 ? s1 : s2;
            if (lane < 3 && s != 0 && c + lane < spx::kSlots) add(wh, bi, c + lane, s);   // (a non-zero sum never points past the slots)
            mine = mine && !take;
            left &= ~__ballot(take);
        }
        if (mine) {
#pragma unroll
            for (int j = 0; j < 3; j++)
                if (a.p[j] != 0 && a.slot + j < spx::kSlots) add(where, idx, a.slot + j, a.p[j]);
        }
    }

    __syncthreads();
    for (int k = tid; k < 2 * spx::kSlots + 2; k += kBurstThreads) {
        const int col = k < 2 * spx::kSlots ? k / spx::kSlots : k - 2 * spx::kSlots;
        const uint32_t idx = col == kPulseHead ? w.head : w.tail;
        if (idx >= (uint32_t)max_bursts) continue;   // (kNoBurst, or a burst behind the list: its column is zero anyway)
        if (k < 2 * spx::kSlots) {
            const unsigned long long value = s_cells[col][k % spx::kSlots];
            if (value) atomicAdd(&g_cells[(size_t)idx * spx::kSlots + k % spx::kSlots], value);
        } else {
            const unsigned long long key = s_key[col];
            if (key) atomicMax(&g_key[idx], key);
        }
    }
}

// peak_at[b * max_bursts + i] = the earliest frame of burst i < max_bursts of band b whose key is peak_key[b * max_bursts + i], for
// the frames of this workgroup's segment.  The same grid and the same words as k_pulse_accumulate, behind it.  The minimum is an
// UNSIGNED one, on the words of the int32 array: the host's -1 fill is 0xffffffff, above every frame.  Of the lanes of a word that hold
// their burst's peak only the first of each burst goes on; the head and the tail burst gather in LDS and flush once.
__global__ __launch_bounds__(kBurstThreads) void k_pulse_peak_frame(const unsigned long long *__restrict__ series, const long long stride,
                                                                    const int width, const BurstKeys keys,
                                                                    const unsigned long long *__restrict__ carries, const int max_bursts,
                                                                    const unsigned long long *__restrict__ peak_key,
                                                                    int32_t *__restrict__ peak_at)
{
    __shared__ unsigned long long s_sum[kBurstWaves];
    __shared__ uint32_t s_at[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.y;
    if (tid < 2) s_at[tid] = kNoBurst;
    const long long x0 = (long long)blockIdx.x * kBurstSegment + (long long)wave * kBurstWaveFrames;
    unsigned long long v[kBurstUnroll];
    uint64_t set[kBurstUnroll], reset[kBurstUnroll];
    pulse_words(series + (size_t)b * (size_t)stride, width, x0, lane, keys.hi[b], keys.lo[b], v, set, reset);
    const unsigned long long carry = carries[(size_t)b * gridDim.x + blockIdx.x];
    const PulseWave w = pulse_wave(s_sum, wave, lane, carry, set, reset);

    const unsigned long long *const g_key = peak_key + (size_t)b * (size_t)max_bursts;
    uint32_t *const g_at = (uint32_t *)peak_at + (size_t)b * (size_t)max_bursts;
    const uint64_t below = (1ull << lane) - 1;
    uint32_t base = w.base, state = w.state;
#pragma unroll
    for (int u = 0; u < kBurstUnroll; u++) {
        const spb::Step st = spb::step(set[u], reset[u], state);
        const uint32_t idx = pulse_index(st, base, lane);
        const long long x = x0 + 64 * u + lane;
        const bool live = x < (long long)width && (st.on >> lane & 1) != 0 && idx < (uint32_t)max_bursts;
        base += spo::popcount(st.rises);
        state = st.carry;
        const unsigned long long best = g_key[live ? idx : 0u];   // (issued by every lane: slot 0 exists, max_bursts > 0)
        const bool match = live && spt::key_of(v[u]) == best;     // (a NaN's key is no burst's peak)
        // the lanes of this lane's burst in front of it: from the burst's rise in this word, or from lane 0, up to the lane
        const uint64_t started = st.rises & ((2ull << lane) - 1);
        const uint64_t from = started ? (1ull << (63 - __clzll((long long)started))) - 1 : 0ull;
        const bool earliest = match && (__ballot(match) & below & ~from) == 0;
        if (earliest) {
            const int where = pulse_where(w, idx);
            if (where != kPulseGlobal) atomicMin(&s_at[where], (uint32_t)x);
            else atomicMin(&g_at[idx], (uint32_t)x);
        }
    }
    __syncthreads();
    if (tid < 2) {
        const uint32_t idx = tid == kPulseHead ? w.head : w.tail;
        if (idx < (uint32_t)max_bursts && s_at[tid] != kNoBurst) atomicMin(&g_at[idx], s_at[tid]);
    }
}

// energy[b * max_bursts + i] and peak[b * max_bursts + i] of the listed bursts i < min(counts[b], max_bursts): plain stores, a thread a
// burst, one writer a slot.  grid = (ceil(max_bursts / 64), bands), 64 threads.  Either output may be null.  A burst's cells are 544
// contiguous bytes: a thread reading its own would touch 64 lines a load, so the wave reads the cells of its 64 bursts as one
// contiguous run, 512 bytes a load, into LDS - a row of kPulseRow words per burst, one word of padding so that the threads' rows start
// on different banks - and every thread finishes its row from there (measured: DESIGN.md section 22).
constexpr int kPulseRow = spx::kSlots + 1;

__global__ __launch_bounds__(64) void k_pulse_finish(const uint32_t *__restrict__ counts, const int max_bursts,
                                                     const unsigned long long *__restrict__ cells,
                                                     const unsigned long long *__restrict__ peak_key, double *__restrict__ energy,
                                                     double *__restrict__ peak)
{
    __shared__ unsigned long long s_rows[64 * kPulseRow];
    const int b = blockIdx.y, lane = threadIdx.x;
    const long long first = (long long)blockIdx.x * 64;
    const uint32_t total = counts[b];
    const long long listed = total < (uint32_t)max_bursts ? (long long)total : (long long)max_bursts;
    if (first >= listed) return;   // (uniform)
    const int here = listed - first < 64 ? (int)(listed - first) : 64;   // the listed bursts of this workgroup
    const size_t at = (size_t)b * (size_t)max_bursts + (size_t)first;
    if (energy) {   // (uniform)
        const unsigned long long *const src = cells + at * spx::kSlots;   // here * kSlots words, inside the band's cells
        for (int k = lane; k < here * spx::kSlots; k += 64) s_rows[(k / spx::kSlots) * kPulseRow + k % spx::kSlots] = src[k];
        __syncthreads();
    }
    if (lane >= here) return;
    if (energy) energy[at + lane] = __longlong_as_double((long long)spp::energy_of((const uint64_t *)&s_rows[lane * kPulseRow]));
    if (peak) peak[at + lane] = __longlong_as_double((long long)peak_key[at + lane]);
}

}  // namespace spk
