// sp_kernel_occupancy.h — the occupancy counts (include/spectroplot_hip.h, sp_plan_execute_occupancy): with hit(x, y) = power[x][y]
// reaches threshold[y], rows[y] = the frames x that hit and frames[b][x] = the rows of the band [y0_b, y1_b) that hit.  The decision is
// sp_occupancy_core.h's and nothing else's: keys compared as unsigned integers.  Both results are sums of hits made by integer adds
// alone - in registers, in LDS and, where workgroups meet on a word, by integer atomics in global memory - so they do not depend on the
// grid, on the order of anything or on how the plane is cut into blocks of frames.  The host zeroes both outputs in front of the first
// block.
//
// One launch, the plane read once whichever outputs are asked, no global workspace, no floating-point compare or add.
#pragma once

#include <hip/hip_runtime.h>

#include "sp_band_list.h"   // the bands travel as they do for k_band_sum
#include "sp_occupancy_core.h"

namespace spk {

constexpr int kOccWaves = 4;           // waves of a workgroup
constexpr int kOccThreads = 64 * kOccWaves;
#ifndef SP_OCC_WAVE_FRAMES
#define SP_OCC_WAVE_FRAMES 4           // (a compile-time knob for tools/occupancy_bench.py's variants only)
#endif
constexpr int kOccWaveFrames = SP_OCC_WAVE_FRAMES;   // frames a wave owns: wave w takes the frames w, w + 4, ... of its piece
constexpr int kOccFrames = kOccWaves * kOccWaveFrames;   // frames of a workgroup's piece (measured: DESIGN.md section 19)
constexpr int kOccUnroll = 8;          // loads of 64 rows a wave has in flight per frame
constexpr int kOccTileRows = 4096;     // rows of a workgroup's tile: one u32 count each in LDS, 16 KiB.  Every plan size up to n = 4096 is
                                       // one tile; SP_MAX_N (2^20 rows) is 256 tiles.
constexpr int kOccFramePitch = kOccFrames + 1;   // s_frames[band][frame of the piece], an odd pitch: lane b's stores spread over the banks

// rows[y] += the hits of row y in the frames [0, frames) of the frame-major plane at `plane` (frame x, row y at plane[x * n + y]) and
// out[b * stride + x_base + x] += the hits of frame x in the rows of band b that lie in this workgroup's tile, for every band b <
// count; either output may be null and is not touched then.  grid = (pieces of kOccFrames frames, tiles of kOccTileRows rows), 256
// threads.
//
// A wave owns kOccWaveFrames frames of the piece and sweeps the tile's rows 64 * kOccUnroll at a time.  Per sweep step it loads the
// rows' thresholds once and makes their keys, then reads the step's rows of each of its frames: 64 rows, 512 contiguous bytes, per
// load, kOccUnroll loads in flight, none under a branch - a lane past the tile's end re-reads the tile's last row and is masked behind
// the load (sp_kernel_track.h).  (The frames are the inner loop and not the outer one so that the thresholds, their keys and the
// bands' bit masks of a step are made once for the wave's frames, and so that a lane adds the hits of its row over those frames in a
// register: one LDS add per row and wave, not one per value.)
//
// Row counts: s_rows[row of the tile].  A lane adds its row's hits with one LDS add without a return value; the addresses of a wave's
// lanes are 64 neighbouring words.  Behind the barrier the slots that are not 0 go to rows[y] by global integer adds, a wave's 64
// lanes on 256 contiguous bytes.
//
// Frame counts: LANE b IS BAND b.  It keeps its [y0, y1) in registers; per load the wave's hits are one uniform 64-bit ballot, of
// which lane b counts the bits of its band (spo::band_mask) into a register per frame - all 64 bands at once in a few vector
// operations, no loop over bands.  At the end lane b < count stores the counts to s_frames[b][frame of the piece], and behind the
// barrier the threads add them to out[b * stride + x_base + x], a band's kOccFrames neighbouring frames on neighbouring words.  With
// one tile every word of `out` gets one add; a band that spans tiles gets one per tile.
__global__ __launch_bounds__(kOccThreads) void k_occupancy_count(const double *__restrict__ plane, const int n, const long long frames,
                                                                 const unsigned long long *__restrict__ threshold, const BandList bands,
                                                                 const int count, uint32_t *__restrict__ rows, uint32_t *__restrict__ out,
                                                                 const long long stride, const long long x_base)
{
    __shared__ uint32_t s_rows[kOccTileRows];
    __shared__ uint32_t s_frames[kBandMax * kOccFramePitch];
    __shared__ int32_t s_band[2 * kBandMax];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r0 = (int)blockIdx.y * kOccTileRows;                               // the tile: rows [r0, r1), not empty
    const int r1 = n - r0 > kOccTileRows ? r0 + kOccTileRows : n;
    const long long first = (long long)blockIdx.x * kOccFrames;
    const bool want_rows = rows != nullptr, want_frames = out != nullptr && count > 0;   // (uniform)

    if (want_rows)
        for (int i = tid; i < r1 - r0; i += kOccThreads) s_rows[i] = 0;
    if (tid < 2 * kBandMax) s_band[tid] = tid < 2 * count ? bands.y[tid] : 0;   // (a lane past the list: the empty band [0, 0))
    __syncthreads();
    const int y0 = s_band[2 * lane], y1 = s_band[2 * lane + 1];

    if (first + wave < frames) {   // (uniform: the wave owns a frame at least)
        // Every load is issued: a frame past the end reads the plane's last frame instead and is dropped behind the loads.
        const unsigned long long *col[kOccWaveFrames];
        bool live[kOccWaveFrames];
        uint32_t band_hits[kOccWaveFrames];
#pragma unroll
        for (int f = 0; f < kOccWaveFrames; f++) {
            const long long x = first + wave + (long long)f * kOccWaves;
            live[f] = x < frames;
            // (64-bit: 8 * width * n passes 4 GiB)
            col[f] = (const unsigned long long *)plane + (size_t)(live[f] ? x : frames - 1) * (size_t)n;
            band_hits[f] = 0;
        }
        const int last = r1 - 1;
        for (int y = r0; y < r1; y += 64 * kOccUnroll) {   // (wave-uniform)
            const int yl = y + lane;
            uint64_t tkey[kOccUnroll], mask[kOccUnroll];
            uint32_t row_hits[kOccUnroll];
#pragma unroll
            for (int u = 0; u < kOccUnroll; u++) tkey[u] = threshold[yl + 64 * u <= last ? yl + 64 * u : last];
#pragma unroll
            for (int u = 0; u < kOccUnroll; u++) {
                // (a row past the tile's end hits nothing)
                tkey[u] = yl + 64 * u <= last ? spo::threshold_key(tkey[u]) : spo::kNoHitKey;
                mask[u] = spo::band_mask(y0, y1, y + 64 * u);
                row_hits[u] = 0;
            }
#pragma unroll
            for (int f = 0; f < kOccWaveFrames; f++) {
                unsigned long long v[kOccUnroll];
#pragma unroll
                for (int u = 0; u < kOccUnroll; u++) v[u] = col[f][yl + 64 * u <= last ? yl + 64 * u : last];
#pragma unroll
                for (int u = 0; u < kOccUnroll; u++) {
                    const bool h = spo::hit(v[u], tkey[u]) && live[f];
                    row_hits[u] += h ? 1u : 0u;
                    if (want_frames) band_hits[f] += spo::popcount(__ballot(h) & mask[u]);
                }
            }
            if (want_rows) {
#pragma unroll
                for (int u = 0; u < kOccUnroll; u++)
                    if (row_hits[u])   // (not 0 only for a row of the tile)
                        (void)__hip_atomic_fetch_add(&s_rows[yl + 64 * u - r0], row_hits[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
        if (want_frames && lane < count) {
#pragma unroll
            for (int f = 0; f < kOccWaveFrames; f++) s_frames[lane * kOccFramePitch + wave + f * kOccWaves] = band_hits[f];
        }
    }
    __syncthreads();

    if (want_rows)
        for (int i = tid; i < r1 - r0; i += kOccThreads) {
            const uint32_t c = s_rows[i];
            if (c) (void)__hip_atomic_fetch_add(&rows[r0 + i], c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    if (want_frames)
        for (int i = tid; i < count * kOccFrames; i += kOccThreads) {
            const int b = i / kOccFrames, t = i % kOccFrames;
            if (first + t < frames) {   // (a frame of the piece that exists was stored by its wave)
                const uint32_t c = s_frames[b * kOccFramePitch + t];
                if (c) (void)__hip_atomic_fetch_add(&out[(size_t)b * (size_t)stride + (size_t)(x_base + first + t)], c, __ATOMIC_RELAXED,
                                                    __HIP_MEMORY_SCOPE_AGENT);
            }
        }
}

}  // namespace spk
