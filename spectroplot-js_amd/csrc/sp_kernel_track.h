// sp_kernel_track.h — the peak track (include/spectroplot_hip.h, sp_plan_execute_track): per band [y0_b, y1_b) of image rows and per
// frame x the strongest row of power[x][y] and its value, row[b][x] and peak[b][x].  The decision is sp_track_core.h's and nothing
// else's: keys (bit patterns without the sign bit) compared as unsigned integers, the smaller row among equal keys, a NaN no
// candidate.  A maximum with a fixed tie rule commutes, so the result does not depend on the order of the rows, on the grid or on how
// the plane is cut into blocks of frames.
//
// One launch, no global workspace, no atomics and no floating-point compare: a frame's best is made inside one wave and stored.
#pragma once

#include <hip/hip_runtime.h>

#include "sp_band_list.h"   // the bands travel as they do for k_band_sum
#include "sp_track_core.h"

namespace spk {

constexpr int kTrackFrames = 8;      // frames of a workgroup: one result slot in LDS each, and one storing thread each.  (Few, as for
                                     // k_band_sum, so that a screen-wide request still fills the chip.)
constexpr int kTrackWaves = 4;       // waves of a workgroup: wave w takes the frames w, w + 4, ... of its piece
constexpr int kTrackThreads = 64 * kTrackWaves;
constexpr int kTrackUnroll = 8;      // loads of 64 rows a wave has in flight

// The candidate lane (l op CTRL) holds, through DPP: both halves of the 64-bit key and the row travel together, from the same lane.
// Every lane of the wave must be here.
template <int CTRL>
__device__ inline void track_take(spt::Best &best)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)best.key, CTRL, 0xf, 0xf, false);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(best.key >> 32), CTRL, 0xf, 0xf, false);
    const int32_t row = __builtin_amdgcn_update_dpp(0, best.row, CTRL, 0xf, 0xf, false);
    spt::merge(best, ((uint64_t)hi << 32) | lo, row);
}

// The best of the wave's 64 running bests, the same in every lane.  Four DPP exchanges make the best of every row of 16 lanes in
// all of its lanes (lane ^ 1, lane ^ 2, then the other quad of eight and the other eight of sixteen through the two mirrors, which
// reach a lane of the other half whatever it holds: the halves are uniform by then); the four rows' bests are read into the scalar
// unit and merged there.  better() is a total order on candidates with distinct rows, so both lanes of an exchange agree.
__device__ inline spt::Best track_wave_best(spt::Best best)
{
    track_take<0xB1>(best);    // quad_perm:[1,0,3,2]
    track_take<0x4E>(best);    // quad_perm:[2,3,0,1]
    track_take<0x141>(best);   // row_half_mirror
    track_take<0x140>(best);   // row_mirror
    spt::Best all;
#pragma unroll
    for (int r = 0; r < 64; r += 16) {
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)best.key, r);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(best.key >> 32), r);
        spt::merge(all, ((uint64_t)hi << 32) | lo, __builtin_amdgcn_readlane(best.row, r));
    }
    return all;
}

// row[b * stride + x_base + x] and peak[...] for the frames x in [0, frames) of the frame-major plane at `plane` (frame x, row y at
// plane[x * n + y]) and every band b of the list; either output may be null and is not written then.  grid = (pieces of kTrackFrames
// frames, bands), 256 threads.  Wave w reads the band's rows of the frames w, w + 4, ... 64 rows at a time, 512 contiguous bytes per
// load, kTrackUnroll loads in flight; a lane keeps its running best over its rows, which ascend; the wave's best goes to the frame's
// slot in LDS.  Behind a barrier thread t < kTrackFrames stores frame t's row and value: neighbouring elements of both arrays.
__global__ __launch_bounds__(kTrackThreads) void k_track_max(const double *__restrict__ plane, const int n, const long long frames,
                                                             const BandList bands, int32_t *__restrict__ row, double *__restrict__ peak,
                                                             const long long stride, const long long x_base)
{
    __shared__ unsigned long long s_peak[kTrackFrames];
    __shared__ int32_t s_row[kTrackFrames];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int y0 = bands.y[2 * blockIdx.y], y1 = bands.y[2 * blockIdx.y + 1];
    const long long first = (long long)blockIdx.x * kTrackFrames;
    for (int t = wave; t < kTrackFrames && first + t < frames; t += kTrackWaves) {
        // (64-bit: 8 * width * n passes 4 GiB)
        const unsigned long long *const col = (const unsigned long long *)plane + (size_t)(first + t) * (size_t)n;
        spt::Best best;
        // (unsigned: y1 may be 2^31 - 1, and a load's last row number must not wrap)
        for (unsigned y = (unsigned)y0; y < (unsigned)y1; y += 64u * kTrackUnroll) {   // (wave-uniform)
            // Every load is issued, none under a branch: a row at or past y1 reads the band's last row instead (y1 - 1 >= y0: the band
            // is not empty here) and is dropped behind the loads, so kTrackUnroll loads are in flight before the first compare.
            const unsigned yl = y + (unsigned)lane, last = (unsigned)y1 - 1u;
            unsigned long long v[kTrackUnroll];
#pragma unroll
            for (unsigned u = 0; u < (unsigned)kTrackUnroll; u++) v[u] = col[yl + 64u * u <= last ? yl + 64u * u : last];
#pragma unroll
            for (unsigned u = 0; u < (unsigned)kTrackUnroll; u++) {
                const unsigned yu = yl + 64u * u;
                spt::fold(best, yu <= last ? spt::key_of(v[u]) : spt::kNanKey, (int32_t)yu);   // (a row outside the band is no candidate)
            }
        }
        best = track_wave_best(best);
        if (lane == 0) {
            s_peak[t] = spt::peak_bits_of(best);
            s_row[t] = spt::row_of(best);
        }
    }
    __syncthreads();
    if (tid < kTrackFrames && first + tid < frames) {
        const size_t at = (size_t)blockIdx.y * (size_t)stride + (size_t)(x_base + first + tid);
        if (row) row[at] = s_row[tid];
        if (peak) peak[at] = __longlong_as_double((long long)s_peak[tid]);
    }
}

}  // namespace spk
