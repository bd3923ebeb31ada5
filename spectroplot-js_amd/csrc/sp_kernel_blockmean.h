// sp_kernel_blockmean.h — the averaged spectrogram (include/spectroplot_hip.h, sp_plan_execute_blockmean): out[c][y] = RN(exact sum of
// power[x][y] over column c's frames) / count_c, and the colouring of a power plane (sp_plan_power_to_index).
//
// k_blockmean is the DIRECT path (sp_blockmean_core.h): whole columns of `group` frames, each made inside one workgroup - k_band_sum's
// "cells in LDS, finished in the workgroup, no global workspace" turned by 90 degrees, with k_mean_accumulate's accumulation.  The sum
// is sp_exact_sum.h's: integer adds only, which commute, so the result does not depend on the deal of frames to waves or of columns to
// workgroups, and it is bit for bit what the carried path (k_mean_accumulate, k_mean_finish) makes of the same frames.  There is no
// floating-point add or compare, no global atomic, and no workgroup waits for another.
#pragma once

#include <hip/hip_runtime.h>

#include "sp_blockmean_core.h"
#include "sp_exact_sum.h"

namespace spk {

// k_mean_accumulate's shape (sp_kernel_mean.h, which this unit does not include: its kernels are sp_kernels.hip's)
constexpr int kBlockMeanRows = 64;      // rows of a workgroup's band: one per lane, so a wave reads 512 contiguous bytes per frame
constexpr int kBlockMeanWaves = 4;      // waves of a workgroup: wave w takes the frames first + w, first + w + 4, ... of a column
constexpr int kBlockMeanThreads = kBlockMeanRows * kBlockMeanWaves;
constexpr int kBlockMeanUnroll = 4;     // frames a wave has in flight (kMeanUnroll)

// Columns [0, columns) of `group` frames each of the frame-major plane at `plane` (frame x, row y at plane[x * n + y]; `frames` frames,
// so only the last column can be short) into out[c * n + y].  grid = (bands of 64 rows, pieces of the columns), 256 threads: workgroup
// (b, p) owns the rows [64 b, 64 b + 64), one per lane, and the columns [p * per, p * per + per), one after the other.  Its cells are
// u64[spx::kSlots][64] in LDS, 34 816 bytes, zeroed once.  Per column: wave w adds the frames w, w + 4, ... of the column, 512
// contiguous bytes per frame and kBlockMeanUnroll loads in flight, with LDS integer adds that skip zero pieces; behind a barrier
// thread t < 64 pushes its row's cells through the Finisher, applies the specials, divides by the column's count and stores: 512
// contiguous bytes per column.
// A column of a few frames touches a few neighbouring cells of the 66, so every thread remembers the lowest and the highest cell it
// added to and folds them into its row's range in LDS (an integer minimum and maximum: no order).  The finishing thread pushes that
// range alone - the cells below it are zero, which is the Finisher's state at count = lo, and the zero cells above it change nothing
// it remembers - and puts the cells it read back to zero: that is the next column's clear.  The ranges are two sets, taken in turn,
// so that a set is reset a whole column before it is used again.
__global__ __launch_bounds__(kBlockMeanThreads) void k_blockmean(const double *__restrict__ plane, const int n, const long long frames,
                                                                 const long long group, const long long columns, const long long per,
                                                                 double *__restrict__ out)
{
    __shared__ unsigned long long cells[spx::kSlots][kBlockMeanRows];
    __shared__ int range_lo[2][kBlockMeanRows], range_hi[2][kBlockMeanRows];
    const int tid = threadIdx.x, lane = tid & (kBlockMeanRows - 1), wave = __builtin_amdgcn_readfirstlane(tid / kBlockMeanRows);
    const int row = (int)blockIdx.x * kBlockMeanRows + lane;
    const bool live = row < n;
    const unsigned long long *const col = (const unsigned long long *)plane + (live ? row : 0);
    for (int k = tid; k < spx::kSlots * kBlockMeanRows; k += kBlockMeanThreads) (&cells[0][0])[k] = 0;
    if (tid < kBlockMeanRows) {
        range_lo[0][tid] = range_lo[1][tid] = spx::kCells;
        range_hi[0][tid] = range_hi[1][tid] = -1;
    }
    __syncthreads();

    const long long c_first = (long long)blockIdx.y * per;
    const long long c_end = c_first + per < columns ? c_first + per : columns;
    for (long long c = c_first; c < c_end; c++) {   // (workgroup-uniform)
        const int set = (int)((c - c_first) & 1);
        const long long first = c * group;
        const long long end = first + group < frames ? first + group : frames;
        int lo = spx::kCells, hi = -1;
        for (long long x = first + wave; x < end; x += kBlockMeanWaves * kBlockMeanUnroll) {   // (wave-uniform)
            unsigned long long v[kBlockMeanUnroll];
            bool have[kBlockMeanUnroll];
#pragma unroll
            for (int u = 0; u < kBlockMeanUnroll; u++) {
                const long long xu = x + (long long)u * kBlockMeanWaves;
                have[u] = live && xu < end;
                v[u] = have[u] ? col[(size_t)xu * (size_t)n] : 0ull;   // (64-bit: 8 * width * n passes 4 GiB)
            }
#pragma unroll
            for (int u = 0; u < kBlockMeanUnroll; u++) {
                if (!have[u]) continue;
                int cell;
                uint32_t p[3];
                const int kind = spx::decompose(v[u], cell, p);
                if (kind == spx::kFinite) {
                    // cell + 2 <= 65: in bounds for every exponent field
                    if (p[0]) atomicAdd(&cells[cell][lane], (unsigned long long)p[0]);
                    if (p[1]) atomicAdd(&cells[cell + 1][lane], (unsigned long long)p[1]);
                    if (p[2]) atomicAdd(&cells[cell + 2][lane], (unsigned long long)p[2]);
                    if (p[0] | p[1] | p[2]) {
                        lo = cell < lo ? cell : lo;
                        hi = cell + 2 > hi ? cell + 2 : hi;
                    }
                } else {
                    atomicAdd(&cells[kind == spx::kNan ? spx::kNanSlot : spx::kInfSlot][lane], 1ull);
                }
            }
        }
        if (hi >= 0) {
            atomicMin(&range_lo[set][lane], lo);
            atomicMax(&range_hi[set][lane], hi);
        }
        __syncthreads();
        if (tid < kBlockMeanRows) {   // (a row past n has added nothing: its range is empty and its cells are zero)
            const int k0 = range_lo[set][lane], k1 = range_hi[set][lane];
            spx::Finisher f;
            f.count = k1 >= 0 ? k0 : 0;   // (k0 zero digits have gone before: the state is the initial one)
            for (int k = k0; k <= k1; k++) {
                f.push(cells[k][lane]);
                cells[k][lane] = 0;
            }
            const unsigned long long nans = cells[spx::kNanSlot][lane], infs = cells[spx::kInfSlot][lane];
            cells[spx::kNanSlot][lane] = 0;
            cells[spx::kInfSlot][lane] = 0;
            const unsigned long long bits = spx::apply_specials(f.result(), nans, infs);
            if (live) out[(size_t)c * (size_t)n + (size_t)row] = __longlong_as_double((long long)bits) / (double)(end - first);
            range_lo[set ^ 1][lane] = spx::kCells;   // (the other set: read a column ago, used again a column from now)
            range_hi[set ^ 1][lane] = -1;
        }
        __syncthreads();   // (the next column adds to the cells the finishing threads have just put back to zero)
    }
}

constexpr int kIndexTile = 64;   // rows and frames of a tile of k_power_to_index
constexpr int kIndexThreads = 256;

// index[j] = spbm::gray_index of power[x * n + y] against the plan's `lut_len` <= 256 colour edges, at the pixel position of "Indexed
// image replies": j = x + width * y (spectrogram layout) or j = n * (width - 1 - x) + (n - 1 - y) (waterfall layout).
// grid = (tiles of 64 frames, bands of 64 rows), 256 threads.  Wave w reads the frames w, w + 4, ... of the tile, lane l row l of the
// band: 512 contiguous bytes.  In the waterfall layout a frame is a run of n bytes, reversed, and the wave stores 64 contiguous bytes
// at once.  In the spectrogram layout neighbouring bytes are neighbouring FRAMES: the tile's indices go through LDS (a row of 64 bytes
// padded to 68, so that the column a wave writes spreads over the banks) and behind a barrier wave w stores the rows w, w + 4, ...,
// lane l frame l: 64 contiguous bytes again.  The edges' bit patterns lie in LDS for the binary search.
__global__ __launch_bounds__(kIndexThreads) void k_power_to_index(const double *__restrict__ power, const int n, const int width,
                                                                  const int waterfall, const double *__restrict__ gray_edge,
                                                                  const int lut_len, uint8_t *__restrict__ index)
{
    __shared__ uint64_t edges[256];
    __shared__ uint8_t tile[kIndexTile][kIndexTile + 4];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    edges[tid] = tid < lut_len ? ((const uint64_t *)gray_edge)[tid] : ~(uint64_t)0;
    __syncthreads();

    const long long x0 = (long long)blockIdx.x * kIndexTile;
    const int y = (int)blockIdx.y * kIndexTile + lane;
    const bool row_live = y < n;
    const unsigned long long *const col = (const unsigned long long *)power + (row_live ? y : 0);
    for (int t = wave; t < kIndexTile; t += kIndexThreads / 64) {   // (wave-uniform)
        const long long x = x0 + t;
        if (x >= width) break;
        const bool have = row_live;
        const unsigned long long v = have ? col[(size_t)x * (size_t)n] : 0ull;   // (64-bit: 8 * width * n passes 4 GiB)
        const uint8_t g = (uint8_t)spbm::gray_index(edges, lut_len, v);
        if (waterfall) {
            if (have) index[(size_t)n * (size_t)(width - 1 - x) + (size_t)(n - 1 - y)] = g;
        } else {
            tile[lane][t] = g;
        }
    }
    if (waterfall) return;   // (workgroup-uniform)
    __syncthreads();
    const long long x = x0 + lane;
    for (int r = wave; r < kIndexTile; r += kIndexThreads / 64) {   // (wave-uniform)
        const int yr = (int)blockIdx.y * kIndexTile + r;
        if (yr >= n) break;
        if (x < width) index[(size_t)x + (size_t)width * (size_t)yr] = tile[r][lane];
    }
}

}  // namespace spk
