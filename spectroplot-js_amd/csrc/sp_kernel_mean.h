// sp_kernel_mean.h — the exact mean-power trace (include/spectroplot_hip.h, sp_plan_execute_mean): mean[y] = RN(exact sum over x of
// power[x][y]) / width.  The sum is sp_exact_sum.h's: every |X|^2 is cut into three 32-bit pieces and added into 64-bit cells with
// INTEGER adds, which commute - the result does not depend on the deal of frames to workgroups, on the grid or on the order in which the
// atomics land.  There is no floating-point add anywhere in the reduction.
//
// The workspace is u64[spx::kSlots][n], slot-major: cells 0 .. 65 of every row, then the rows' NaN counts and +inf counts.  A wave's
// atomic instruction on one slot covers 64 neighbouring rows, 512 contiguous bytes.  It is zero before a request's first accumulate.
#pragma once

#include <hip/hip_runtime.h>

#include "sp_exact_sum.h"

namespace spk {

constexpr int kMeanRows = 64;       // rows of a workgroup's band: one per lane, so a wave reads 512 contiguous bytes per frame
constexpr int kMeanWaves = 4;       // waves of a workgroup: wave w takes the frames first + w, first + w + 4, ... of its piece
constexpr int kMeanThreads = kMeanRows * kMeanWaves;
constexpr int kMeanUnroll = 4;      // frames a wave has in flight

// frame pieces of a launch over `frames` frames of n rows: enough workgroups for a few per CU, no piece below 32 frames
__host__ __device__ inline int mean_bands(int n) { return (n + kMeanRows - 1) / kMeanRows; }
inline int mean_pieces(int n, long long frames, int cu_count)
{
    long long pieces = (4ll * cu_count + mean_bands(n) - 1) / mean_bands(n);
    const long long most = (frames + 31) / 32;
    if (pieces > most) pieces = most;
    return (int)(pieces < 1 ? 1 : pieces);
}

// Adds the frames [0, frames) of the frame-major plane at `plane` (frame x, row y at plane[x * n + y]) into the workspace.
// grid = (bands, pieces): workgroup (b, p) owns the rows [64 b, 64 b + 64) and the frames [p * per, p * per + per).  Its cells live in
// LDS, [slot][row], shared by its waves through LDS integer atomics; at the end every non-zero cell goes to the workspace in one 64-bit
// global integer atomic.  A request's values occupy a few neighbouring cells, so nearly every cell is zero and is skipped.
__global__ __launch_bounds__(kMeanThreads) void k_mean_accumulate(const double *__restrict__ plane, const int n, const long long frames,
                                                                  const long long per, unsigned long long *__restrict__ ws)
{
    __shared__ unsigned long long cells[spx::kSlots][kMeanRows];
    const int tid = threadIdx.x, lane = tid & (kMeanRows - 1), wave = tid / kMeanRows;
    for (int k = tid; k < spx::kSlots * kMeanRows; k += kMeanThreads) (&cells[0][0])[k] = 0;
    __syncthreads();

    const int row = (int)blockIdx.x * kMeanRows + lane;
    const long long first = (long long)blockIdx.y * per;
    const long long end = first + per < frames ? first + per : frames;
    if (row < n) {
        const unsigned long long *const col = (const unsigned long long *)plane + row;
        for (long long x = first + wave; x < end; x += kMeanWaves * kMeanUnroll) {
            unsigned long long v[kMeanUnroll];
            bool have[kMeanUnroll];
#pragma unroll
            for (int u = 0; u < kMeanUnroll; u++) {
                const long long xu = x + (long long)u * kMeanWaves;
                have[u] = xu < end;
                v[u] = have[u] ? col[(size_t)xu * (size_t)n] : 0ull;   // (64-bit: 8 * width * n passes 4 GiB)
            }
#pragma unroll
            for (int u = 0; u < kMeanUnroll; u++) {
                if (!have[u]) continue;
                int cell;
                uint32_t p[3];
                const int kind = spx::decompose(v[u], cell, p);
                if (kind == spx::kFinite) {
                    // cell + 2 <= 65: in bounds for every exponent field
                    if (p[0]) atomicAdd(&cells[cell][lane], (unsigned long long)p[0]);
                    if (p[1]) atomicAdd(&cells[cell + 1][lane], (unsigned long long)p[1]);
                    if (p[2]) atomicAdd(&cells[cell + 2][lane], (unsigned long long)p[2]);
                } else {
                    atomicAdd(&cells[kind == spx::kNan ? spx::kNanSlot : spx::kInfSlot][lane], 1ull);
                }
            }
        }
    }
    __syncthreads();
    if (row < n) {
        for (int k = wave; k < spx::kSlots; k += kMeanWaves) {
            const unsigned long long c = cells[k][lane];
            if (c) atomicAdd(&ws[(size_t)k * (size_t)n + (size_t)row], c);
        }
    }
}

// mean[y] = RN(the row's exact sum) / width with the NaN and inf rule, one thread per row; width == 0 gives 0 / 0 = NaN.
__global__ void k_mean_finish(const unsigned long long *__restrict__ ws, const int n, const int width, double *__restrict__ mean)
{
    const int y = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (y >= n) return;
    spx::Finisher f;
    for (int k = 0; k < spx::kCells; k++) f.push(ws[(size_t)k * (size_t)n + (size_t)y]);
    const unsigned long long bits =
        spx::apply_specials(f.result(), ws[(size_t)spx::kNanSlot * (size_t)n + (size_t)y], ws[(size_t)spx::kInfSlot * (size_t)n + (size_t)y]);
    mean[y] = __longlong_as_double((long long)bits) / (double)width;
}

}  // namespace spk
