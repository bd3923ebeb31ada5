// sp_kernel_variance.h — the exact variance and spectral-kurtosis traces (include/spectroplot_hip.h, sp_plan_execute_variance): per row
// RN(sum p), RN(sum p^2) and RN(W * sum p^2 - (sum p)^2) over the request's W frames.  The sums are sp_variance_core.h's: every |X|^2
// is cut into three 32-bit pieces and its exact square into five, and all eight are added into 64-bit cells with INTEGER adds, which
// commute - the result does not depend on the deal of frames to workgroups, on the grid or on the order in which the atomics land.
// There is no floating-point operation anywhere in the reduction or in the subtraction.
//
// The workspace is u64[spv::kSlots][n], slot-major: the 66 cells of every row's sum, the 132 cells of its sum of squares, then the
// rows' NaN counts and +inf counts.  It is zero before a request's first accumulate.
#pragma once

#include <hip/hip_runtime.h>

#include "sp_variance_core.h"

namespace spk {

// k_mean_accumulate's shape with HALF its rows: 200 slots of 64 rows would be 100 KiB of LDS, one workgroup per CU; 32 rows are 50 KiB,
// three workgroups (twelve waves) per CU of gfx950's 160 KiB.  A wave covers the 32 rows of two neighbouring
// frames: two runs of 256 contiguous bytes.
constexpr int kVarRows = 32;        // rows of a workgroup's band: lane & 31
constexpr int kVarFrames = 8;       // frames a workgroup reads side by side: tid / 32 (two to a wave, four waves)
constexpr int kVarThreads = kVarRows * kVarFrames;
constexpr int kVarUnroll = 4;       // loads a thread has in flight: 32 frames of a piece per round

// frame pieces of a launch over `frames` frames of n rows: two rounds of three workgroups per CU, no piece below 32 frames
__host__ __device__ inline int variance_bands(int n) { return (n + kVarRows - 1) / kVarRows; }
inline int variance_pieces(int n, long long frames, int cu_count)
{
    long long pieces = (6ll * cu_count + variance_bands(n) - 1) / variance_bands(n);
    const long long most = (frames + 31) / 32;
    if (pieces > most) pieces = most;
    return (int)(pieces < 1 ? 1 : pieces);
}

// Adds the frames [0, frames) of the frame-major plane at `plane` (frame x, row y at plane[x * n + y]) into the workspace: every value
// is read ONCE and gives both its pieces and its square's.  grid = (bands, pieces): workgroup (b, p) owns the rows [32 b, 32 b + 32)
// and the frames [p * per, p * per + per).  Its cells live in LDS, [slot][row], shared by its threads through LDS integer atomics; at
// the end every non-zero cell goes to the workspace in one 64-bit global integer atomic.  A request's values occupy a few neighbouring
// cells, so nearly every cell is zero and is skipped.
__global__ __launch_bounds__(kVarThreads) void k_variance_accumulate(const double *__restrict__ plane, const int n, const long long frames,
                                                                     const long long per, unsigned long long *__restrict__ ws)
{
    __shared__ unsigned long long cells[spv::kSlots][kVarRows];
    const int tid = threadIdx.x, lane = tid & (kVarRows - 1), sub = tid / kVarRows;
    for (int k = tid; k < spv::kSlots * kVarRows; k += kVarThreads) (&cells[0][0])[k] = 0;
    __syncthreads();

    const int row = (int)blockIdx.x * kVarRows + lane;
    const long long first = (long long)blockIdx.y * per;
    const long long end = first + per < frames ? first + per : frames;
    if (row < n) {
        const unsigned long long *const col = (const unsigned long long *)plane + row;
        for (long long x = first + sub; x < end; x += kVarFrames * kVarUnroll) {
            unsigned long long v[kVarUnroll];
            bool have[kVarUnroll];
#pragma unroll
            for (int u = 0; u < kVarUnroll; u++) {
                const long long xu = x + (long long)u * kVarFrames;
                have[u] = xu < end;
                v[u] = have[u] ? col[(size_t)xu * (size_t)n] : 0ull;   // (64-bit: 8 * width * n passes 4 GiB)
            }
#pragma unroll
            for (int u = 0; u < kVarUnroll; u++) {
                if (!have[u]) continue;
                int cell;
                uint32_t p[3], q[5];
                const int kind = spx::decompose(v[u], cell, p);
                if (kind == spx::kFinite) {
                    // cell + 2 <= 65 and, for the squares, cell + 4 <= 131: in bounds for every exponent field
                    if (p[0]) atomicAdd(&cells[spv::kSumSlot + cell][lane], (unsigned long long)p[0]);
                    if (p[1]) atomicAdd(&cells[spv::kSumSlot + cell + 1][lane], (unsigned long long)p[1]);
                    if (p[2]) atomicAdd(&cells[spv::kSumSlot + cell + 2][lane], (unsigned long long)p[2]);
                    spv::decompose_squared(v[u], cell, q);
#pragma unroll
                    for (int j = 0; j < 5; j++)
                        if (q[j]) atomicAdd(&cells[spv::kSquareSlot + cell + j][lane], (unsigned long long)q[j]);
                } else {
                    atomicAdd(&cells[kind == spx::kNan ? spv::kNanSlot : spv::kInfSlot][lane], 1ull);
                }
            }
        }
    }
    __syncthreads();
    if (row < n) {
        for (int k = sub; k < spv::kSlots; k += kVarFrames) {
            const unsigned long long c = cells[k][lane];
            if (c) atomicAdd(&ws[(size_t)k * (size_t)n + (size_t)row], c);
        }
    }
}

// out[0][y], out[1][y], out[2][y] = the row's three results (spv::finish_row) with the NaN and inf rule, one thread per row; width == 0
// finds a workspace of zeros and writes three times +0.0.
__global__ void k_variance_finish(const unsigned long long *__restrict__ ws, const int n, const int width, double *__restrict__ out)
{
    const int y = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (y >= n) return;
    uint64_t r[3];
    spv::finish_row((const uint64_t *)ws + y, (size_t)n, (uint32_t)width, r);
    for (int k = 0; k < 3; k++) out[(size_t)k * (size_t)n + (size_t)y] = __longlong_as_double((long long)r[k]);
}

}  // namespace spk
