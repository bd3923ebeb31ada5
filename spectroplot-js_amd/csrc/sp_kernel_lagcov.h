// sp_kernel_lagcov.h — the exact lagged covariances of band-power series (include/spectroplot_hip.h, sp_plan_execute_lagcov): per pair
// (a, b) of series and lag l RN(sum a[x] b[x + l]), RN(N * sum a[x] b[x + l] - sum a[x] * sum b[x + l]) and RN(sum b[x + l]) over the
// N = width - lags + 1 terms every lag has.  The sums are sp_lagcov_core.h's: every b[x + l] is cut into three 32-bit pieces and the
// exact product a[x] * b[x + l] into five, and all eight are added into 64-bit cells with INTEGER adds, which commute - the result
// does not depend on the deal of terms to workgroups, on the grid or on the order in which the atomics land.  There is no
// floating-point operation anywhere in the reduction or in the subtraction.
//
// The workspace is u64[spl::kSlots][npairs * lags], slot-major - per (pair, lag) the 66 cells of B, the 132 cells of P and the NaN and
// +inf counts of its terms' operands - and behind it u64[npairs][spl::kPairCells], the cells of every pair's A.  It is zero before a
// request's accumulate.
#pragma once

#include <hip/hip_runtime.h>

#include "sp_lagcov_core.h"

namespace spk {

// k_variance_accumulate's shape with the ROW replaced by the LAG: 200 slots of 32 lags are 50 KiB of LDS, three workgroups (twelve
// waves) per CU of gfx950's 160 KiB (DESIGN.md sections 25 and 26).  The 32 lanes of a stream read ONE a[x] and 256 contiguous bytes
// of b.
constexpr int kLagLanes = 32;       // lags of a workgroup's band: lane & 31
constexpr int kLagStreams = 8;      // terms a workgroup reads side by side: tid / 32 (two to a wave, four waves)
constexpr int kLagThreads = kLagLanes * kLagStreams;
constexpr int kLagUnroll = 4;       // loads a thread has in flight: 32 terms of a piece per round

// the (ia, ib) of a launch's pairs: they travel in the kernel's arguments
struct LagPairs {
    int32_t v[2 * spl::kMaxPairs];
};

// pieces of a launch over `terms` terms: two rounds of three workgroups per CU, no piece below 32 terms
__host__ __device__ inline int lagcov_lag_bands(int lags) { return (lags + kLagLanes - 1) / kLagLanes; }
inline int lagcov_pieces(int npairs, int lags, long long terms, int cu_count)
{
    const long long bands = (long long)npairs * lagcov_lag_bands(lags);
    long long pieces = (6ll * cu_count + bands - 1) / bands;
    const long long most = (terms + 31) / 32;
    if (pieces > most) pieces = most;
    return (int)(pieces < 1 ? 1 : pieces);
}

// Adds the terms [0, terms) of every pair and lag into the workspace; `series` is band-major, band i's frames at series + i * width,
// and terms + lags - 1 <= width: the last frame read is b[terms - 1 + lags - 1].  grid = (npairs * lag bands, pieces): workgroup
// (g, q) owns pair g / lag bands, the lags [32 (g % lag bands), + 32) and the terms [q * per, q * per + per).  Its cells live in LDS,
// [slot][lag], shared by its threads through LDS integer atomics; at the end every non-zero cell goes to the workspace in one 64-bit
// global integer atomic.  No load is made past the piece's end, and none for a lag at or beyond `lags`.  A's pieces are added by the
// pair's FIRST lag band alone, piece j by lane j of the stream that read the term: once per pair and term.
__global__ __launch_bounds__(kLagThreads) void k_lagcov_accumulate(const double *__restrict__ series, const long long width, const LagPairs pairs,
                                                                   const int lags, const long long terms, const long long per,
                                                                   unsigned long long *__restrict__ ws, unsigned long long *__restrict__ aws)
{
    __shared__ unsigned long long cells[spl::kSlots][kLagLanes];
    __shared__ unsigned long long acells[spl::kPairCells];
    const int tid = threadIdx.x, lane = tid & (kLagLanes - 1), sub = tid / kLagLanes;
    for (int k = tid; k < spl::kSlots * kLagLanes; k += kLagThreads) (&cells[0][0])[k] = 0;
    if (tid < spl::kPairCells) acells[tid] = 0;
    __syncthreads();

    const int lag_bands = lagcov_lag_bands(lags);
    const int pair = (int)blockIdx.x / lag_bands, band = (int)blockIdx.x % lag_bands;
    const int lag = band * kLagLanes + lane;
    const bool live = lag < lags;
    const long long first = (long long)blockIdx.y * per;
    const long long end = first + per < terms ? first + per : terms;
    const unsigned long long *const sa = (const unsigned long long *)series + (size_t)pairs.v[2 * pair] * (size_t)width;
    const unsigned long long *const sb = (const unsigned long long *)series + (size_t)pairs.v[2 * pair + 1] * (size_t)width + (live ? lag : 0);
    for (long long x = first + sub; x < end; x += kLagStreams * kLagUnroll) {
        unsigned long long va[kLagUnroll], vb[kLagUnroll];
        bool have[kLagUnroll];
#pragma unroll
        for (int u = 0; u < kLagUnroll; u++) {
            const long long xu = x + (long long)u * kLagStreams;
            have[u] = xu < end;
            va[u] = have[u] ? sa[xu] : 0ull;
            vb[u] = have[u] && live ? sb[xu] : 0ull;   // (xu + lag <= terms - 1 + lags - 1 <= width - 1)
        }
#pragma unroll
        for (int u = 0; u < kLagUnroll; u++) {
            if (!have[u]) continue;
            int ca, cb, cp;
            uint32_t pa[3], pb[3], q[5];
            const int ka = spx::decompose(va[u], ca, pa);
            if (band == 0 && lane < 3 && ka == spx::kFinite) {
                // ca + 2 <= 65: in bounds for every exponent field
                const uint32_t piece = lane == 0 ? pa[0] : lane == 1 ? pa[1] : pa[2];
                if (piece) atomicAdd(&acells[ca + lane], (unsigned long long)piece);
            }
            if (!live) continue;
            const int kb = spx::decompose(vb[u], cb, pb);
            if (ka != spx::kFinite) atomicAdd(&cells[ka == spx::kNan ? spv::kNanSlot : spv::kInfSlot][lane], 1ull);
            if (kb != spx::kFinite) atomicAdd(&cells[kb == spx::kNan ? spv::kNanSlot : spv::kInfSlot][lane], 1ull);
            else {
                // cb + 2 <= 65 and, for the products, cp + 4 <= 131
                if (pb[0]) atomicAdd(&cells[spv::kSumSlot + cb][lane], (unsigned long long)pb[0]);
                if (pb[1]) atomicAdd(&cells[spv::kSumSlot + cb + 1][lane], (unsigned long long)pb[1]);
                if (pb[2]) atomicAdd(&cells[spv::kSumSlot + cb + 2][lane], (unsigned long long)pb[2]);
            }
            // (a zero operand has no pieces: (bits << 1) == 0 is +0.0 or -0.0)
            if (ka == spx::kFinite && kb == spx::kFinite && (va[u] << 1) && (vb[u] << 1)) {
                spl::decompose_product(va[u], vb[u], cp, q);
#pragma unroll
                for (int j = 0; j < 5; j++)
                    if (q[j]) atomicAdd(&cells[spv::kSquareSlot + cp + j][lane], (unsigned long long)q[j]);
            }
        }
    }
    __syncthreads();
    if (live) {
        const size_t total = (size_t)gridDim.x / (size_t)lag_bands * (size_t)lags;   // npairs * lags
        const size_t at = (size_t)pair * (size_t)lags + (size_t)lag;
        for (int k = sub; k < spl::kSlots; k += kLagStreams) {
            const unsigned long long c = cells[k][lane];
            if (c) atomicAdd(&ws[(size_t)k * total + at], c);
        }
    }
    if (band == 0 && tid < spl::kPairCells) {
        const unsigned long long c = acells[tid];
        if (c) atomicAdd(&aws[(size_t)pair * spl::kPairCells + tid], c);
    }
}

// out[0][p][l], out[1][p][l], out[2][p][l] = the three results of pair p and lag l (spl::finish_row) with the NaN and inf rule, one
// thread per (p, l); terms == 0 finds a workspace of zeros and writes three times +0.0.
__global__ void k_lagcov_finish(const unsigned long long *__restrict__ ws, const unsigned long long *__restrict__ aws, const int npairs,
                                const int lags, const int terms, double *__restrict__ out)
{
    const int at = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const int total = npairs * lags;
    if (at >= total) return;
    uint64_t r[3];
    spl::finish_row((const uint64_t *)ws + at, (size_t)total, (const uint64_t *)aws + (size_t)(at / lags) * spl::kPairCells, 1, (uint32_t)terms,
                    r);
    for (int k = 0; k < 3; k++) out[(size_t)k * (size_t)total + (size_t)at] = __longlong_as_double((long long)r[k]);
}

}  // namespace spk
