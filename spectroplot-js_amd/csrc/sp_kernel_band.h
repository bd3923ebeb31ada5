// sp_kernel_band.h — the exact band-power series (include/spectroplot_hip.h, sp_plan_execute_bandpower): band[b][x] = RN(exact sum
// over the image rows y in [y0_b, y1_b) of power[x][y]).  The sum is sp_exact_sum.h's, as for the mean (sp_kernel_mean.h), turned by
// 90 degrees: the mean adds along x into one accumulator per row, this adds along y into one accumulator per frame.  Integer adds only,
// so the result does not depend on the order of the rows, on the grid or on how the plane is cut into blocks of frames.
//
// One launch, no global workspace: a frame's whole sum is made inside one workgroup, finished there and stored.
#pragma once

#include <hip/hip_runtime.h>

#include "sp_band_list.h"
#include "sp_exact_sum.h"

namespace spk {

constexpr int kBandFrames = 8;      // frames of a workgroup: one LDS column each, and one finishing thread each.  (Few, so that a
                                    // screen-wide request still fills the chip: a band has width / 8 workgroups and no more.)
constexpr int kBandWaves = 4;       // waves of a workgroup: wave w takes the frames w, w + 4, ... of its piece
constexpr int kBandThreads = 64 * kBandWaves;
constexpr int kBandUnroll = 4;      // loads of 64 rows a wave has in flight

// Lane 15 of every row of 16 lanes gets the row's sum (the other lanes a prefix of it); no overflow is looked after here.
__device__ inline uint32_t band_row_sum(uint32_t x)
{
#define SP_DPP_ADD(ctrl) x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, ctrl, 0xf, 0xf, false);
    SP_DPP_ADD(0x111)   // row_shr:1
    SP_DPP_ADD(0x112)   // row_shr:2
    SP_DPP_ADD(0x114)   // row_shr:4
    SP_DPP_ADD(0x118)   // row_shr:8
#undef SP_DPP_ADD
    return x;
}
// the sum of band_row_sum's four row sums, below 2^38 for addends below 2^32 each row
__device__ inline unsigned long long band_rows_total(uint32_t x)
{
    return (unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)x, 15) + (uint32_t)__builtin_amdgcn_readlane((int)x, 31) +
           (uint32_t)__builtin_amdgcn_readlane((int)x, 47) + (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
}

// Adds the wave's 64 values (lane l holds `bits` where `have`) into column t of the cells.  The column is the wave's own, but all 64
// values of a frame land in the few cells around the frame's level, and 64 LDS atomics on one address serialise.  So the wave folds
// first: it takes the cell number of the first lane that still has a value, sums the three pieces of every lane with that cell number
// across the wave in the VALU, and lanes 0 .. 2 add the three totals; those lanes retire and the loop goes on while a lane is left.
// A spectrum's values spend a few rounds; 64 values of 64 different cells spend 64.
// A piece is below 2^32 and a row of 16 lanes would pass 32 bits: the low 28 bits of the three pieces are summed apart from their
// high 4 bits, which travel packed in one word (three fields of 10 bits: 64 * 15 < 1024).
// Every lane of the wave must be here (the DPP adds read their neighbours).
__device__ inline void band_fold(unsigned long long (*cells)[kBandFrames], const int t, const int lane, const bool have, const unsigned long long bits)
{
    int cell;
    uint32_t p[3];
    const int kind = spx::decompose(bits, cell, p);
    const unsigned long long nans = __ballot(have && kind == spx::kNan), infs = __ballot(have && kind == spx::kInf);
    if (nans | infs) {   // (wave-uniform)
        if (lane == 0) {
            if (nans) atomicAdd(&cells[spx::kNanSlot][t], (unsigned long long)__popcll(nans));
            if (infs) atomicAdd(&cells[spx::kInfSlot][t], (unsigned long long)__popcll(infs));
        }
    }
    bool mine = have && kind == spx::kFinite && (p[0] | p[1] | p[2]) != 0;
    unsigned long long live = __ballot(mine);
    while (live) {   // (wave-uniform)
        const int c = __builtin_amdgcn_readlane(cell, __ffsll((long long)live) - 1);
        const bool take = mine && cell == c;
        const uint32_t q0 = take ? p[0] : 0u, q1 = take ? p[1] : 0u, q2 = take ? p[2] : 0u;
        const uint32_t high = band_row_sum((q0 >> 28) | ((q1 >> 28) << 10) | ((q2 >> 28) << 20));
        const uint32_t hs = (uint32_t)band_rows_total(high);   // (three fields below 1024 each: no carry between them)
        const unsigned long long s0 = band_rows_total(band_row_sum(q0 & 0x0fffffffu)) + ((unsigned long long)(hs & 0x3ffu) << 28);
        const unsigned long long s1 = band_rows_total(band_row_sum(q1 & 0x0fffffffu)) + ((unsigned long long)((hs >> 10) & 0x3ffu) << 28);
        const unsigned long long s2 = band_rows_total(band_row_sum(q2 & 0x0fffffffu)) + ((unsigned long long)((hs >> 20) & 0x3ffu) << 28);
        // c + 2 <= 65: in bounds for every exponent field.  (An LDS add without a return value: nothing waits for it.)
        if (lane < 3) atomicAdd(&cells[c + lane][t], lane == 0 ? s0 : lane == 1 ? s1 : s2);
        mine = mine && !take;
        live &= ~__ballot(take);
    }
}

// band[b * stride + x_base + x] for the frames x in [0, frames) of the frame-major plane at `plane` (frame x, row y at
// plane[x * n + y]) and every band b of the list.  grid = (pieces of kBandFrames frames, bands), 256 threads.  Workgroup (p, b): its
// cells are u64[spx::kSlots][kBandFrames] in LDS, slot-major with one column per frame - the mean kernel's shape.  Wave w reads the
// band's rows of the frames w, w + 4, ... 64 rows at a time, 512 contiguous bytes per load, kBandUnroll loads in flight, and folds them
// into the frame's column.  Behind a barrier thread t < kBandFrames finishes column t and stores the frame's sum: neighbouring doubles.
__global__ __launch_bounds__(kBandThreads) void k_band_sum(const double *__restrict__ plane, const int n, const long long frames,
                                                           const BandList bands, double *__restrict__ band, const long long stride,
                                                           const long long x_base)
{
    __shared__ unsigned long long cells[spx::kSlots][kBandFrames];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int k = tid; k < spx::kSlots * kBandFrames; k += kBandThreads) (&cells[0][0])[k] = 0;
    __syncthreads();

    const int y0 = bands.y[2 * blockIdx.y], y1 = bands.y[2 * blockIdx.y + 1];
    const long long first = (long long)blockIdx.x * kBandFrames;
    for (int t = wave; t < kBandFrames && first + t < frames; t += kBandWaves) {
        // (64-bit: 8 * width * n passes 4 GiB)
        const unsigned long long *const col = (const unsigned long long *)plane + (size_t)(first + t) * (size_t)n;
        for (int y = y0; y < y1; y += 64 * kBandUnroll) {
            unsigned long long v[kBandUnroll];
            bool have[kBandUnroll];
#pragma unroll
            for (int u = 0; u < kBandUnroll; u++) {
                const int yu = y + 64 * u + lane;
                have[u] = yu < y1;
                v[u] = have[u] ? col[yu] : 0ull;
            }
#pragma unroll
            for (int u = 0; u < kBandUnroll; u++) {
                if (y + 64 * u >= y1) break;   // (wave-uniform)
                band_fold(cells, t, lane, have[u], v[u]);
            }
        }
    }
    __syncthreads();
    if (tid < kBandFrames && first + tid < frames) {
        spx::Finisher f;
        for (int k = 0; k < spx::kCells; k++) f.push(cells[k][tid]);
        const unsigned long long bits = spx::apply_specials(f.result(), cells[spx::kNanSlot][tid], cells[spx::kInfSlot][tid]);
        band[(size_t)blockIdx.y * (size_t)stride + (size_t)(x_base + first + tid)] = __longlong_as_double((long long)bits);
    }
}

}  // namespace spk
