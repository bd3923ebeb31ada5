// sp_kernel_moment.h — the exact spectral moments of a band per frame (include/spectroplot_hip.h, sp_plan_execute_moments):
// m[k][b][x] = RN(exact sum over the image rows y in [y0_b, y1_b) of (y - y0_b)^k * power[x][y]), k = 0 .. ORDER.  k_band_sum's shape
// (sp_kernel_band.h) with sp_moment_core.h's weighted pieces: integer adds only, so the bits do not depend on the order of the rows, on
// the grid or on how the plane is cut into blocks of frames.
//
// One launch, no global workspace: a frame's sums are made inside one workgroup, finished there and stored.
#pragma once

#include <hip/hip_runtime.h>

#include "sp_band_list.h"
#include "sp_moment_core.h"

namespace spk {

constexpr int kMomentFrames = 8;     // frames of a workgroup, as k_band_sum's: one LDS column each
constexpr int kMomentWaves = 4;      // wave w takes the frames w, w + 4, ... of its piece
constexpr int kMomentThreads = 64 * kMomentWaves;
constexpr int kMomentUnroll = 4;     // loads of 64 rows a wave has in flight

// the pieces of a value over its moments: 3 for m0 (the fourth is 0 at weight 1), 4 for m1, 4 for m2
constexpr int moment_pieces(int order) { return order == 0 ? 3 : order == 1 ? 7 : 11; }
// the LDS slots of a frame: one accumulator per moment, then the shared NaN and +inf counters
constexpr int moment_slots(int order) { return (order + 1) * spm::kCells + 2; }
// piece i's moment and its place j among the moment's pieces
constexpr int moment_of_piece(int i) { return i < 3 ? 0 : i < 7 ? 1 : 2; }
constexpr int place_of_piece(int i) { return i < 3 ? i : i < 7 ? i - 3 : i - 7; }

// Lane 15 of every row of 16 lanes gets the row's sum (the other lanes a prefix of it); the caller keeps the addends below 2^28.
__device__ inline uint32_t moment_row_sum(uint32_t x)
{
#define SP_DPP_ADD(ctrl) x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, ctrl, 0xf, 0xf, false);
    SP_DPP_ADD(0x111)   // row_shr:1
    SP_DPP_ADD(0x112)   // row_shr:2
    SP_DPP_ADD(0x114)   // row_shr:4
    SP_DPP_ADD(0x118)   // row_shr:8
#undef SP_DPP_ADD
    return x;
}
// the sum of moment_row_sum's four row sums
__device__ inline unsigned long long moment_rows_total(uint32_t x)
{
    return (unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)x, 15) + (uint32_t)__builtin_amdgcn_readlane((int)x, 31) +
           (uint32_t)__builtin_amdgcn_readlane((int)x, 47) + (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
}

// Adds the wave's 64 values (lane l holds `bits` of the row at distance r from the band's first where `have`) into column t of the
// cells, weighted for every moment.  band_fold's loop carries over because the weight does not move a value's cell: the wave takes the
// cell number of the first lane that still has a value, sums the 3 + 4 + 4 pieces of every lane with that cell number across the wave
// in the VALU, and lanes 0 .. 10 add the totals; those lanes retire and the loop goes on while a lane is left.
// The 28-bit / 4-bit split of a piece is kept (not 64-bit row sums, which would double every DPP add): the low 28 bits of a piece are
// summed apart - a row of 16 lanes stays below 2^32, the four rows' total below 2^34 - and the high 4 bits travel three pieces to a
// word, fields of 10 bits (64 * 15 = 960 < 1024: no carry between fields).  A total is below 2^34 + 960 * 2^28 < 2^38.
// Every lane of the wave must be here (the DPP adds read their neighbours).
template <int ORDER>
__device__ inline void moment_fold(unsigned long long (*cells)[kMomentFrames], const int t, const int lane, const bool have,
                                   const unsigned long long bits, const uint32_t r)
{
    constexpr int NP = moment_pieces(ORDER), NH = (NP + 2) / 3;
    int cell;
    uint32_t p[NP];
    int kind;
    {
        uint32_t q[4];
        kind = spm::decompose_weighted(bits, 1ull, cell, q);
        p[0] = q[0], p[1] = q[1], p[2] = q[2];   // (q[3] == 0 at weight 1)
        if constexpr (ORDER >= 1) {
            spm::decompose_weighted(bits, spm::weight(r, 1), cell, q);
#pragma unroll
            for (int j = 0; j < 4; j++) p[3 + j] = q[j];
        }
        if constexpr (ORDER >= 2) {
            spm::decompose_weighted(bits, spm::weight(r, 2), cell, q);
#pragma unroll
            for (int j = 0; j < 4; j++) p[7 + j] = q[j];
        }
    }
    const unsigned long long nans = __ballot(have && kind == spx::kNan), infs = __ballot(have && kind == spx::kInf);
    if (nans | infs) {   // (wave-uniform)
        if (lane == 0) {
            if (nans) atomicAdd(&cells[(ORDER + 1) * spm::kCells][t], (unsigned long long)__popcll(nans));
            if (infs) atomicAdd(&cells[(ORDER + 1) * spm::kCells + 1][t], (unsigned long long)__popcll(infs));
        }
    }
    // (the unweighted pieces decide: a value of weight 0 retires with its cell's round, and adds zeros)
    bool mine = have && kind == spx::kFinite && (p[0] | p[1] | p[2]) != 0;
    unsigned long long live = __ballot(mine);
    while (live) {   // (wave-uniform)
        const int c = __builtin_amdgcn_readlane(cell, __ffsll((long long)live) - 1);
        const bool take = mine && cell == c;
        uint32_t q[NP], hs[NH];
#pragma unroll
        for (int i = 0; i < NP; i++) q[i] = take ? p[i] : 0u;
#pragma unroll
        for (int h = 0; h < NH; h++) {
            uint32_t x = 0;
#pragma unroll
            for (int f = 0; f < 3; f++)
                if (3 * h + f < NP) x |= (q[3 * h + f] >> 28) << (10 * f);
            hs[h] = (uint32_t)moment_rows_total(moment_row_sum(x));
        }
        unsigned long long mine_sum = 0;
        int slot = 0;
#pragma unroll
        for (int i = 0; i < NP; i++) {
            const unsigned long long s = moment_rows_total(moment_row_sum(q[i] & 0x0fffffffu)) +
                                         ((unsigned long long)((hs[i / 3] >> (10 * (i % 3))) & 0x3ffu) << 28);
            if (lane == i) mine_sum = s, slot = moment_of_piece(i) * spm::kCells + c + place_of_piece(i);
        }
        // c + 3 <= 66 < spm::kCells: in bounds for every exponent field.  (An LDS add without a return value: nothing waits for it.)
        if (lane < NP) atomicAdd(&cells[slot][t], mine_sum);
        mine = mine && !take;
        live &= ~__ballot(take);
    }
}

// m[(k * gridDim.y + b) * stride + x_base + x] for the frames x in [0, frames) of the frame-major plane at `plane` (frame x, row y at
// plane[x * n + y]), every band b of the list and k = 0 .. ORDER.  grid = (pieces of kMomentFrames frames, bands), 256 threads.
// Workgroup (p, b): its cells are u64[moment_slots(ORDER)][kMomentFrames] in LDS, slot-major with one column per frame - at ORDER 2
// (3 * 68 + 2) * 8 * 8 = 13 184 bytes.  Wave w reads the band's rows of the frames w, w + 4, ... 64 rows at a time and folds them
// into the frame's column.  Behind a barrier thread t < (ORDER + 1) * kMomentFrames finishes moment t / 8 of column t % 8 and stores
// it: neighbouring doubles per moment.
template <int ORDER>
__global__ __launch_bounds__(kMomentThreads) void k_moment_sum(const double *__restrict__ plane, const int n, const long long frames,
                                                               const BandList bands, double *__restrict__ out, const long long stride,
                                                               const long long x_base)
{
    constexpr int kSlots = moment_slots(ORDER);
    __shared__ unsigned long long cells[kSlots][kMomentFrames];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int k = tid; k < kSlots * kMomentFrames; k += kMomentThreads) (&cells[0][0])[k] = 0;
    __syncthreads();

    const int y0 = bands.y[2 * blockIdx.y], y1 = bands.y[2 * blockIdx.y + 1];
    const long long first = (long long)blockIdx.x * kMomentFrames;
    for (int t = wave; t < kMomentFrames && first + t < frames; t += kMomentWaves) {
        // (64-bit: 8 * width * n passes 4 GiB)
        const unsigned long long *const col = (const unsigned long long *)plane + (size_t)(first + t) * (size_t)n;
        for (int y = y0; y < y1; y += 64 * kMomentUnroll) {
            unsigned long long v[kMomentUnroll];
            bool have[kMomentUnroll];
#pragma unroll
            for (int u = 0; u < kMomentUnroll; u++) {
                const int yu = y + 64 * u + lane;
                have[u] = yu < y1;
                v[u] = have[u] ? col[yu] : 0ull;
            }
#pragma unroll
            for (int u = 0; u < kMomentUnroll; u++) {
                if (y + 64 * u >= y1) break;   // (wave-uniform)
                // (a lane past y1 has no value: its distance is not looked at, and is kept below 2^20 all the same)
                moment_fold<ORDER>(cells, t, lane, have[u], v[u], have[u] ? (uint32_t)(y + 64 * u + lane - y0) : 0u);
            }
        }
    }
    __syncthreads();
    const int f = tid % kMomentFrames, k = tid / kMomentFrames;
    if (k <= ORDER && first + f < frames) {
        spx::Finisher fin;
        for (int c = 0; c < spm::kCells; c++) fin.push(cells[k * spm::kCells + c][f]);
        const unsigned long long bits =
            spx::apply_specials(fin.result(), cells[(ORDER + 1) * spm::kCells][f], cells[(ORDER + 1) * spm::kCells + 1][f]);
        out[((size_t)k * gridDim.y + blockIdx.y) * (size_t)stride + (size_t)(x_base + first + f)] = __longlong_as_double((long long)bits);
    }
}

}  // namespace spk
