// sp_kernel_band.h — the exact band-power series and the exact spectral moments of a band (include/spectroplot_hip.h,
// sp_plan_execute_bandpower and sp_plan_execute_moments), one kernel body over the moments' ORDER:
//   m[k][b][x] = RN(exact sum over the image rows y in [y0_b, y1_b) of (y - y0_b)^k * power[x][y]), k = 0 .. ORDER,
// and m[0] alone, ORDER 0, is the band-power series.  The sum is sp_exact_sum.h's, as for the mean (sp_kernel_mean.h), turned by 90
// degrees: the mean adds along x into one accumulator per row, this adds along y into ORDER + 1 accumulators per frame; a higher moment
// has sp_moment_core.h's weighted pieces.  Integer adds only, so the result does not depend on the order of the rows, on the grid or on
// how the plane is cut into blocks of frames.
//
// One launch, no global workspace: a frame's sums are made inside one workgroup, finished there and stored.
#pragma once

#include <hip/hip_runtime.h>

#include "sp_band_list.h"
#include "sp_moment_core.h"
#include "sp_wave_sum.h"

namespace spk {

constexpr int kBandFrames = 8;      // frames of a workgroup: one LDS column each.  (Few, so that a screen-wide request still fills the
                                    // chip: a band has width / 8 workgroups and no more.)
constexpr int kBandWaves = 4;       // waves of a workgroup: wave w takes the frames w, w + 4, ... of its piece
constexpr int kBandThreads = 64 * kBandWaves;
constexpr int kBandUnroll = 4;      // loads of 64 rows a wave has in flight

// The cells of one accumulator: ORDER 0 has sp_exact_sum.h's three pieces a value and its 66 cells, a weighted value has four pieces
// and sp_moment_core.h's 68.  The LDS slots of a frame: one accumulator per moment, then the shared NaN and +inf counters.
constexpr int band_cells(int order) { return order == 0 ? spx::kCells : spm::kCells; }
constexpr int band_slots(int order) { return (order + 1) * band_cells(order) + 2; }
// the pieces of a value over its moments: 3 for m0 (the fourth is 0 at weight 1), 4 for m1, 4 for m2
constexpr int band_pieces(int order) { return order == 0 ? 3 : order == 1 ? 7 : 11; }
// piece i's slot from its value's cell on: its moment's accumulator and its place j among the moment's pieces
constexpr int band_piece_slot(int order, int i) { return i < 3 ? i : i < 7 ? band_cells(order) + i - 3 : 2 * band_cells(order) + i - 7; }

// Adds the wave's 64 values (lane l holds `bits` of the row at distance r from the band's first where `have`) into column t of the
// cells, weighted for every moment; a NaN or a +inf is counted.  The column is the wave's own, but all 64 values of a frame land in
// the few cells around the frame's level, and 64 LDS atomics on one address serialise.  So the wave folds first: it takes the cell
// number of the first lane that still has a value, sums the NP pieces of every lane with that cell number across the wave in the VALU,
// and lanes 0 .. NP - 1 add the totals, piece i to the slot c + band_piece_slot(ORDER, i); those lanes retire and the loop goes on
// while a lane is left.  (A weight does not move a value's cell, so the pieces of every moment go in one round.)  A spectrum's values
// spend a few rounds; 64 values of 64 different cells spend 64.
// A piece is below 2^32 and a row of 16 lanes would pass 32 bits - and 64-bit row sums would double every DPP add: the low 28 bits of
// a piece are summed apart - a row stays below 2^32, the four rows' total below 2^34 - and the high 4 bits travel three pieces to a
// word, fields of 10 bits (64 * 15 = 960 < 1024: no carry between fields).  A total is below 2^34 + 960 * 2^28 < 2^38.
// Every lane of the wave must be here (sp_wave_sum.h).
template <int ORDER>
__device__ inline void band_fold(unsigned long long (*cells)[kBandFrames], const int t, const int lane, const bool have,
                                 const unsigned long long bits, const uint32_t r)
{
    constexpr int NP = band_pieces(ORDER), NH = (NP + 2) / 3, kNan = (ORDER + 1) * band_cells(ORDER), kInf = kNan + 1;
    int cell;
    uint32_t p[NP];
    int kind;
    if constexpr (ORDER == 0) {
        kind = spx::decompose(bits, cell, p);
    } else {
        uint32_t q[4];
        kind = spm::decompose_weighted(bits, 1ull, cell, q);
        p[0] = q[0], p[1] = q[1], p[2] = q[2];   // (q[3] == 0 at weight 1)
        spm::decompose_weighted(bits, spm::weight(r, 1), cell, q);
#pragma unroll
        for (int j = 0; j < 4; j++) p[3 + j] = q[j];
        if constexpr (ORDER >= 2) {
            spm::decompose_weighted(bits, spm::weight(r, 2), cell, q);
#pragma unroll
            for (int j = 0; j < 4; j++) p[7 + j] = q[j];
        }
    }
    const unsigned long long nans = __ballot(have && kind == spx::kNan), infs = __ballot(have && kind == spx::kInf);
    if (nans | infs) {   // (wave-uniform)
        if (lane == 0) {
            if (nans) atomicAdd(&cells[kNan][t], (unsigned long long)__popcll(nans));
            if (infs) atomicAdd(&cells[kInf][t], (unsigned long long)__popcll(infs));
        }
    }
    // (the unweighted pieces decide: a value of weight 0 retires with its cell's round, and adds zeros)
    bool mine = have && kind == spx::kFinite && (p[0] | p[1] | p[2]) != 0;
    unsigned long long live = __ballot(mine);
    while (live) {   // (wave-uniform)
        const int c = __builtin_amdgcn_readlane(cell, __ffsll((long long)live) - 1);
        const bool take = mine && cell == c;
        // Lane i < NP adds piece i's total to the slot c + band_piece_slot(ORDER, i): c <= 63 and a piece's place <= 3, in bounds of its
        // accumulator for every exponent field.  (An LDS add without a return value: nothing waits for it.)
        if constexpr (ORDER == 0) {
            // NP == 3 and one accumulator, written out: the loops below give the same sums at NP == 3 but other instructions, and
            // tests/test_isa_checks.py holds this instance to the band kernel's stream as it was measured
            const uint32_t q0 = take ? p[0] : 0u, q1 = take ? p[1] : 0u, q2 = take ? p[2] : 0u;
            const uint32_t high = wave_row_sums((q0 >> 28) | ((q1 >> 28) << 10) | ((q2 >> 28) << 20));
            const uint32_t hs = (uint32_t)wave_rows_total(high);
            const unsigned long long s0 = wave_rows_total(wave_row_sums(q0 & 0x0fffffffu)) + ((unsigned long long)(hs & 0x3ffu) << 28);
            const unsigned long long s1 = wave_rows_total(wave_row_sums(q1 & 0x0fffffffu)) + ((unsigned long long)((hs >> 10) & 0x3ffu) << 28);
            const unsigned long long s2 = wave_rows_total(wave_row_sums(q2 & 0x0fffffffu)) + ((unsigned long long)((hs >> 20) & 0x3ffu) << 28);
            if (lane < 3) atomicAdd(&cells[c + lane][t], lane == 0 ? s0 : lane == 1 ? s1 : s2);
        } else {
            uint32_t q[NP], hs[NH];
#pragma unroll
            for (int i = 0; i < NP; i++) q[i] = take ? p[i] : 0u;
#pragma unroll
            for (int h = 0; h < NH; h++) {
                uint32_t x = 0;
#pragma unroll
                for (int f = 0; f < 3; f++)
                    if (3 * h + f < NP) x |= (q[3 * h + f] >> 28) << (10 * f);
                hs[h] = (uint32_t)wave_rows_total(wave_row_sums(x));
            }
            unsigned long long sum = 0;
            int slot = 0;
#pragma unroll
            for (int i = 0; i < NP; i++) {
                const unsigned long long s = wave_rows_total(wave_row_sums(q[i] & 0x0fffffffu)) +
                                             ((unsigned long long)((hs[i / 3] >> (10 * (i % 3))) & 0x3ffu) << 28);
                if (lane == i) sum = s, slot = c + band_piece_slot(ORDER, i);
            }
            if (lane < NP) atomicAdd(&cells[slot][t], sum);
        }
        mine = mine && !take;
        live &= ~__ballot(take);
    }
}

// m[(k * gridDim.y + b) * stride + x_base + x] for the frames x in [0, frames) of the frame-major plane at `plane` (frame x, row y at
// plane[x * n + y]), every band b of the list and k = 0 .. ORDER.  grid = (pieces of kBandFrames frames, bands), 256 threads.
// Workgroup (p, b): its cells are u64[band_slots(ORDER)][kBandFrames] in LDS, slot-major with one column per frame - the mean kernel's
// shape; 4352, 8832 and 13 184 bytes at ORDER 0, 1 and 2.  Wave w reads the band's rows of the frames w, w + 4, ... 64 rows at a time,
// 512 contiguous bytes per load, kBandUnroll loads in flight, and folds them into the frame's column.  Behind a barrier thread
// t < (ORDER + 1) * kBandFrames finishes moment t / 8 of column t % 8 and stores it: neighbouring doubles per moment.
template <int ORDER>
__global__ __launch_bounds__(kBandThreads) void k_band_sum(const double *__restrict__ plane, const int n, const long long frames,
                                                           const BandList bands, double *__restrict__ out, const long long stride,
                                                           const long long x_base)
{
    constexpr int kCells = band_cells(ORDER), kSlots = band_slots(ORDER);
    __shared__ unsigned long long cells[kSlots][kBandFrames];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int k = tid; k < kSlots * kBandFrames; k += kBandThreads) (&cells[0][0])[k] = 0;
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
                // (a lane past y1 has no value: its distance is not looked at, and is kept below 2^20 all the same)
                band_fold<ORDER>(cells, t, lane, have[u], v[u], have[u] ? (uint32_t)(y + 64 * u + lane - y0) : 0u);
            }
        }
    }
    __syncthreads();
    const int f = tid % kBandFrames, k = tid / kBandFrames;
    if (k <= ORDER && first + f < frames) {
        spx::Finisher fin;
        for (int c = 0; c < kCells; c++) fin.push(cells[k * kCells + c][f]);
        const unsigned long long bits =
            spx::apply_specials(fin.result(), cells[(ORDER + 1) * kCells][f], cells[(ORDER + 1) * kCells + 1][f]);
        out[((size_t)k * gridDim.y + blockIdx.y) * (size_t)stride + (size_t)(x_base + first + f)] = __longlong_as_double((long long)bits);
    }
}

}  // namespace spk
