// sp_kernel_density.h — k_density_count: the persistence spectrum's count of an index image's bytes per image row.
// Its decomposition (DensityShape, density_shape, density_rect) is host + device arithmetic in sp_kernel_args.h.
#pragma once

#include "sp_kernel_args.h"

constexpr int kDensityAhead = 4;   // loads a lane has in flight before it counts the first

// The frames [x_begin, x_end) of an index image (n rows, `width` frames, either layout) counted per image row.  Slot s of the workgroup
// keeps row y0 + s; the cell of index g is s * 256 + ((g + s) & 255): a histogram is 256 wide whatever lut_len is, so no byte can
// index past it, and rotated by its slot, so that one index in neighbouring rows (a waterfall wave's lanes) lies in different banks.
// Equal neighbours are merged before the LDS add - a lane's 16 frames of one row (spectrogram), a lane's successive frames of its four
// bins (waterfall) - so a flat row costs one add per 16 pixels instead of 16 to one address.
template <bool WATERFALL>
__global__ void __launch_bounds__(kDensityThreads)
k_density_count(const uint8_t *__restrict__ index, int n, int width, int x_begin, int x_end, int lut_len, uint32_t *__restrict__ density)
{
    constexpr int ROWS = WATERFALL ? kDensityRowsWaterfall : kDensityRowsSpectrogram;
    __shared__ uint32_t s_h[ROWS * 256];
    const int t = threadIdx.x;
    for (int i = t; i < ROWS * 256; i += kDensityThreads) s_h[i] = 0;
    __syncthreads();
    const DensityShape d = density_shape(n, WATERFALL, x_begin, x_end);
    int y0, y1, x0, x1;
    density_rect(d, n, x_begin, x_end, (long long)blockIdx.x, y0, y1, x0, x1);
    const auto add = [&](int slot, uint32_t g, uint32_t count) { atomicAdd(&s_h[slot * 256 + (int)((g + (uint32_t)slot) & 255u)], count); };

    if (!WATERFALL) {
        // image: n rows x width columns; 32 lanes per row, a lane takes 16 consecutive frames of its row per pass (512 frames a pass):
        // one 16-byte load where the piece is whole and lies aligned, four dwords where it lies 4-byte aligned, else byte by byte.
        // The loads of kDensityAhead passes are issued before the first of them is counted (a pass is a load and the LDS adds that
        // wait for it; one after the other, a workgroup's time is its passes' memory latencies added up).
        const int slot = t >> 5, y = y0 + slot;
        if (y < y1) {
            const uint8_t *const row = index + (size_t)y * (size_t)width;
            const auto fetch = [&](long long xa, uint32_t (&w)[4]) -> int {   // -> the piece's pixels (0: it lies behind the range)
                w[0] = w[1] = w[2] = w[3] = 0;
                if (xa >= x1) return 0;
                const uint8_t *const p = row + xa;
                const int cnt = x1 - xa < 16 ? (int)(x1 - xa) : 16;
                if (cnt == 16 && ((uintptr_t)p & 15) == 0) {
                    const uint4 v = *(const uint4 *)p;
                    w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
                } else if (cnt == 16 && ((uintptr_t)p & 3) == 0) {
#pragma unroll
                    for (int k = 0; k < 4; k++) w[k] = ((const uint32_t *)p)[k];
                } else {
#pragma unroll
                    for (int k = 0; k < 16; k++)
                        if (k < cnt) w[k >> 2] |= (uint32_t)p[k] << (8 * (k & 3));
                }
                return cnt;
            };
            const auto count = [&](const uint32_t (&w)[4], int cnt) {
                if (cnt < 1) return;
                uint32_t cur = w[0] & 255u, run = 1;
#pragma unroll
                for (int k = 1; k < 16; k++) {
                    const uint32_t b = (w[k >> 2] >> (8 * (k & 3))) & 255u;
                    if (k < cnt) {
                        if (b == cur) {
                            run++;
                        } else {
                            add(slot, cur, run);
                            cur = b;
                            run = 1;
                        }
                    }
                }
                add(slot, cur, run);
            };
            for (long long xa = (long long)x0 + 16 * (t & 31); xa < x1; xa += 512 * kDensityAhead) {
                uint32_t w[kDensityAhead][4];
                int cnt[kDensityAhead];
#pragma unroll
                for (int u = 0; u < kDensityAhead; u++) cnt[u] = fetch(xa + 512 * u, w[u]);
#pragma unroll
                for (int u = 0; u < kDensityAhead; u++) count(w[u], cnt[u]);
            }
        }
    } else {
        // image: width rows x n columns, frame x in row width - 1 - x, image row y in column n - 1 - y: the band's rows are the
        // columns [n - y1, n - y0).  16 lanes per frame, a lane takes four consecutive columns (one dword where they exist and lie
        // aligned, else bytes) of every 16th frame, kDensityAhead loads ahead as above; byte j of its word belongs to slot top - j.
        const int cols = y1 - y0, q = t & 15, valid = cols - 4 * q < 4 ? cols - 4 * q : 4, top = cols - 1 - 4 * q;
        if (valid > 0) {
            const auto flush = [&](uint32_t word, uint32_t count) {
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (j < valid) add(top - j, (word >> (8 * j)) & 255u, count);
            };
            const auto fetch = [&](long long x) -> uint32_t {   // (x < x1)
                const uint8_t *const p = index + (size_t)((long long)width - 1 - x) * (size_t)n + (size_t)(n - y1 + 4 * q);
                if (valid == 4 && ((uintptr_t)p & 3) == 0) return *(const uint32_t *)p;
                uint32_t word = 0;
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (j < valid) word |= (uint32_t)p[j] << (8 * j);
                return word;
            };
            uint32_t held = 0, run = 0;
            for (long long xa = (long long)x0 + (t >> 4); xa < x1; xa += 16 * kDensityAhead) {
                uint32_t word[kDensityAhead];
#pragma unroll
                for (int u = 0; u < kDensityAhead; u++) word[u] = xa + 16 * u < x1 ? fetch(xa + 16 * u) : 0u;
#pragma unroll
                for (int u = 0; u < kDensityAhead; u++) {
                    if (xa + 16 * u >= x1) continue;
                    if (run && word[u] == held) {
                        run++;
                    } else {
                        if (run) flush(held, run);
                        held = word[u];
                        run = 1;
                    }
                }
            }
            if (run) flush(held, run);
        }
    }
    __syncthreads();
    // the workgroup's share: its non-zero cells of indices the map has, one no-return atomic each (consecutive lanes, consecutive cells)
    for (int i = t; i < ROWS * 256; i += kDensityThreads) {
        const int slot = i >> 8, y = y0 + slot, g = (i - slot) & 255;
        const uint32_t v = s_h[i];
        if (v && y < y1 && g < lut_len) atomicAdd(&density[(size_t)y * (size_t)lut_len + (size_t)g], v);
    }
}
