// sp_kernel_index.h — the small kernels of indexed images: RGBA -> index (the render_extract path) and index -> RGBA through a LUT.
#pragma once

#include "sp_kernel_args.h"

// Byte 0 of every pixel of a band of an RGBA image: `rows` rows of row_px pixels, pitch_px pixels apart in both images.  A thread takes
// the four pixels [4q, 4q + 4) of a row: one 16-byte load and one dword store where both lie aligned and the row has them, else pixel
// by pixel (a row's ragged end, rows that start off 16 bytes).
__global__ void k_extract_index(const uint8_t *__restrict__ rgba, uint8_t *__restrict__ index, size_t row_px, size_t rows, size_t pitch_px)
{
    const size_t quads = (row_px + 3) / 4;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= quads * rows) return;
    const size_t r = i / quads, q = i % quads;
    const uint8_t *const src = rgba + 4 * (r * pitch_px + 4 * q);
    uint8_t *const dst = index + r * pitch_px + 4 * q;
    if (4 * q + 4 <= row_px && ((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 3) == 0) {
        const uint4 v = *(const uint4 *)src;
        *(uint32_t *)dst = (v.x & 255u) | ((v.y & 255u) << 8) | ((v.z & 255u) << 16) | (v.w << 24);
        return;
    }
    for (size_t k = 0; k < 4 && 4 * q + k < row_px; k++) dst[k] = src[4 * k];
}

// index -> RGBA through a LUT.  The index image is read in 16-byte units from its first aligned byte on, one unit per thread: a 16-byte
// load and four 16-byte stores where the unit's pixels lie aligned in the RGBA image, dword or byte stores where they do not; the
// pixels in front of the first unit and behind the last one (at most 15 each) are taken byte-wise by workgroup 0's first threads.
__global__ void k_index_to_rgba(const uint8_t *__restrict__ index, size_t pixels, const IndexLut lut, uint8_t *__restrict__ rgba)
{
    __shared__ uint32_t s_lut[256];
    s_lut[threadIdx.x] = lut.v[threadIdx.x];
    __syncthreads();
    const auto put = [&](size_t i, uint32_t c) {
        uint8_t *const d = rgba + 4 * i;
        if (((uintptr_t)d & 3) == 0) {
            *(uint32_t *)d = c;
        } else {
            for (int k = 0; k < 4; k++) d[k] = (uint8_t)(c >> (8 * k));
        }
    };
    size_t head = (size_t)(-(intptr_t)(uintptr_t)index) & 15;
    if (head > pixels) head = pixels;
    const size_t units = (pixels - head) / 16, tail0 = head + 16 * units;
    if (blockIdx.x == 0) {
        const size_t t = threadIdx.x;
        if (t < head) put(t, s_lut[index[t]]);
        else if (t - head < pixels - tail0) put(tail0 + (t - head), s_lut[index[tail0 + (t - head)]]);
    }
    const size_t u = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= units) return;
    const size_t i0 = head + 16 * u;
    const uint4 v = *(const uint4 *)(index + i0);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    const bool wide = ((uintptr_t)(rgba + 4 * i0) & 15) == 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t c0 = s_lut[w[k] & 255u], c1 = s_lut[(w[k] >> 8) & 255u], c2 = s_lut[(w[k] >> 16) & 255u], c3 = s_lut[w[k] >> 24];
        if (wide) {
            *(uint4 *)(rgba + 4 * (i0 + 4 * k)) = make_uint4(c0, c1, c2, c3);
        } else {
            put(i0 + 4 * k, c0);
            put(i0 + 4 * k + 1, c1);
            put(i0 + 4 * k + 2, c2);
            put(i0 + 4 * k + 3, c3);
        }
    }
}
