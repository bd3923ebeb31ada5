// sp_kernel_small.h — the small kernels around the frame loops: the timing pair's empty kernel, the merge of slice replies, the
// placement of gathered strips and the clearing of a batch's replies.
#pragma once

#include "sp_kernel_frames_batch.h"

// what sp_context_event_pair_overhead_ms puts between the context's two events
__global__ void k_noop() {}

// `rank_stride`: 64-bit words between two ranks' records of the same render; blockIdx.y: the render of a batch (its records start
// blockIdx.y * record_len words into every rank's block, its merged record blockIdx.y * record_len words into the outputs)
__global__ void k_merge_replies(const unsigned long long *rec, int count, int lut_len, size_t rank_stride, unsigned long long *c_hist,
                                unsigned long long *cb_hist, double *minmax)
{
    const int stride = lut_len + SP_CB_HIST_SIZE + 2;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const size_t shift = (size_t)blockIdx.y * (size_t)stride;
    rec += shift;
    if (i < lut_len + SP_CB_HIST_SIZE) {
        unsigned long long s = 0;
        for (int r = 0; r < count; r++) s += rec[(size_t)r * rank_stride + i];                      // spectroplot.js:1232-1238
        if (i < lut_len) {
            if (c_hist) c_hist[shift + i] = s;
        } else if (cb_hist) {
            cb_hist[shift + i - lut_len] = s;
        }
    } else if (i < stride && minmax) {
        const int k = i - (lut_len + SP_CB_HIST_SIZE);                                              // 0: min, 1: max
        double v = __longlong_as_double((long long)rec[i]);
        for (int r = 1; r < count; r++) {
            const double w = __longlong_as_double((long long)rec[(size_t)r * rank_stride + i]);
            v = k == 0 ? (w < v ? w : v) : (w > v ? w : v);                                         // the `<` / `>` updates of :1230-1231
        }
        minmax[shift + k] = v;
    }
}

// putImageData(strip, offset, 0) for every gathered strip at once (lib/spectroplot.js:1241-1244): strip r of `count`, laid end to end in
// `strips` as an all-gather / gather delivers them, goes to columns [r * slice_width, (r + 1) * slice_width) of the n x width image
// (spectrogram), or to rows [width - slice_width - r * slice_width, ...) of the width x n image (waterfall: row bands in reverse order).
// One thread moves one V (16 bytes = 4 pixels where the widths allow, else one pixel); reads and writes are whole row pieces.
// (spgeo::SliceLayout in sp_geometry.h is the host-side twin of this arithmetic.)
template <typename V>
__global__ void k_place_strips(uint8_t *__restrict__ image, const uint8_t *__restrict__ strips, int count, int n, int width, int slice_width,
                               int waterfall)
{
    constexpr int PX = (int)sizeof(V) / 4;
    const size_t units_per_strip = (size_t)slice_width * (size_t)n / PX;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= units_per_strip * (size_t)count) return;
    const int r = (int)(i / units_per_strip);
    const size_t u = i % units_per_strip;
    size_t dst;
    if (waterfall) {
        dst = ((size_t)(width - slice_width - r * slice_width) * (size_t)n) / PX + u;        // one contiguous band of rows
    } else {
        const size_t row_units = (size_t)slice_width / PX;
        const size_t y = u / row_units, x = u % row_units;
        dst = (y * (size_t)width + (size_t)r * (size_t)slice_width) / PX + x;
    }
    ((V *)image)[dst] = ((const V *)strips)[i];
}

// Clears the replies of a batch's items before its launches: histograms 0, dBfs range (0, -200) (worker.js:35-41).  One workgroup per item.
__global__ void k_batch_clear(const spk2::BatchItem *items, int lut_len)
{
    const spk2::BatchItem &it = items[blockIdx.x];
    for (int i = threadIdx.x; i < lut_len + SP_CB_HIST_SIZE + 2; i += blockDim.x) {
        if (i < lut_len) {
            if (it.out_c) it.out_c[i] = 0;
        } else if (i < lut_len + SP_CB_HIST_SIZE) {
            if (it.out_cb) it.out_cb[i - lut_len] = 0;
        } else if (it.out_minmax) {
            it.out_minmax[i - lut_len - SP_CB_HIST_SIZE] = i == lut_len + SP_CB_HIST_SIZE ? 0.0 : -200.0;
        }
    }
}
