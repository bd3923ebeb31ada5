// sp_kernel_args.h — what the host fills or evaluates for the kernels of sp_kernels.hip: argument structs and host + device
// arithmetic, no kernel.  The kernels' headers include it, and so does sp_launch.h for the API.
#pragma once

#include "sp_kernels_common.h"

namespace spk {

// k_finish_frames (sp_kernel_scratch.h)
struct FinishArgs {
    const uint8_t *bytes;
    int64_t nbytes, nelem;
    double stride;
    int32_t n, width, format;
    double block_norm_db, gain, range;
    const double *frame_min, *frame_max;
    uint8_t *gauge_mins, *gauge_maxs, *gauge_amps;
    unsigned long long *mm_acc;   // [2] bit patterns of min / max |X|^2 over all frames; reset to {+inf, 0} here
    double *out_minmax;       // [2] or nullptr
    // histograms: the scratch kernel adds into context-owned accumulators (zero before and after every request);
    // this kernel moves them to the caller's arrays, so a reply always holds the counts of its own request
    int32_t lut_len;
    unsigned long long *acc_c, *acc_cb;
    unsigned long long *out_c, *out_cb;   // or nullptr
};

// k_synth_trinoise (sp_synth.h)
struct SynthArgs {
    uint8_t *out;
    uint64_t t0, count;
    uint32_t seed, step, gshift;
    double amp, namp;
};

}  // namespace spk

// sp_index_to_rgba's table travels in the kernel arguments (1 KiB): nothing to copy, nothing of the caller's to keep alive
struct IndexLut {
    uint32_t v[256];
};

// k_density_count's decomposition: a workgroup counts a rectangle of the index image - `rows` image rows x `frames` frames - into one
// u32[256] histogram per row in LDS and then adds its non-zero cells to the caller's array.  It depends on n, the layout and the frame
// range only.  Spectrogram layout (a row's frames are consecutive bytes): 8 rows x 2048 frames, 8 KiB of LDS, 16 Ki pixels against at
// most 2048 global atomics.  Waterfall layout (a frame's bins are consecutive bytes, so a workgroup wants many bins for whole
// cache lines): 64 rows x 512 frames, 64 KiB of LDS, 32 Ki pixels against at most 16 Ki global atomics.
constexpr int kDensityThreads = 256;
constexpr int kDensityRowsSpectrogram = 8, kDensityFramesSpectrogram = 2048;
constexpr int kDensityRowsWaterfall = 64, kDensityFramesWaterfall = 512;

struct DensityShape {
    int rows, frames;          // of one workgroup's rectangle
    long long bands, pieces;   // ceil(n / rows) bands of rows x ceil(range / frames) pieces of frames: workgroup = band * pieces + piece
};

__host__ __device__ inline DensityShape density_shape(int n, bool waterfall, int x_begin, int x_end)
{
    DensityShape d;
    d.rows = waterfall ? kDensityRowsWaterfall : kDensityRowsSpectrogram;
    d.frames = waterfall ? kDensityFramesWaterfall : kDensityFramesSpectrogram;
    d.bands = ((long long)n + d.rows - 1) / d.rows;
    d.pieces = ((long long)x_end - x_begin + d.frames - 1) / d.frames;
    return d;
}

// the rectangle of workgroup wg: rows [y0, y1) x frames [x0, x1), inside [0, n) x [x_begin, x_end)
__host__ __device__ inline void density_rect(const DensityShape &d, int n, int x_begin, int x_end, long long wg, int &y0, int &y1, int &x0,
                                             int &x1)
{
    const long long band = wg / d.pieces, piece = wg % d.pieces;
    const long long ya = band * d.rows, yb = ya + d.rows, xa = x_begin + piece * d.frames, xb = xa + d.frames;
    y0 = (int)ya;
    y1 = (int)(yb < n ? yb : n);
    x0 = (int)xa;
    x1 = (int)(xb < x_end ? xb : x_end);
}
