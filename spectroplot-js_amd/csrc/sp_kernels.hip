// sp_kernels.hip — every kernel outside the frame-loop objects (sp_inst_frames.hip) and its launcher (sp_launch.h): the scratch
// kernels in all their formats, the synthesiser and the small kernels around the frame loops.  The only unit that includes their
// headers: host code reaches them through the launchers, so no change to it rebuilds or moves a kernel.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "sp_launch.h"
#include "sp_kernel_scratch.h"
#include "sp_kernel_mean.h"
#include "sp_synth.h"
#include "sp_kernel_index.h"
#include "sp_kernel_density.h"
#include "sp_kernel_small.h"

namespace {

template <typename F>
int dispatch_format(int32_t fmt, F &&f)
{
    switch (fmt) {
#define SP_CASE(X) case X: f(std::integral_constant<int, X>{}); return SP_OK;
        SP_FORMATS_BUT_CF64(SP_CASE) SP_CASE(SP_FMT_CF64)
#undef SP_CASE
    default: return SP_ERR_INVALID_ARG;
    }
}

// A scratch kernel's format and WIDE variant: launch(F, WIDE, grid, block) - F: the format as an integral_constant, WIDE:
// std::true_type where spk::scratch_wide(n).
template <typename Launch>
int dispatch_scratch(int format, int n, unsigned blocks, Launch &&launch)
{
    return dispatch_format(format, [&](auto F) {
        const dim3 grid(blocks), block(spk::kScratchThreads);
        if (spk::scratch_wide(n)) launch(F, std::true_type{}, grid, block);
        else launch(F, std::false_type{}, grid, block);
    });
}

// workgroups of 256 threads for `units` threads; false: more than one grid holds
bool blocks_of_256(size_t units, unsigned *blocks)
{
    const size_t b = (units + 255) / 256;
    *blocks = (unsigned)b;
    return b <= 0x7fffffffull;
}

}  // namespace

namespace spk {

int launch_scratch_radix2(const FrameArgs &a, int format, unsigned blocks, bool hold, int peak_m, int peak_nsamp, hipStream_t stream)
{
    return dispatch_scratch(format, a.n, blocks, [&](auto F, auto WIDE, dim3 grid, dim3 block) {
        constexpr int FMT = decltype(F)::value;
        constexpr bool W = decltype(WIDE)::value;
        if (hold) hipLaunchKernelGGL((k_scratch_radix2<FMT, W, true>), grid, block, 0, stream, a, peak_m, peak_nsamp);
        else hipLaunchKernelGGL((k_scratch_radix2<FMT, W, false>), grid, block, 0, stream, a, 1, peak_nsamp);
    });
}

int launch_scratch_traces(const FrameArgs &a, int format, unsigned blocks, unsigned long long *ws, hipStream_t stream)
{
    return dispatch_scratch(format, a.n, blocks, [&](auto F, auto WIDE, dim3 grid, dim3 block) {
        hipLaunchKernelGGL((k_scratch_traces<decltype(F)::value, decltype(WIDE)::value>), grid, block, 0, stream, a, ws);
    });
}

int launch_scratch_power(const FrameArgs &a, int format, unsigned blocks, double *power, hipStream_t stream)
{
    return dispatch_scratch(format, a.n, blocks, [&](auto F, auto WIDE, dim3 grid, dim3 block) {
        hipLaunchKernelGGL((k_scratch_power<decltype(F)::value, decltype(WIDE)::value>), grid, block, 0, stream, a, power);
    });
}

void launch_finish_frames(const FinishArgs &a, hipStream_t stream)
{
    int blocks = 3 * ((a.width + kFinishThreads - 1) / kFinishThreads);   // three roles per 256 frames
    const int bins = a.lut_len > SP_CB_HIST_SIZE ? a.lut_len : SP_CB_HIST_SIZE;   // it also moves the histograms
    const int hb = (bins + kFinishThreads - 1) / kFinishThreads;
    if (blocks < hb) blocks = hb;
    blocks += 1;          // the dBfs range: a workgroup of its own, behind neither the histograms nor a gauge
    hipLaunchKernelGGL(k_finish_frames, dim3((unsigned)blocks), dim3(kFinishThreads), 0, stream, a);
}

void launch_traces_clear(unsigned long long *ws, int n, hipStream_t stream)
{
    hipLaunchKernelGGL(k_traces_clear, dim3((unsigned)((2 * n + 255) / 256)), dim3(256), 0, stream, ws, n);
}

void launch_traces_finish(const unsigned long long *ws, int n, double block_norm_db, double gain, double *trace_min, double *trace_max,
                          hipStream_t stream)
{
    hipLaunchKernelGGL(k_traces_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, ws, n, block_norm_db, gain, trace_min, trace_max);
}

void launch_power_to_db(const double *d_power, size_t count, double block_norm_db, double gain, double *d_db, int cu_count, hipStream_t stream)
{
    size_t blocks = (count + 255) / 256;
    const size_t most = 16 * (size_t)cu_count;   // (a grid-stride loop: enough workgroups to fill the chip)
    if (blocks > most) blocks = most;
    hipLaunchKernelGGL(k_power_to_db, dim3((unsigned)blocks), dim3(256), 0, stream, d_power, count, block_norm_db, gain, d_db);
}

void mean_launch_shape(int n, long long frames, int cu_count, long long shape[3])
{
    const int pieces = mean_pieces(n, frames, cu_count);
    shape[0] = mean_bands(n), shape[1] = pieces, shape[2] = (frames + pieces - 1) / pieces;
}

void launch_mean_accumulate(const double *plane, int n, long long frames, unsigned long long *ws, int cu_count, hipStream_t stream)
{
    long long shape[3];
    mean_launch_shape(n, frames, cu_count, shape);
    hipLaunchKernelGGL(k_mean_accumulate, dim3((unsigned)shape[0], (unsigned)shape[1]), dim3(kMeanThreads), 0, stream, plane, n, frames, shape[2], ws);
}

void launch_mean_finish(const unsigned long long *ws, int n, int width, double *mean, hipStream_t stream)
{
    hipLaunchKernelGGL(k_mean_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, ws, n, width, mean);
}

int launch_synth_trinoise(const SynthArgs &a, int format, hipStream_t stream)
{
    unsigned blocks;
    if (!blocks_of_256(a.count, &blocks)) return SP_ERR_UNSUPPORTED;
    return dispatch_format(format, [&](auto F) {
        hipLaunchKernelGGL(k_synth_trinoise<decltype(F)::value>, dim3(blocks), dim3(256), 0, stream, a);
    });
}

void launch_noop(hipStream_t stream) { hipLaunchKernelGGL(k_noop, dim3(1), dim3(64), 0, stream); }

int launch_extract_index(const uint8_t *rgba, uint8_t *index, size_t row_px, size_t rows, size_t pitch_px, hipStream_t stream)
{
    unsigned blocks;
    if (!blocks_of_256(((row_px + 3) / 4) * rows, &blocks)) return SP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_extract_index, dim3(blocks), dim3(256), 0, stream, rgba, index, row_px, rows, pitch_px);
    return SP_OK;
}

int launch_index_to_rgba(const uint8_t *index, size_t pixels, const IndexLut &lut, uint8_t *rgba, hipStream_t stream)
{
    const size_t blocks = (pixels / 16 + 255) / 256 + 1;
    if (blocks > 0x7fffffffull) return SP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_index_to_rgba, dim3((unsigned)blocks), dim3(256), 0, stream, index, pixels, lut, rgba);
    return SP_OK;
}

int launch_density_count(const uint8_t *index, int n, int width, bool waterfall, int x_begin, int x_end, int lut_len, uint32_t *density,
                         hipStream_t stream)
{
    const DensityShape d = density_shape(n, waterfall, x_begin, x_end);
    const long long grid = d.bands * d.pieces;
    if (grid > 0x7fffffffll) return SP_ERR_UNSUPPORTED;
    if (waterfall)
        hipLaunchKernelGGL(k_density_count<true>, dim3((unsigned)grid), dim3(kDensityThreads), 0, stream, index, n, width, x_begin, x_end, lut_len,
                           density);
    else
        hipLaunchKernelGGL(k_density_count<false>, dim3((unsigned)grid), dim3(kDensityThreads), 0, stream, index, n, width, x_begin, x_end, lut_len,
                           density);
    return SP_OK;
}

void launch_merge_replies(const unsigned long long *rec, int count, int lut_len, size_t rank_stride, int renders, unsigned long long *c_hist,
                          unsigned long long *cb_hist, double *minmax, hipStream_t stream)
{
    const int total = lut_len + SP_CB_HIST_SIZE + 2;
    hipLaunchKernelGGL(k_merge_replies, dim3((unsigned)((total + 255) / 256), (unsigned)renders), dim3(256), 0, stream, rec, count, lut_len,
                       rank_stride, c_hist, cb_hist, minmax);
}

int launch_place_strips(bool wide, uint8_t *image, const uint8_t *strips, int count, int n, int width, int slice_width, int waterfall,
                        hipStream_t stream)
{
    unsigned blocks;
    if (!blocks_of_256((size_t)slice_width * (size_t)n * (size_t)count / (wide ? 4 : 1), &blocks)) return SP_ERR_UNSUPPORTED;
    if (wide) hipLaunchKernelGGL(k_place_strips<uint4>, dim3(blocks), dim3(256), 0, stream, image, strips, count, n, width, slice_width, waterfall);
    else hipLaunchKernelGGL(k_place_strips<uint32_t>, dim3(blocks), dim3(256), 0, stream, image, strips, count, n, width, slice_width, waterfall);
    return SP_OK;
}

void launch_batch_clear(const spk2::BatchItem *items, unsigned count, int lut_len, hipStream_t stream)
{
    hipLaunchKernelGGL(k_batch_clear, dim3(count), dim3(256), 0, stream, items, lut_len);
}

}  // namespace spk
