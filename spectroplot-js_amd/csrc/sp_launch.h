// sp_launch.h — the launchers of every kernel outside the frame-loop objects (sp_kernels.hip): the scratch kernels, the synthesiser and
// the small kernels around the frame loops.  Plain functions, as spk2::launch_frames* are for the frame loops: arguments and a stream
// in, a status out where a launch can be refused - SP_ERR_INVALID_ARG for an unknown format, SP_ERR_UNSUPPORTED for work that does not
// fit one grid - and nothing is launched then.  The grid and block arithmetic that follows from a kernel's constants is the launcher's.
// The caller asks hipGetLastError() behind every launch.
#pragma once

#include "sp_kernel_args.h"

namespace spk2 {
struct BatchItem;   // sp_kernel_frames_batch.h
}

namespace spk {

// Whether a scratch kernel runs as its four-stage (WIDE) variant: from n = 4096 on, where every thread still has a 16-point item.
inline bool scratch_wide(int n) { return n >= 4096; }

// The scratch kernels over `blocks` workgroups (a.scratch holds their slabs); the four-stage variants where scratch_wide(a.n).
// k_scratch_radix2 holds the peak over peak_m sub-frames per column where `hold`.
int launch_scratch_radix2(const FrameArgs &a, int format, unsigned blocks, bool hold, int peak_m, int peak_nsamp, hipStream_t stream);
int launch_scratch_traces(const FrameArgs &a, int format, unsigned blocks, unsigned long long *ws, hipStream_t stream);
int launch_scratch_power(const FrameArgs &a, int format, unsigned blocks, double *power, hipStream_t stream);
// k_finish_frames behind a request's last scratch launch: three roles per 256 frames (at least enough threads to move the histograms)
// and the dBfs range's workgroup
void launch_finish_frames(const FinishArgs &a, hipStream_t stream);

void launch_traces_clear(unsigned long long *ws, int n, hipStream_t stream);
void launch_traces_finish(const unsigned long long *ws, int n, double block_norm_db, double gain, double *trace_min, double *trace_max,
                          hipStream_t stream);
// d_db[k] = dB of d_power[k], k < count (a grid-stride loop: no more workgroups than fill the chip)
void launch_power_to_db(const double *d_power, size_t count, double block_norm_db, double gain, double *d_db, int cu_count, hipStream_t stream);

// the `frames` > 0 frames of the frame-major plane (n rows each) added into the exact-sum workspace; the workspace into the mean
void launch_mean_accumulate(const double *plane, int n, long long frames, unsigned long long *ws, int cu_count, hipStream_t stream);
// ... and the grid launch_mean_accumulate gives k_mean_accumulate: {bands of rows, pieces of the frames, frames per piece}
void mean_launch_shape(int n, long long frames, int cu_count, long long shape[3]);
void launch_mean_finish(const unsigned long long *ws, int n, int width, double *mean, hipStream_t stream);
// the `frames` > 0 frames of the frame-major plane added into the variance workspace u64[spv::kSlots][n] (every value gives its pieces
// and its square's); the grid that gives k_variance_accumulate, {bands of rows, pieces of the frames, frames per piece}; and the
// workspace into out[3][n], the sum, the sum of squares and width * sum of squares - sum^2, each rounded once.  (The two kernels and
// these launchers are sp_variance.hip, a unit of their own.)
void launch_variance_accumulate(const double *plane, int n, long long frames, unsigned long long *ws, int cu_count, hipStream_t stream);
void variance_launch_shape(int n, long long frames, int cu_count, long long shape[3]);
void launch_variance_finish(const unsigned long long *ws, int n, int width, double *out, hipStream_t stream);
// out[(k * count + b) * stride + x_base + x] = the exact sum of (y - y0_b)^k times the rows [y0_b, y1_b) = [bands[2 b], bands[2 b + 1])
// of frame x of the frame-major plane, k = 0 .. order, for its `frames` > 0 frames and the `count` bands of the HOST array `bands`
// (1 .. SP_MAX_BANDS, each within 0 <= y0 <= y1 <= n: the caller has checked them); they travel in the kernel's arguments.  Order 0 is
// the band-power series, band[b * stride + x_base + x]; orders 1 and 2 are the moments (the caller has checked the order, and
// n <= SP_MAX_N above order 0).  One launch.  (k_band_sum<order> and this launcher are sp_band.hip, a unit of their own.)
void launch_band_sum(const double *plane, int n, long long frames, const int32_t *bands, int count, int order, double *out, long long stride,
                     long long x_base, hipStream_t stream);
// row[b * stride + x_base + x] and peak[b * stride + x_base + x] = the strongest row of the rows [bands[2 b], bands[2 b + 1]) of frame
// x and its value (-1 and a NaN where the band holds no value), for the plane, frames and bands of launch_band_sum; a null `row` or
// `peak` is not written.  One launch.  (k_track_max and this launcher are sp_track.hip, a unit of their own.)
void launch_track_max(const double *plane, int n, long long frames, const int32_t *bands, int count, int32_t *row, double *peak,
                      long long stride, long long x_base, hipStream_t stream);
// rows[y] += the frames of the plane whose row y reaches threshold[y] (n device doubles), and out[b * stride + x_base + x] += the rows
// of [bands[2 b], bands[2 b + 1]) of frame x that reach theirs, for the plane, frames and bands of launch_band_sum (`count` may be 0);
// a null `rows` or `out` is not touched, one of them is not null, and the caller has zeroed both.  One launch.  (k_occupancy_count and
// this launcher are sp_occupancy.hip, a unit of their own.)
void launch_occupancy_count(const double *plane, int n, long long frames, const double *threshold, const int32_t *bands, int count,
                            uint32_t *rows, uint32_t *out, long long stride, long long x_base, hipStream_t stream);
// keys[y * width + x_base + x] = the key (sp_track_core.h) of frame x, row y of the frame-major plane, for its `frames` > 0 frames: the
// block transposed into the workspace u64 keys[n][width] of a percentile request.  One launch.
void launch_quantile_gather(const double *plane, int n, long long frames, unsigned long long *keys, long long width, long long x_base,
                            hipStream_t stream);
// out[r * n + y] = element ranks[r] of row y's `width` keys sorted ascending, as a value's bits or the one NaN, for the `count` ranks of
// the HOST array `ranks` (1 .. SP_MAX_RANKS, each within 0 <= k < width: the caller has checked them); width == 0 gives NaNs.  One
// launch of n workgroups.  (k_quantile_gather, k_quantile_select and these launchers are sp_quantile.hip, a unit of their own.)
void launch_quantile_select(const unsigned long long *keys, int n, int width, const int32_t *ranks, int count, double *out, hipStream_t stream);
// The burst lists of the band-major series f64[count][width] at `series` (0 <= count <= SP_MAX_BANDS, width >= 0): counts[b] = the
// bursts of band b and edges[b][2 i], edges[b][2 i + 1] = the start and the end of burst i < max_bursts, against the HOST arrays
// hi_key[count] and lo_key[count] (spo::threshold_key of the thresholds; the caller has checked them).  Either output may be null; the
// caller has filled `edges` with -1.  `records`: burst_record_bytes(count, width) bytes of device memory, 8-byte aligned, for the
// segments' summaries and carries.  Three launches - one where width == 0, two where edges is null or max_bursts == 0 - none where
// count == 0.  (k_burst_summary, k_burst_carry, k_burst_emit and this launcher are sp_burst.hip, a unit of their own.)
size_t burst_record_bytes(int count, int width);
void launch_bursts(const double *series, int count, int width, const uint64_t *hi_key, const uint64_t *lo_key, int max_bursts,
                   unsigned long long *records, uint32_t *counts, int32_t *edges, hipStream_t stream);
// The burst measurements behind launch_bursts on the same series, keys and `records` (the carries are read from them): for the listed
// bursts i < min(counts[b], max_bursts) of band b energy[b][i], peak[b][i] and peak_at[b][i], each of which may be null - not all.
// `counts` is NOT null here: launch_bursts' counts, the caller's or a workspace's.  The caller has filled the three outputs with 0xFF
// bytes.  `work`: pulse_work_bytes(count, max_bursts) bytes of device memory, 8-byte aligned - the bursts' cells
// u64[count][max_bursts][spx::kSlots] and their peak keys u64[count][max_bursts] - which this zeroes on the stream in front.  A memset
// and up to three launches; none where count == 0, width == 0 or max_bursts == 0.  (k_pulse_accumulate, k_pulse_peak_frame,
// k_pulse_finish and this launcher are sp_pulse.hip, a unit of their own.)
size_t pulse_work_bytes(int count, int max_bursts);
hipError_t launch_pulses(const double *series, int count, int width, const uint64_t *hi_key, const uint64_t *lo_key, int max_bursts,
                         const unsigned long long *records, const uint32_t *counts, void *work, double *energy, double *peak,
                         int32_t *peak_at, hipStream_t stream);
// The lagged covariance sums of the band-major series f64[count][width] at `series` (width >= 0): out[3][npairs][lags] for the HOST
// array `pairs` of npairs index pairs (1 .. SP_MAX_LAG_PAIRS, each index within [0, count)) and the lags [0, lags), 1 <= lags <=
// SP_MAX_LAGS (the caller has checked them); every lag has width - lags + 1 terms, none where that is below 1, and the reply is zeros
// then.  `work`: lagcov_work_bytes(npairs, lags) bytes of device memory, 8-byte aligned - the (pair, lag)s' cells
// u64[spv::kSlots][npairs * lags] and the pairs' u64[npairs][66] - which this zeroes on the stream in front.  A memset and two launches,
// one where there is no term.  ... and the grid it gives k_lagcov_accumulate: {pairs times bands of 32 lags, pieces of the terms,
// terms per piece}.  (k_lagcov_accumulate, k_lagcov_finish and this launcher are sp_lagcov.hip, a unit of their own.)
size_t lagcov_work_bytes(int npairs, int lags);
hipError_t launch_lagcov(const double *series, long long width, const int32_t *pairs, int npairs, int lags, void *work, double *out,
                         int cu_count, hipStream_t stream);
void lagcov_launch_shape(int npairs, int lags, long long terms, int cu_count, long long shape[3]);

// out[c * n + y] = RN(exact sum of the rows y of column c's frames) / the column's frames, for the columns of `group` >= 1 frames each
// that the `frames` > 0 frames of the frame-major plane make: ceil(frames / group) of them, only the last one short.  One launch, no
// workspace.  ... and the grid it gives k_blockmean: {bands of rows, pieces of the columns, columns per piece}.  (k_blockmean,
// k_power_to_index and these launchers are sp_blockmean.hip, a unit of their own.)
void launch_blockmean(const double *plane, int n, long long frames, long long group, double *out, int cu_count, hipStream_t stream);
void blockmean_launch_shape(int n, long long frames, long long group, int cu_count, long long shape[3]);
// index[pixel of (x, y)] = the colour index of power[x * n + y] against the lut_len <= 256 device doubles at gray_edge, for the `width`
// > 0 frames of the plane, at the pixel positions of an index image in the layout `waterfall` names.  One launch;
// SP_ERR_UNSUPPORTED for a LUT a byte cannot index or more than 65535 bands of 64 rows.
int launch_power_to_index(const double *power, int n, int width, bool waterfall, const double *gray_edge, int lut_len, uint8_t *index,
                          hipStream_t stream);

int launch_synth_trinoise(const SynthArgs &a, int format, hipStream_t stream);

void launch_noop(hipStream_t stream);
int launch_extract_index(const uint8_t *rgba, uint8_t *index, size_t row_px, size_t rows, size_t pitch_px, hipStream_t stream);
int launch_index_to_rgba(const uint8_t *index, size_t pixels, const IndexLut &lut, uint8_t *rgba, hipStream_t stream);
// the frames [x_begin, x_end), x_begin < x_end, of an index image ADDED to `density`
int launch_density_count(const uint8_t *index, int n, int width, bool waterfall, int x_begin, int x_end, int lut_len, uint32_t *density,
                         hipStream_t stream);

// `renders` records of lut_len + SP_CB_HIST_SIZE + 2 words per rank, merged one by one (sp_merge_replies: one)
void launch_merge_replies(const unsigned long long *rec, int count, int lut_len, size_t rank_stride, int renders, unsigned long long *c_hist,
                          unsigned long long *cb_hist, double *minmax, hipStream_t stream);
// `wide`: 16-byte units (the caller has checked widths and alignment), else one pixel per thread
int launch_place_strips(bool wide, uint8_t *image, const uint8_t *strips, int count, int n, int width, int slice_width, int waterfall,
                        hipStream_t stream);
void launch_batch_clear(const spk2::BatchItem *items, unsigned count, int lut_len, hipStream_t stream);

}  // namespace spk
