// sp_geometry.h — where the frames of a request lie in its capture, and how its samples travel to the device: pure host arithmetic,
// no HIP.  A request's frame geometry has ONE definition, `Geometry`; the peak detector's sub-frame rule and the host render's
// upload plan are computed from it.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "sp_formats.h"

namespace spgeo {

// The frame geometry of one request (format, n, nbytes, width), in the reference's arithmetic.
struct Geometry {
    int32_t n = 0, width = 0, sample_width = 1;
    size_t nbytes = 0;
    double sample_count = 0;   // byteLength / sampleWidth                                                    samples.js:167
    int64_t nsamp = 0;         // floor(sample_count)
    double stride = 0;         // (sample_count - n) / (width - 1), samples between two frames' starts        worker.js:50
                               // (one frame or none: 0 - (S - n) / 0 is an infinity or a NaN and ~~(0.5 + it * 0) = 0, as with 0)
    bool in_bounds = false;    // every frame lies inside the capture, every start is a plain int32 (ToInt32 is then truncation)
    // the sample where frame x starts: ~~(0.5 + stride * x)                                                  worker.js:72
    int64_t start(int32_t x) const { return spjs::to_int32(0.5 + stride * (double)x); }
};
Geometry geometry(const spfmt::Format &f, int32_t n, size_t nbytes, int32_t width);

// The peak detector's sub-frame rule (include/spectroplot_hip.h, enum sp_detector): M sub-frames per column and how many of them the
// last column has, and floor(sampleCount), which every sub-frame j >= 1 must end at or before.  The only definition behind
// sp_peak_subframes.  (PeakShape{}: the sample detector's request - one sub-frame, nothing to hold.)
struct PeakShape {
    int32_t m = 1, last_count = 0;
    int64_t nsamp = 0;
};
PeakShape peak_shape(const Geometry &g);

// ---- sparse requests: upload only what the frames read --------------------------------------------------------------------------------
// With stride > n the reference's loop touches n samples per frame and skips the rest (lib/worker.js:50, 70-75) - its interactive shape:
// a long capture at a screen-wide `width`.  Copying the capture contiguously moves stride / n times the bytes any frame reads.  Instead
// a chunk's frames travel as the rows of pitched copies (hipMemcpy2DAsync: source rows floor(stride) samples apart) into a packed device
// buffer whose rows are P samples apart, and the kernel is launched on that buffer with the stride P + frac(stride): frame x then
// starts at ~~(0.5 + (P + frac) x) = P x + floor(0.5 + frac x), which is where the pitched copy put it, because the capture has it at
// floor(stride) x + floor(0.5 + frac x).  The identity holds in exact arithmetic; the two sides round differently in f64, so the host
// evaluates both for EVERY frame and takes the contiguous path if a single one disagrees.  The start's fractional drift within a chunk
// (d_j = start_j - start_0 - j floor(stride), 0 <= d_j <= j) is what a pitched copy cannot follow row by row: it covers a run of rows
// whose drifts differ by at most `span` samples and brings that many samples more per row (span: a few hundred samples, at most n/2,
// chosen in build_packed_chunks to balance the cost of a copy call against the extra bytes); P = n + the widest run's range.
// A frame's centre sample (gauge_amps) lies inside the frame, and nothing else of the path depends on where a frame came from.
struct PackedBlock {
    int32_t j0, j1;        // rows of the chunk (frame x0 + j)
    int32_t dmin, dmax;    // their drifts lie in [dmin, dmax]
};
struct PackedChunk {
    int32_t x0 = 0, x1 = 0;
    int64_t first = 0;     // the capture's sample where frame x0 starts
    int64_t F = 0;         // samples between the capture's rows: floor(stride)
    int64_t P = 0;         // samples between the device rows
    size_t dev_off = 0;    // the chunk's byte offset in the staging buffer
    double stride2 = 0;    // P + frac(stride): the kernel's stride
    int64_t pos2_x0 = 0;   // ~~(0.5 + stride2 * x0): the kernel's start of frame x0
    int64_t pos2_last = 0; // ... and of frame x1 - 1
    std::vector<PackedBlock> blocks;
    std::vector<int32_t> drift;   // d_j per row
};

// the most chunks a request is cut into (chunk_bounds); the host render keeps a pair of events per chunk
constexpr int kMaxChunks = 6;

// How a request's samples travel to the device: [0, width) cut into chunks of frames and, for a sparse request, every chunk's packed
// layout.
struct UploadPlan {
    bool packed = false;
    std::vector<int32_t> bounds;         // chunk k: frames [bounds[k], bounds[k + 1])
    std::vector<PackedChunk> chunks;     // packed: chunk k's layout
    size_t dev_bytes = 0, link_bytes = 0;   // the staging buffer it needs; what crosses the link
};
// packable: the request's kernel can read a packed chunk; chunkable: the request may be pipelined; out_bytes: the image that comes
// back over the link.
void plan_upload(const Geometry &g, bool packable, bool chunkable, size_t out_bytes, UploadPlan &u);

// ---- band-power series: bands of image rows -----------------------------------------------------------------------------------------
// What every band-power entry point refuses of its bands (include/spectroplot_hip.h): nullptr where they are in order - count within
// 0 .. SP_MAX_BANDS, `bands` non-null where count > 0, every band within 0 <= y0 <= y1 <= n - else the refusal's text.
const char *check_bands(int32_t n, const int32_t *bands, int32_t count);

// ---- sliced renders: where the strips of `count` workers lie in the caller's image --------------------------------------------------
// The caller's layout (lib/spectroplot.js:1206-1244), in bytes of the RGBA image: every worker renders sliceWidth = ~~(width / workers)
// frames (:1208) and strip r is put at (r * sliceWidth, 0) of the width x n spectrogram - a band of columns - or at
// (0, width - sliceWidth - r * sliceWidth) of the n x width waterfall - a band of rows, in reverse order (:1244).  The
// width - workers * sliceWidth frames that no worker renders stay as the caller's fresh canvas has them: clear.  Bands and rest are
// rectangles of `rows` rows of `row_bytes`, `pitch` bytes apart; a row band is one row.  The host-side twin of k_place_strips.
struct SliceLayout {
    size_t n, width, count;
    bool waterfall;
    size_t slice_width, rest;   // frames per strip; frames no strip draws
    SliceLayout(int32_t n_, int32_t width_, int32_t count_, bool waterfall_)
        : n((size_t)n_), width((size_t)width_), count((size_t)count_), waterfall(waterfall_), slice_width((size_t)(width_ / count_)),
          rest(width - slice_width * count)
    {
    }
    size_t image_bytes() const { return 4 * width * n; }
    size_t strip_bytes() const { return 4 * slice_width * n; }
    size_t band_offset(size_t r) const { return waterfall ? 4 * n * (width - slice_width - slice_width * r) : 4 * slice_width * r; }
    size_t band_pitch() const { return waterfall ? strip_bytes() : 4 * width; }
    size_t band_row_bytes() const { return waterfall ? strip_bytes() : 4 * slice_width; }
    size_t band_rows() const { return waterfall ? 1 : n; }
    size_t gauge_offset(size_t r) const { return slice_width * r; }   // slice r's gauges: columns [r * sliceWidth, (r + 1) * sliceWidth)
    size_t rest_offset() const { return waterfall ? 0 : 4 * slice_width * count; }
    size_t rest_pitch() const { return waterfall ? 4 * n * rest : 4 * width; }
    size_t rest_row_bytes() const { return waterfall ? 4 * n * rest : 4 * rest; }
    size_t rest_rows() const { return waterfall ? 1 : n; }
};

}  // namespace spgeo
