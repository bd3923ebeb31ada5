// sp_geometry.cpp — a request's frame geometry, the peak detector's sub-frame rule and the upload plan (see sp_geometry.h).
// Compiled with -ffp-contract=off.
#include "sp_geometry.h"

#include <cmath>
#include <cstring>
#include <utility>

#include "../../include/spectroplot_hip.h"

namespace spgeo {

Geometry geometry(const spfmt::Format &f, int32_t n, size_t nbytes, int32_t width)
{
    Geometry g;
    g.n = n;
    g.width = width;
    g.sample_width = f.width;
    g.nbytes = nbytes;
    g.sample_count = (double)nbytes / (double)f.width;
    g.nsamp = (int64_t)std::floor(g.sample_count);
    if (width == 1) {
        g.in_bounds = (size_t)n * (size_t)f.width <= nbytes;
    } else if (width > 1) {
        g.stride = (g.sample_count - (double)n) / (double)(width - 1);
        // do all frames lie inside the buffer?
        if (g.stride >= 0.0 && std::isfinite(g.stride) && 0.5 + g.stride * (double)(width - 1) < 2147483647.0)
            g.in_bounds = (size_t)(g.start(width - 1) + n) * (size_t)f.width <= nbytes;
    }
    return g;
}

PeakShape peak_shape(const Geometry &g)
{
    PeakShape ps;
    ps.nsamp = g.nsamp;
    if (g.width < 1) return ps;
    ps.last_count = 1;
    if (g.width < 2) return ps;
    if (!std::isfinite(g.stride) || !(g.stride >= 2.0 * (double)g.n)) return ps;
    const double m = std::floor(g.stride / (double)g.n);
    ps.m = m < 2147483647.0 ? (int32_t)m : 2147483647;
    const int64_t p = g.start(g.width - 1);
    for (int32_t j = 1; j < ps.m && (double)(p + ((int64_t)j + 1) * g.n) <= g.sample_count; j++) ps.last_count = j + 1;
    return ps;
}

// A request is packed, or pipelined in chunks, only with every frame's start well inside int32.  The bound is a condition of the upload
// plan, stricter than Geometry::in_bounds' - stated here once, not a second derivation of the stride.
static bool starts_fit_packing(const Geometry &g)
{
    return g.stride >= 0.0 && std::isfinite(g.stride) && 0.5 + g.stride * (double)(g.width - 1) < 2147483000.0;
}

// Cuts [0, width) at `bounds` and lays every chunk out; false = this request is not worth packing or cannot be (then nothing is used).
static bool build_packed_chunks(const Geometry &g, const std::vector<int32_t> &bounds, std::vector<PackedChunk> &out, size_t *dev_bytes,
                                size_t *link_bytes)
{
    const int n = g.n, sample_width = g.sample_width;
    const int32_t width = g.width;
    const size_t nbytes = g.nbytes;
    const double stride = g.stride;
    out.clear();
    if (width < 2 || !(stride > (double)n) || !starts_fit_packing(g)) return false;
    const int64_t F = (int64_t)std::floor(stride);
    const double frac = stride - (double)F;
    size_t off = 256, moved = 0;
    for (size_t c = 0; c + 1 < bounds.size(); c++) {
        PackedChunk ch;
        ch.x0 = bounds[c];
        ch.x1 = bounds[c + 1];
        if (ch.x1 <= ch.x0) continue;
        ch.first = g.start(ch.x0);
        ch.F = F;
        const int rows = ch.x1 - ch.x0;
        ch.drift.resize((size_t)rows);
        for (int j = 0; j < rows; j++) {
            const int64_t d = g.start(ch.x0 + j) - ch.first - (int64_t)j * F;
            if (d < 0 || d > (int64_t)rows) return false;       // (0 <= d_j <= j in exact arithmetic)
            ch.drift[(size_t)j] = (int32_t)d;
        }
        // the frame must also END inside the capture (the caller established in_bounds for the request as a whole)
        if ((size_t)(ch.first + (int64_t)(rows - 1) * F + ch.drift[(size_t)rows - 1] + n) * (size_t)sample_width > nbytes) return false;
        // runs of rows whose drifts stay within `span` samples of each other: one pitched copy each, its rows widened by the run's drift
        // range.  A copy call costs the link ~11 us (tools/pcie_probe.hip: 17 MiB in 16 pitched copies 0.49 ms, in one 0.32 ms), a
        // widened row span / 2 samples on average: rows * frac / span calls against rows * span / 2 samples at ~55 GB/s balance at
        // span = sqrt(2 * 11 us * frac * 55 GB/s / bytes per sample) - 275 samples for cf32 at frac = 0.5 - kept within [16, n/2].
        int32_t span = (int32_t)std::sqrt(2.0 * 11e-6 * (frac > 1e-3 ? frac : 1e-3) * 55e9 / (double)sample_width);
        span = span > n / 2 ? n / 2 : span;
        span = span < 16 ? 16 : span;
        int32_t widest = 0;
        for (int j = 0; j < rows;) {
            PackedBlock b{j, j + 1, ch.drift[(size_t)j], ch.drift[(size_t)j]};
            while (b.j1 < rows) {
                const int32_t d = ch.drift[(size_t)b.j1];
                const int32_t lo = d < b.dmin ? d : b.dmin, hi = d > b.dmax ? d : b.dmax;
                if (hi - lo > span) break;
                b.dmin = lo;
                b.dmax = hi;
                b.j1++;
            }
            moved += (size_t)(b.j1 - b.j0) * (size_t)(n + b.dmax - b.dmin) * (size_t)sample_width;
            if (b.dmax - b.dmin > widest) widest = b.dmax - b.dmin;
            ch.blocks.push_back(b);
            j = b.j1;
        }
        // device rows P apart: wide enough that a widened row ends where the next one begins (row j of a run lands at j P + dmin and is
        // n + dmax - dmin long); the frames themselves sit at j P + d_j, their drift accumulating as it does in the capture
        ch.P = (int64_t)n + widest;
        ch.stride2 = (double)ch.P + frac;
        if (!((double)(ch.P + 1) * (double)width < 2147483000.0)) return false;       // the kernel's positions are int32
        ch.pos2_x0 = spjs::to_int32(0.5 + ch.stride2 * (double)ch.x0);
        for (int j = 0; j < rows; j++) {
            const int64_t pos2 = spjs::to_int32(0.5 + ch.stride2 * (double)(ch.x0 + j));
            if (pos2 - ch.pos2_x0 != (int64_t)j * ch.P + ch.drift[(size_t)j]) return false;   // the two sides of the identity rounded apart
            if (j == rows - 1) ch.pos2_last = pos2;
        }
        ch.dev_off = off;
        off += ((size_t)((int64_t)rows * ch.P + ch.drift[(size_t)rows - 1] + widest) * (size_t)sample_width + 255) & ~(size_t)255;
        out.push_back(std::move(ch));
    }
    *dev_bytes = off + 256;
    *link_bytes = moved;
    // worth it only if clearly fewer bytes cross the link, and not in a hail of small copies
    size_t copies = 0;
    for (const PackedChunk &ch : out) copies += ch.blocks.size();
    return !out.empty() && moved <= nbytes / 4 * 3 && copies <= 512;
}

// How [0, width) is cut into chunks of frames for a request that moves in_est bytes of samples in and out_bytes of image out.
static void chunk_bounds(int32_t width, size_t in_est, size_t out_bytes, bool chunkable, std::vector<int32_t> &bounds)
{
    int chunks = 1;
    if (chunkable && width >= 1024 && in_est + out_bytes >= ((size_t)16 << 20)) chunks = in_est + out_bytes >= ((size_t)64 << 20) ? kMaxChunks : 4;
    // The busier direction of the link never pauses; what does not overlap it is one chunk's way in the other direction plus its
    // render: the LAST chunk's image when the samples are the longer transfer, the FIRST chunk's samples when the image is.  So the
    // chunks shrink (or grow) geometrically towards that end - each 0.65 of its neighbour, which also keeps the shorter direction
    // from falling behind - instead of being equal (measured, config 2: 8 equal chunks 2.73 ms, pure two-way copy 2.37 ms; every
    // additional copy call costs the link ~13 us, so few chunks).  Chunks end on multiples of 32 frames.
    const bool in_heavy = in_est >= out_bytes;
    double w[kMaxChunks], sum = 0, acc = 0;
    for (int k = 0; k < chunks; k++) sum += (w[k] = std::pow(0.65, in_heavy ? k : chunks - 1 - k));
    bounds.assign(1, 0);
    for (int k = 0; k + 1 < chunks; k++) {
        acc += w[k];
        const int32_t x = (int32_t)((int64_t)((double)width * acc / sum) & ~(int64_t)31);
        if (x > bounds.back() && x < width) bounds.push_back(x);
    }
    bounds.push_back(width);   // (width = 0: one empty chunk, so that the reply still gets its initial values)
}

void plan_upload(const Geometry &g, bool packable, bool chunkable, size_t out_bytes, UploadPlan &u)
{
    const bool fit = starts_fit_packing(g);
    // a sparse request (stride > n, every frame inside the capture) is cut by the bytes its frames read; if it cannot be packed after
    // all, it is cut again by the whole capture
    bool sparse = packable && fit && g.width >= 2 && g.stride > (double)g.n && g.in_bounds;
    for (;; sparse = false) {
        chunk_bounds(g.width, sparse ? (size_t)g.width * (size_t)g.n * (size_t)g.sample_width : g.nbytes, out_bytes, chunkable && fit, u.bounds);
        u.packed = sparse && build_packed_chunks(g, u.bounds, u.chunks, &u.dev_bytes, &u.link_bytes) && u.chunks.size() + 1 == u.bounds.size();
        if (u.packed || !sparse) break;
    }
    if (u.packed) return;
    u.chunks.clear();
    u.dev_bytes = g.nbytes + 16;
    u.link_bytes = g.nbytes;
}

const char *check_bands(int32_t n, const int32_t *bands, int32_t count)
{
    if (count < 0 || count > SP_MAX_BANDS) return "count must be 0 .. SP_MAX_BANDS";
    if (count > 0 && !bands) return "bands is null";
    for (int32_t b = 0; b < count; b++) {
        const int32_t y0 = bands[2 * b], y1 = bands[2 * b + 1];
        if (y0 < 0 || y1 < y0 || y1 > n) return "a band must satisfy 0 <= y0 <= y1 <= n";
    }
    return nullptr;
}

}  // namespace spgeo

extern "C" int sp_band_rows(int32_t n, double f_lo, double f_hi, int32_t *y0, int32_t *y1)
{
    if (!y0 || !y1 || f_lo != f_lo || f_hi != f_hi || f_lo > f_hi || n < 2) return SP_ERR_INVALID_ARG;
    if (n & (n - 1)) return SP_ERR_NOT_POW2;
    const double half = (double)(n / 2), dn = (double)n;
    const auto clamp = [dn](double v) { return (int32_t)(v < 0.0 ? 0.0 : v > dn ? dn : v); };   // (an infinity clamps; no NaN comes here)
    const int32_t a = clamp(std::ceil(half - f_hi * dn)), b = clamp(std::floor(half - f_lo * dn) + 1.0);
    *y0 = a;
    *y1 = b < a ? a : b;
    return SP_OK;
}

extern "C" int sp_peak_subframes(int32_t format, int32_t n, size_t nbytes, int32_t width, int32_t *subframes, int32_t *last_column_count)
{
    if (format < 0 || format >= SP_FMT_COUNT || n < 1 || width < 0) return SP_ERR_INVALID_ARG;
    const spgeo::PeakShape ps = spgeo::peak_shape(spgeo::geometry(spfmt::describe(format), n, nbytes, width));
    if (subframes) *subframes = ps.m;
    if (last_column_count) *last_column_count = ps.last_count;
    return SP_OK;
}

// (tests) The upload plan sp_render would use for a request of this shape - pure host arithmetic, no device.  out[]: packed (0 / 1),
// chunks, device bytes, link bytes; per chunk x0, x1 and, if packed, first, F, P, dev_off, pos2_x0, pos2_last, the bits of stride2,
// blocks, then j0, j1, dmin, dmax per block.
extern "C" int sp_debug_upload_plan(int32_t format, int32_t n, size_t nbytes, int32_t width, int32_t want_image, int64_t *out, size_t capacity,
                                    size_t *used)
{
    if (format < 0 || format >= SP_FMT_COUNT || n < 2 || width < 1 || !out || !used) return SP_ERR_INVALID_ARG;
    spgeo::UploadPlan u;
    spgeo::plan_upload(spgeo::geometry(spfmt::describe(format), n, nbytes, width), true, want_image != 0, 4 * (size_t)width * (size_t)n, u);
    std::vector<int64_t> v{u.packed ? 1 : 0, (int64_t)u.bounds.size() - 1, u.packed ? (int64_t)u.dev_bytes : 0, (int64_t)u.link_bytes};
    for (size_t c = 0; c + 1 < u.bounds.size(); c++) {
        v.push_back(u.bounds[c]);
        v.push_back(u.bounds[c + 1]);
        if (!u.packed) continue;
        const spgeo::PackedChunk &ch = u.chunks[c];
        int64_t bits;
        memcpy(&bits, &ch.stride2, 8);
        for (int64_t x : {ch.first, ch.F, ch.P, (int64_t)ch.dev_off, ch.pos2_x0, ch.pos2_last, bits, (int64_t)ch.blocks.size()}) v.push_back(x);
        for (const spgeo::PackedBlock &b : ch.blocks)
            for (int64_t x : {(int64_t)b.j0, (int64_t)b.j1, (int64_t)b.dmin, (int64_t)b.dmax}) v.push_back(x);
    }
    *used = v.size();
    if (v.size() > capacity) return SP_ERR_INVALID_ARG;
    memcpy(out, v.data(), v.size() * 8);
    return SP_OK;
}

// (tests) The slice layout of a sliced render of this shape (spgeo::SliceLayout) - pure host arithmetic, no device.  out[]: slice width,
// strip bytes, rest, the bands' pitch, row bytes and rows, the rest's offset, pitch, row bytes and rows; per strip its band's and its
// gauges' offset.
extern "C" int sp_debug_slice_layout(int32_t n, int32_t width, int32_t count, int32_t waterfall, int64_t *out, size_t capacity, size_t *used)
{
    if (n < 1 || width < 0 || count < 1 || !out || !used) return SP_ERR_INVALID_ARG;
    const spgeo::SliceLayout s(n, width, count, waterfall != 0);
    std::vector<int64_t> v;
    for (size_t x : {s.slice_width, s.strip_bytes(), s.rest, s.band_pitch(), s.band_row_bytes(), s.band_rows(), s.rest_offset(), s.rest_pitch(),
                     s.rest_row_bytes(), s.rest_rows()})
        v.push_back((int64_t)x);
    for (size_t r = 0; r < s.count; r++) {
        v.push_back((int64_t)s.band_offset(r));
        v.push_back((int64_t)s.gauge_offset(r));
    }
    *used = v.size();
    if (v.size() > capacity) return SP_ERR_INVALID_ARG;
    memcpy(out, v.data(), v.size() * 8);
    return SP_OK;
}
