// sp_api.hip — C ABI of the library (include/spectroplot_hip.h): contexts, plans, the frame-loop launch.
//
// One sp_context mirrors one reference Worker instance (lib/spectroplot.js:85-116): requests run in order on
// its stream.  A plan holds everything the reference computes once per request before its frame loop
// (lib/worker.js:30-62) plus the threshold tables that stand in for the per-pixel Math.log10.
//
// Host code only: the frame-loop kernels are reached through spk2::launch_frames* (sp_inst_frames.hip), every other kernel through the
// launchers of sp_launch.h (sp_kernels.hip).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/spectroplot_hip.h"
#include "sp_geometry.h"
#include "sp_host.h"
#include "sp_kernel_frames_batch.h"
#include "sp_kernel_frames_peak.h"
#include "sp_kernel_frames_traces.h"
#include "sp_kernel_frames_power.h"
#include "sp_kernel_frames_index.h"
#include "sp_launch.h"
#include "sp_exact_sum.h"
#include "sp_track_core.h"
#include "sp_occupancy_core.h"
#include "sp_quantile_core.h"
#include "sp_burst_core.h"
#include "sp_pulse_core.h"
#include "sp_blockmean_core.h"
#include "sp_moment_core.h"
#include "sp_variance_core.h"
#include "sp_lagcov_core.h"
#include "sp_cmap_tables.h"

namespace {

struct DeviceBuffer {
    void *p = nullptr;
    size_t cap = 0;
    int reserve(size_t bytes)
    {
        if (bytes <= cap) return SP_OK;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        size_t want = bytes + bytes / 8 + 256;
        if (hipMalloc(&p, want) != hipSuccess) {
            if (hipMalloc(&p, bytes) != hipSuccess) return SP_ERR_NOMEM;
            want = bytes;
        }
        cap = want;
        return SP_OK;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

// page-locked host memory owned by a context (the landing place of a reply's small outputs)
struct HostBuffer {
    void *p = nullptr;
    size_t cap = 0;
    int reserve(size_t bytes)
    {
        if (bytes <= cap) return SP_OK;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
        const size_t want = bytes + bytes / 8 + 256;
        if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) return SP_ERR_NOMEM;
        cap = want;
        return SP_OK;
    }
    void release()
    {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
};

// sp_render_named: the names and numbers of the last request and the arrays built from them (windowc empty: none is remembered - the
// cached plan came from arrays, or the render failed)
struct NamedRequest {
    std::string format, window, cmap;
    int32_t n = 0, channel_mode = 0, waterfall = 0;
    double gain = 0, range = 0;   // compared bit by bit
    std::vector<double> windowc;
    std::vector<uint8_t> lut;
    double block_norm = 0;
    static std::string str(const char *s) { return s ? s : ""; }
    bool same(const sp_named_request &r) const
    {
        return !windowc.empty() && format == str(r.format) && window == str(r.window) && cmap == str(r.cmap) && n == r.n
               && channel_mode == (r.channel_mode ? 1 : 0) && waterfall == (r.waterfall ? 1 : 0) && !memcmp(&gain, &r.gain, 8)
               && !memcmp(&range, &r.range, 8);
    }
};

}  // namespace

struct sp_context {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    std::string error;
    int cu_count = 256;          // what every launch is shaped by: the device's own count, or sp_context_debug_set_cu_count's
    int device_cu_count = 256;   // hipGetDeviceProperties' multiProcessorCount (what an override of 0 puts back)
    // workspace of the frame loop
    DeviceBuffer frame_minmax;   // 2 * width doubles (the scratch kernel's frame extremes, read by k_finish_frames)
    DeviceBuffer partial;        // [0,4) the number of the last request k_frames has started; the scratch kernel's {min,max} and histogram accumulators
    DeviceBuffer scratch;        // scratch kernel slabs
    DeviceBuffer traces_ws;      // a traces request's extremes per bin, u64[2 n] (sp_kernel_scratch.h: k_traces_clear)
    DeviceBuffer power_plane;    // sp_render_power: the request's plane on the device, 8 * width * n bytes (grown, never shrunk)
    DeviceBuffer mean_ws;        // a mean request's exact-sum cells, u64[spx::kSlots][n] (sp_kernel_mean.h; grown, never shrunk)
    DeviceBuffer variance_ws;    // a variance request's cells, u64[spv::kSlots][n] (sp_kernel_variance.h; grown, never shrunk)
    DeviceBuffer quantile_ws;    // a percentile request's whole plane as keys, u64[n][width] (sp_kernel_quantile.h; grown, never shrunk)
    DeviceBuffer burst_ws;       // a burst request's band series f64[count][width] and, behind it, its segments' summaries and carries (sp_kernel_burst.h; grown, never shrunk)
    DeviceBuffer pulse_ws;       // a burst-measurement request's cells u64[count][max_bursts][spx::kSlots], peak keys u64[count][max_bursts] and, behind them, count uint32 for a request without a counts array (sp_kernel_pulse.h; grown, never shrunk)
    DeviceBuffer lagcov_ws;      // a lagged-covariance request's band series f64[count][width] and, behind it, its cells u64[spv::kSlots][npairs * lags] and u64[npairs][66] (sp_kernel_lagcov.h; grown, never shrunk)
    DeviceBuffer plane_window;   // a mean, band-power or track request: the block of frames of its plane that is being consumed (plane_blocks)
    int32_t blockmean_direct_max = 0;   // sp_context_set_blockmean_direct_max: the largest group k_blockmean takes; 0 is the built default, SP_BLOCKMEAN_DIRECT_FRAMES
    int64_t blockmean_next = 0;         // a block-mean request: the frame its next run begins with (BlockMeanKind::consume)
    size_t mean_window_bytes = 0; // sp_context_set_mean_window: the window's size at the most; 0 is the default, kPlaneWindowDefault
    DeviceBuffer index_rgba;     // an indexed request's temporary RGBA image on the render_extract path (grown, never shrunk)
    DeviceBuffer density_index;  // sp_plan_execute_density: the request's index image, width * n bytes (grown, never shrunk)
    DeviceBuffer density_reply;  // ... and the reply record its render's side outputs go to (sphost::ReplyRecord)
    // staging for sp_render (host-buffer entry point)
    DeviceBuffer in_bytes, out_rgba, render_small;
    HostBuffer host_small;
    // sp_render's copy streams and events: the image goes back to the host chunk by chunk while later chunks still arrive
    hipStream_t copy_in = nullptr, copy_out = nullptr;
    hipEvent_t ev_arrived[spgeo::kMaxChunks] = {}, ev_rendered[spgeo::kMaxChunks] = {};
    sp_plan *cached_plan = nullptr;
    NamedRequest named;          // sp_render_named: what the cached plan was built from
    long long plans_created = 0; // sp_context_plan_creations: how many plans (table sets on the device) this context has built
    bool acc_dirty = false;      // a request failed between its launches: accumulators must be re-initialised
    size_t last_upload_bytes = 0; // what the last sp_render sent over the host link (a sparse request sends its frames only)
    int last_chunks = 0;          // ... and in how many chunks of frames the streamer carried that request out
    uint32_t seq = 0;            // requests started on this context (k_frames publishes the number once the reply is cleared; never 0)
    // sp_plan_execute_batch: the work list (item records, group -> item maps) on the device and its page-locked source, which is
    // rewritten only once the event says the previous batch's copy has read it
    DeviceBuffer batch_dev;
    HostBuffer batch_host;
    hipEvent_t ev_batch = nullptr;
    hipEvent_t ev_batch_done = nullptr;   // behind the last batch's launches: the next table copy waits for it (on whatever stream)
    // timing
    bool timing = false;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
};

// The kernels of a request.  The values are public: sp_plan_force_kernel and SP_FORCE_KERNEL take them.
enum Kernel {
    kKernelAuto = 0,         // (sp_plan_force_kernel: the library chooses)
    kKernelScratch = 1,      // k_scratch_radix2
    kKernelLdsR16 = 2,       // k_lds_r16, round 1's frame loop: removed in round 3
    kKernelFrames = 3,       // k_frames
    kKernelFramesPeak = 4,   // k_frames_peak
};
// a frame-loop kernel finishes the request itself (histograms, dBfs range, gauges); behind the scratch kernel a finish kernel is queued
static bool finishes_request(int kernel) { return kernel == kKernelFrames || kernel == kKernelFramesPeak; }

struct sp_plan {
    sp_context *ctx = nullptr;
    sp_request req{};               // windowc / lut_rgb pointers are NOT kept (copied below)
    std::vector<double> window;
    std::vector<uint8_t> lut;
    int levels = 0;
    spfmt::Format fmt{};
    double block_norm_db = 0;
    float gray_a = 0, gray_b = 0, cb_a = 0, cb_b = 0;
    bool edges_in_f32 = false;      // every colour / centi-bel edge lies in [2^-100, 2^100]: the f32 first guess is enough
    bool taper_finite = false;      // no +-inf / NaN in windowc: the (1, 0) butterflies may skip their products on integer samples
    bool tw16_ok = false;           // the first-pass twiddle literals of k_frames equal this plan's table entries
    sphost::Thresholds th{};        // f32 coefficients of both frame-loop kernels (edge vectors are released after the upload)
    DeviceBuffer tables;            // one allocation, carved below
    const double *d_window = nullptr, *d_cos = nullptr, *d_sin = nullptr, *d_gray_edge = nullptr, *d_cb_edge = nullptr;
    const uint32_t *d_lut = nullptr;
    const uint16_t *d_cell_g = nullptr, *d_cell_l = nullptr;   // merged-cell ranges per colour index / level (k_frames)
    const double2 *d_stage_tw = nullptr;   // per-stage twiddle tables for k_frames
    DeviceBuffer ident_lut;         // indexed requests on the render_extract path: the LUT whose entry i is (i, 0, 0), built on first use
    int force_kernel = kKernelAuto;
};

namespace {

int fail(sp_context *ctx, int code, const std::string &msg)
{
    if (ctx) ctx->error = msg;
    return code;
}

int hip_fail(sp_context *ctx, hipError_t e, const char *what)
{
    return fail(ctx, SP_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

#define SP_HIP(ctx, call)                                            \
    do {                                                             \
        hipError_t e_ = (call);                                      \
        if (e_ != hipSuccess) return hip_fail((ctx), e_, #call);     \
    } while (0)

int validate_request(sp_context *ctx, const sp_request *r)
{
    std::string why;
    const int rc = sphost::validate_request(r, why);
    return rc ? fail(ctx, rc, why) : SP_OK;
}

// The context's timing pair around what body() queues on the context's stream: ev0 in front of it and ev1 behind it where timing is
// on.  A body that fails leaves ev1 and `timed` as they were.
template <typename Body>
int timed(sp_context *ctx, Body &&body)
{
    if (ctx->timing) SP_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    const int rc = body();
    if (rc) return rc;
    if (ctx->timing) {
        SP_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
        ctx->timed = true;
    }
    return SP_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------------- host helpers

extern "C" int sp_version(void) { return SP_VERSION; }

extern "C" const char *sp_status_string(int status)
{
    switch (status) {
    case SP_OK: return "ok";
    case SP_ERR_INVALID_ARG: return "invalid argument";
    case SP_ERR_NOT_POW2: return "Length is not a power of 2";
    case SP_ERR_BYTE_LENGTH: return "byte length is not a multiple of the element size";
    case SP_ERR_UNSUPPORTED: return "unsupported by this library";
    case SP_ERR_NO_DEVICE: return "no HIP device";
    case SP_ERR_HIP: return "HIP runtime error";
    case SP_ERR_NOMEM: return "out of device memory";
    default: return "unknown status";
    }
}

extern "C" const char *sp_last_error(const sp_context *ctx) { return ctx ? ctx->error.c_str() : ""; }

extern "C" int sp_format_parse(const char *name, int32_t *format, int32_t *sample_width)
{
    const int32_t id = sphost::parse_format(name ? name : "");
    if (format) *format = id;
    if (sample_width) *sample_width = spfmt::describe(id).width;
    return SP_OK;
}

extern "C" int sp_format_element_size(int32_t format)
{
    if (format < 0 || format >= SP_FMT_COUNT) return SP_ERR_INVALID_ARG;
    return spfmt::describe(format).elem;
}

extern "C" int sp_slice_bounds(size_t nbytes, int32_t sample_width, int32_t index, int32_t count, size_t *begin, size_t *end)
{
    if (sample_width < 1 || count < 1 || index < 0 || index >= count || !begin || !end) return SP_ERR_INVALID_ARG;
    const size_t end_sample = nbytes / (size_t)sample_width;                     // ~~(byteLength / sampleWidth)
    const size_t slice_len = (size_t)sample_width * (end_sample / (size_t)count);  // sampleWidth * ~~(samples / count)
    *begin = slice_len * (size_t)index;
    *end = slice_len * ((size_t)index + 1);
    return SP_OK;
}

extern "C" int sp_window(const char *name, int32_t n, double *window, double *weight)
{
    if (!name || n < 1 || !window || !weight) return SP_ERR_INVALID_ARG;
    return sphost::window(name, n, window, weight) ? SP_OK : SP_ERR_INVALID_ARG;
}

extern "C" int sp_twiddles(int32_t n, double *cos_table, double *sin_table)
{
    if (n < 1 || sphost::log2_exact(n) < 0) return SP_ERR_NOT_POW2;
    if (!cos_table || !sin_table) return SP_ERR_INVALID_ARG;
    sphost::twiddles(n, cos_table, sin_table);
    return SP_OK;
}

extern "C" double sp_js_log10(double x) { return spjs::log10(x); }

extern "C" int sp_cmap_count(void) { return spcmap::kCount; }

extern "C" const char *sp_cmap_key(int32_t index) { return index >= 0 && index < spcmap::kCount ? spcmap::kEntries[index].key : ""; }

static int cmap_index(const char *name)
{
    const char *keys[spcmap::kCount];
    for (int i = 0; i < spcmap::kCount; i++) keys[i] = spcmap::kEntries[i].key;
    return sphost::lookup_key(keys, spcmap::kCount, name);
}

// entry `i` of the colour-map table as r, g, b bytes: the literal tables of the reference as tables, its computed maps
// (lib/soxcmap.js, lib/naivecmap.js) evaluated by their generators
static void cmap_bytes(int i, uint8_t *rgb)
{
    const spcmap::Entry &e = spcmap::kEntries[i];
    if (e.offset >= 0) memcpy(rgb, spcmap::kData + e.offset, 3 * (size_t)e.length);
    else if (!sphost::cmap_generate(e.key, e.length, rgb)) memset(rgb, 0, 3 * (size_t)e.length);   // (every offset -1 entry has a generator: test_abi_cpu)
}

extern "C" int sp_cmap(const char *name, uint8_t *rgb, int32_t capacity_entries, int32_t *lut_len)
{
    const int i = cmap_index(name);
    if (i < 0) return SP_ERR_UNSUPPORTED;
    const spcmap::Entry &e = spcmap::kEntries[i];
    if (lut_len) *lut_len = e.length;
    if (!rgb || capacity_entries < e.length) return SP_ERR_INVALID_ARG;
    cmap_bytes(i, rgb);
    return SP_OK;
}

extern "C" int sp_cmap_generate(const char *key, int32_t stops, uint8_t *rgb)
{
    if (!key || stops < 1 || stops > 65536 || !rgb) return SP_ERR_INVALID_ARG;
    return sphost::cmap_generate(key, stops, rgb) ? SP_OK : SP_ERR_UNSUPPORTED;
}

extern "C" int sp_host_alloc(size_t nbytes, void **ptr)
{
    if (!ptr) return SP_ERR_INVALID_ARG;
    *ptr = nullptr;
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess || c <= 0) return SP_ERR_NO_DEVICE;
    return hipHostMalloc(ptr, nbytes ? nbytes : 1, hipHostMallocDefault) == hipSuccess ? SP_OK : SP_ERR_NOMEM;
}

extern "C" void sp_host_free(void *ptr)
{
    if (ptr) (void)hipHostFree(ptr);
}

extern "C" int sp_host_register(void *ptr, size_t nbytes)
{
    if (!ptr || !nbytes) return SP_ERR_INVALID_ARG;
    return hipHostRegister(ptr, nbytes, hipHostRegisterDefault) == hipSuccess ? SP_OK : SP_ERR_HIP;
}

extern "C" void sp_host_unregister(void *ptr)
{
    if (ptr) (void)hipHostUnregister(ptr);
}

// ------------------------------------------------------------------------------------------------- contexts

extern "C" int sp_device_count(int32_t *count)
{
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) c = 0;
    if (count) *count = c;
    return c > 0 ? SP_OK : SP_ERR_NO_DEVICE;
}

extern "C" int sp_context_create(int32_t device, sp_context **out)
{
    if (!out) return SP_ERR_INVALID_ARG;
    *out = nullptr;
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess || c <= 0) return SP_ERR_NO_DEVICE;
    if (device < 0 || device >= c) return SP_ERR_INVALID_ARG;
    sp_context *ctx = new (std::nothrow) sp_context;
    if (!ctx) return SP_ERR_NOMEM;
    ctx->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking) != hipSuccess) {
        delete ctx;
        return SP_ERR_HIP;
    }
    ctx->stream = ctx->own_stream;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) ctx->cu_count = ctx->device_cu_count = prop.multiProcessorCount;
    (void)hipEventCreate(&ctx->ev0);
    (void)hipEventCreate(&ctx->ev1);
    *out = ctx;
    return SP_OK;
}

extern "C" void sp_context_destroy(sp_context *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->cached_plan) sp_plan_destroy(ctx->cached_plan);
    ctx->frame_minmax.release();
    ctx->partial.release();
    ctx->scratch.release();
    ctx->traces_ws.release();
    ctx->power_plane.release();
    ctx->mean_ws.release();
    ctx->variance_ws.release();
    ctx->quantile_ws.release();
    ctx->burst_ws.release();
    ctx->pulse_ws.release();
    ctx->lagcov_ws.release();
    ctx->plane_window.release();
    ctx->index_rgba.release();
    ctx->density_index.release();
    ctx->density_reply.release();
    ctx->in_bytes.release();
    ctx->out_rgba.release();
    ctx->render_small.release();
    ctx->host_small.release();
    if (ctx->ev_batch) (void)hipEventDestroy(ctx->ev_batch);
    if (ctx->ev_batch_done) (void)hipEventDestroy(ctx->ev_batch_done);
    ctx->batch_dev.release();
    ctx->batch_host.release();
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    for (int k = 0; k < spgeo::kMaxChunks; k++) {
        if (ctx->ev_arrived[k]) (void)hipEventDestroy(ctx->ev_arrived[k]);
        if (ctx->ev_rendered[k]) (void)hipEventDestroy(ctx->ev_rendered[k]);
    }
    if (ctx->copy_in) (void)hipStreamDestroy(ctx->copy_in);
    if (ctx->copy_out) (void)hipStreamDestroy(ctx->copy_out);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    delete ctx;
}

extern "C" int sp_context_set_stream(sp_context *ctx, void *hip_stream)
{
    if (!ctx) return SP_ERR_INVALID_ARG;
    ctx->stream = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
    return SP_OK;
}

extern "C" int sp_context_get_stream(const sp_context *ctx, void **hip_stream)
{
    if (!ctx || !hip_stream) return SP_ERR_INVALID_ARG;
    *hip_stream = ctx->stream == ctx->own_stream ? nullptr : (void *)ctx->stream;
    return SP_OK;
}

extern "C" int sp_context_synchronize(sp_context *ctx)
{
    if (!ctx) return SP_ERR_INVALID_ARG;
    SP_HIP(ctx, hipSetDevice(ctx->device));
    SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SP_OK;
}

extern "C" int sp_context_enable_timing(sp_context *ctx, int32_t on)
{
    if (!ctx) return SP_ERR_INVALID_ARG;
    ctx->timing = on != 0;
    ctx->timed = false;
    return SP_OK;
}

extern "C" int sp_context_last_kernel_ms(sp_context *ctx, float *ms)
{
    if (!ctx || !ms) return SP_ERR_INVALID_ARG;
    if (!ctx->timed) return fail(ctx, SP_ERR_INVALID_ARG, "no timed execute on this context");
    SP_HIP(ctx, hipEventSynchronize(ctx->ev1));
    SP_HIP(ctx, hipEventElapsedTime(ms, ctx->ev0, ctx->ev1));
    return SP_OK;
}

extern "C" int sp_context_event_pair_overhead_ms(sp_context *ctx, float *ms)
{
    if (!ctx || !ms) return SP_ERR_INVALID_ARG;
    SP_HIP(ctx, hipSetDevice(ctx->device));
    float best = 1e30f;
    for (int i = 0; i < 8; i++) {
        SP_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
        spk::launch_noop(ctx->stream);
        SP_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
        SP_HIP(ctx, hipEventSynchronize(ctx->ev1));
        float t = 0;
        SP_HIP(ctx, hipEventElapsedTime(&t, ctx->ev0, ctx->ev1));
        if (t < best) best = t;
    }
    ctx->timed = false;
    *ms = best;
    return SP_OK;
}

// ------------------------------------------------------------------------------------------------- device memory

extern "C" int sp_device_alloc(sp_context *ctx, size_t nbytes, void **d_ptr)
{
    if (!ctx || !d_ptr) return SP_ERR_INVALID_ARG;
    SP_HIP(ctx, hipSetDevice(ctx->device));
    if (hipMalloc(d_ptr, nbytes ? nbytes : 1) != hipSuccess) return fail(ctx, SP_ERR_NOMEM, "hipMalloc failed");
    return SP_OK;
}

extern "C" int sp_device_free(sp_context *ctx, void *d_ptr)
{
    if (!ctx) return SP_ERR_INVALID_ARG;
    SP_HIP(ctx, hipSetDevice(ctx->device));
    SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    SP_HIP(ctx, hipFree(d_ptr));
    return SP_OK;
}

extern "C" int sp_device_upload(sp_context *ctx, void *d_dst, const void *src, size_t nbytes)
{
    if (!ctx) return SP_ERR_INVALID_ARG;
    SP_HIP(ctx, hipSetDevice(ctx->device));
    SP_HIP(ctx, hipMemcpyAsync(d_dst, src, nbytes, hipMemcpyHostToDevice, ctx->stream));
    SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SP_OK;
}

extern "C" int sp_device_download(sp_context *ctx, void *dst, const void *d_src, size_t nbytes)
{
    if (!ctx) return SP_ERR_INVALID_ARG;
    SP_HIP(ctx, hipSetDevice(ctx->device));
    SP_HIP(ctx, hipMemcpyAsync(dst, d_src, nbytes, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SP_OK;
}

extern "C" int sp_device_memset(sp_context *ctx, void *d_ptr, int value, size_t nbytes)
{
    if (!ctx) return SP_ERR_INVALID_ARG;
    SP_HIP(ctx, hipSetDevice(ctx->device));
    SP_HIP(ctx, hipMemsetAsync(d_ptr, value, nbytes, ctx->stream));
    return SP_OK;
}

extern "C" int sp_synth_trinoise(sp_context *ctx, void *d_bytes, int32_t format, uint64_t t0, uint64_t count, uint32_t seed,
                                 uint32_t step, uint32_t gshift, double amp, double namp)
{
    if (!ctx || !d_bytes) return SP_ERR_INVALID_ARG;
    if (format < 0 || format >= SP_FMT_COUNT) return fail(ctx, SP_ERR_INVALID_ARG, "unknown format id");
    if (count == 0) return SP_OK;
    SP_HIP(ctx, hipSetDevice(ctx->device));
    const spk::SynthArgs a{(uint8_t *)d_bytes, t0, count, seed, step, gshift, amp, namp};
    const int rc = spk::launch_synth_trinoise(a, format, ctx->stream);
    if (rc) return rc == SP_ERR_UNSUPPORTED ? fail(ctx, rc, "synth: too many samples for one launch") : rc;
    SP_HIP(ctx, hipGetLastError());
    return SP_OK;
}

// ------------------------------------------------------------------------------------------------- plans

extern "C" int sp_plan_create(sp_context *ctx, const sp_request *req, sp_plan **out)
{
    if (!ctx || !out) return SP_ERR_INVALID_ARG;
    *out = nullptr;
    int rc = validate_request(ctx, req);
    if (rc) return rc;
    SP_HIP(ctx, hipSetDevice(ctx->device));

    sp_plan *p = new (std::nothrow) sp_plan;
    if (!p) return fail(ctx, SP_ERR_NOMEM, "out of host memory");
    p->ctx = ctx;
    p->req = *req;
    p->window.assign(req->windowc, req->windowc + req->n);
    p->lut.assign(req->lut_rgb, req->lut_rgb + 3 * (size_t)req->lut_len);
    p->req.windowc = nullptr;
    p->req.lut_rgb = nullptr;
    p->levels = sphost::log2_exact(req->n);
    p->fmt = spfmt::describe(req->format);

    const int n = req->n, half = n / 2, L = req->lut_len;
    std::vector<double> ct((size_t)half), st((size_t)half);
    sphost::twiddles(n, ct.data(), st.data());
    const sphost::PixelMath pm(req->block_norm, req->gain, req->range, L);
    const sphost::Thresholds th = sphost::build_thresholds(pm, L);
    p->block_norm_db = pm.block_norm_db;
    p->gray_a = th.gray_a;
    p->gray_b = th.gray_b;
    p->cb_a = th.cb_a;
    p->cb_b = th.cb_b;
    p->edges_in_f32 = true;
    for (int g = 1; g < L; g++) p->edges_in_f32 &= th.gray_edge[(size_t)g] >= 0x1p-100 && th.gray_edge[(size_t)g] <= 0x1p100;
    for (int j = 1; j <= SP_CB_HIST_SIZE; j++) p->edges_in_f32 &= th.cb_edge[(size_t)j] >= 0x1p-100 && th.cb_edge[(size_t)j] <= 0x1p100;
    p->taper_finite = true;
    for (int i = 0; i < n; i++) p->taper_finite &= std::isfinite(p->window[(size_t)i]);
    p->tw16_ok = n >= 16;
    for (int k = 0; k < 8 && p->tw16_ok; k++)
        p->tw16_ok = ct[(size_t)k * (size_t)(n / 16)] == spk2::kTw16Host[k].c && st[(size_t)k * (size_t)(n / 16)] == spk2::kTw16Host[k].s;
    p->th = th;
    p->th.gray_edge.clear();
    p->th.cb_edge.clear();
    p->th.cell_g.clear();
    p->th.cell_l.clear();
    std::vector<uint32_t> lut32((size_t)L);
    for (int i = 0; i < L; i++)
        lut32[(size_t)i] = (uint32_t)p->lut[3 * (size_t)i] | ((uint32_t)p->lut[3 * (size_t)i + 1] << 8)
                           | ((uint32_t)p->lut[3 * (size_t)i + 2] << 16) | 0xff000000u;
    // per-stage twiddle tables for k_frames: stage s (size 2^s) has 2^(s-1) entries (cos, sin), consecutive
    std::vector<double2> stage_tw;
    if (spk::frame_parts_support(n)) {
        stage_tw.resize((size_t)n);   // entries 1 .. n-1 used: stage s starts at 2^(s-1)
        stage_tw[0] = make_double2(0, 0);
        for (int s = 1; s <= p->levels; s++) {
            const int cnt = 1 << (s - 1);
            for (int m = 0; m < cnt; m++) {
                const int k = m << (p->levels - s);
                stage_tw[(size_t)(cnt + m)] = make_double2(ct[(size_t)k], st[(size_t)k]);
            }
        }
    }

    // one device allocation: [window n][cos half][sin half][gray_edge L][cb_edge 1001][stage_tw 2n doubles][lut L u32]
    const size_t nd = (size_t)n + 2 * (size_t)half + (size_t)L + (SP_CB_HIST_SIZE + 1) + 2 * stage_tw.size();
    const size_t cell_u16 = th.cell_g.size() + th.cell_l.size();
    const size_t bytes = nd * sizeof(double) + (((size_t)L * sizeof(uint32_t) + 7) & ~(size_t)7) + cell_u16 * sizeof(uint16_t);
    rc = p->tables.reserve(bytes);
    if (rc) {
        delete p;
        return fail(ctx, rc, "plan tables: out of device memory");
    }
    std::vector<uint8_t> host(bytes);
    double *h = (double *)host.data();
    double *d = (double *)p->tables.p;
    size_t o = 0;
    auto put = [&](const void *src, size_t count) {
        if (count) memcpy(h + o, src, count * sizeof(double));
        const double *dev = d + o;
        o += count;
        return dev;
    };
    p->d_window = put(p->window.data(), (size_t)n);
    p->d_cos = put(ct.data(), (size_t)half);
    p->d_sin = put(st.data(), (size_t)half);
    p->d_gray_edge = put(th.gray_edge.data(), (size_t)L);
    p->d_cb_edge = put(th.cb_edge.data(), SP_CB_HIST_SIZE + 1);
    p->d_stage_tw = (const double2 *)put(stage_tw.data(), 2 * stage_tw.size());
    memcpy(h + o, lut32.data(), (size_t)L * sizeof(uint32_t));
    p->d_lut = (const uint32_t *)(d + o);
    {
        const size_t off = o * sizeof(double) + (((size_t)L * sizeof(uint32_t) + 7) & ~(size_t)7);
        memcpy(host.data() + off, th.cell_g.data(), th.cell_g.size() * sizeof(uint16_t));
        memcpy(host.data() + off + th.cell_g.size() * sizeof(uint16_t), th.cell_l.data(), th.cell_l.size() * sizeof(uint16_t));
        p->d_cell_g = (const uint16_t *)((const char *)p->tables.p + off);
        p->d_cell_l = p->d_cell_g + th.cell_g.size();
    }
    hipError_t e = hipMemcpyAsync(p->tables.p, host.data(), bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        p->tables.release();
        delete p;
        return hip_fail(ctx, e, "plan table upload");
    }
    ctx->plans_created++;
    *out = p;
    return SP_OK;
}

extern "C" int sp_context_plan_creations(const sp_context *ctx, int64_t *count)
{
    if (!ctx || !count) return SP_ERR_INVALID_ARG;
    *count = (int64_t)ctx->plans_created;
    return SP_OK;
}

extern "C" void sp_plan_destroy(sp_plan *plan)
{
    if (!plan) return;
    if (plan->ctx) {
        (void)hipSetDevice(plan->ctx->device);
        (void)hipStreamSynchronize(plan->ctx->stream);
        if (plan->ctx->cached_plan == plan) plan->ctx->cached_plan = nullptr;
    }
    plan->tables.release();
    plan->ident_lut.release();
    delete plan;
}

// k_frames skips the products of (1, 0) butterflies on integer samples, which is exact only with a finite taper; it takes its
// indices from an f32 scale, which needs every edge inside the f32 range and usable margins (sp_host.cpp); its first-pass twiddles
// are literals, checked against this plan's table.
static bool plan_frames_capable(const sp_plan *plan)
{
    return spk2::frames_kernel_supports(plan->req.n) && plan->req.lut_len >= 2 && plan->req.lut_len <= spk::kLdsMaxLut
           && plan->gray_b <= spk::kLdsMaxGrayB && plan->edges_in_f32 && plan->taper_finite && plan->th.frames_ok && plan->tw16_ok;
}

static int plan_kernel(const sp_plan *plan)
{
    if (plan->force_kernel) return plan->force_kernel;
#ifdef SP_EXPERIMENT_KNOBS
    static const int env_kernel = getenv("SP_FORCE_KERNEL") ? atoi(getenv("SP_FORCE_KERNEL")) : 0;
    if (env_kernel == kKernelFrames && plan_frames_capable(plan)) return kKernelFrames;
    if (env_kernel == kKernelScratch) return kKernelScratch;
#endif
    // k_frames is the fast path; the scratch kernel covers every request it does not
    return plan_frames_capable(plan) ? kKernelFrames : kKernelScratch;
}

// The kernel of one request of a plan: plan_kernel's, or for a peak plan's request with M >= 2 sub-frames per column k_frames_peak
// where it covers the plan, else the scratch kernel (it holds the peak too).  M == 1 is the sample detector: the same kernels.
static int request_kernel(const sp_plan *plan, int32_t peak_m)
{
    const int k = plan_kernel(plan);
    if (plan->req.detector != SP_DETECTOR_PEAK || peak_m < 2) return k;
    return k == kKernelFrames && spk2::frames_peak_supports(plan->req.n) ? kKernelFramesPeak : kKernelScratch;
}

extern "C" int sp_plan_force_kernel(sp_plan *plan, int32_t which)
{
    if (!plan || which < kKernelAuto || which > kKernelFrames) return SP_ERR_INVALID_ARG;
    if (which == kKernelLdsR16) return fail(plan->ctx, SP_ERR_UNSUPPORTED, "k_lds_r16 is no longer part of the library");
    if (which == kKernelFrames && !plan_frames_capable(plan)) return fail(plan->ctx, SP_ERR_UNSUPPORTED, "k_frames does not cover this request");
    plan->force_kernel = which;
    return SP_OK;
}

static const char *kernel_name(int kernel)
{
    return kernel == kKernelFramesPeak ? "frames_peak" : kernel == kKernelFrames ? "frames" : "scratch_radix2";
}

extern "C" const char *sp_plan_kernel_name(const sp_plan *plan) { return plan ? kernel_name(request_kernel(plan, 2)) : ""; }

extern "C" const char *sp_plan_kernel_name_for(const sp_plan *plan, size_t nbytes, int32_t width)
{
    return plan ? kernel_name(request_kernel(plan, spgeo::peak_shape(spgeo::geometry(plan->fmt, plan->req.n, nbytes, width)).m)) : "";
}

// The frame loop over frames [x_begin, x_end) of a width-frame image.  `first` prepares the context's workspace and accumulators,
// `last` ends the request: k_frames then produces histograms and dBfs range itself (its last workgroup; the gauges it writes group by
// group in every launch), behind the scratch kernel a finish kernel is queued.  sp_plan_execute is the whole range in one launch - ONE
// kernel for every request k_frames covers; sp_render walks the image in chunks so that the copies to and from the host overlap.
// `shape`: the request's geometry and peak shape, computed once per request from its own nbytes and width (request_shape).
// `src` (sp_render's packed upload, below): the frames [x_begin, x_end) do not lie in the capture at d_bytes but in a packed copy of it;
// the kernel is handed that copy's address, length and stride instead (every frame inside it), everything else - image geometry, frame
// numbers, peak shape, kernel choice, reply - stays the request's.
struct PackedSource {
    const void *bytes;     // address of (virtual) sample 0 of the packed layout
    size_t nbytes;         // its (virtual) length
    double stride;         // frame x starts at sample ~~(0.5 + stride * x) of it
};

// The kernel arguments a plan fixes: sizes, layout, the device tables and the epilogue's constants.
static void plan_frame_args(const sp_plan *plan, spk::FrameArgs &a)
{
    a.n = plan->req.n;
    a.levels = plan->levels;
    a.channel_mode = plan->req.channel_mode ? 1 : 0;
    a.waterfall = plan->req.waterfall ? 1 : 0;
    a.lut_len = plan->req.lut_len;
    a.sample_width = plan->fmt.width;
    a.window = plan->d_window;
    a.cos_t = plan->d_cos;
    a.sin_t = plan->d_sin;
    a.gray_edge = plan->d_gray_edge;
    a.cb_edge = plan->d_cb_edge;
    a.lut_rgba = plan->d_lut;
    a.gray_a = plan->gray_a;
    a.gray_b = plan->gray_b;
    a.cb_a = plan->cb_a;
    a.cb_b = plan->cb_b;
    a.g2_a = plan->th.g2_a;
    a.g2_b = plan->th.g2_b;
    a.g2_thr = plan->th.g2_thr;
    a.g2_m = plan->th.g2_m;
    a.c2_a = plan->th.c2_a;
    a.c2_b = plan->th.c2_b;
    a.c2_thr = plan->th.c2_thr;
    a.c2_m = plan->th.c2_m;
    a.c2_lo = plan->th.c2_lo;
    a.c2_hi = plan->th.c2_hi;
    a.block_norm_db = plan->block_norm_db;
    a.gain = plan->req.gain;
    a.range = plan->req.range;
    a.cell_g = plan->d_cell_g;
    a.cell_l = plan->d_cell_l;
    a.cells = plan->th.cells;
}

struct RequestShape {
    spgeo::Geometry g;
    spgeo::PeakShape peak;   // the peak detector's sub-frames per column (m = 1: the request is the sample detector's, kernels included)
};

static RequestShape request_shape(const sp_plan *plan, size_t nbytes, int32_t width)
{
    const spgeo::Geometry g = spgeo::geometry(plan->fmt, plan->req.n, nbytes, width);
    return {g, plan->req.detector == SP_DETECTOR_PEAK ? spgeo::peak_shape(g) : spgeo::PeakShape{}};
}

// The limits of one capture and its image.  `reply`: device pointers the kernels add to with 64-bit atomics (null: none to check);
// `who`: "" for a request, "batch item: " for an item of a batch.
static int check_capture(sp_context *ctx, const spfmt::Format &f, int n, const void *bytes, size_t nbytes, int32_t width, const sp_reply *reply,
                         const std::string &who)
{
    const bool item = !who.empty();
    if (width < 0) return fail(ctx, SP_ERR_INVALID_ARG, who + "width < 0");
    if (nbytes && !bytes) return fail(ctx, SP_ERR_INVALID_ARG, who + (item ? "bytes is null" : "d_bytes is null"));
    if (nbytes % (size_t)f.elem) return fail(ctx, SP_ERR_BYTE_LENGTH, who + "byte length is not a multiple of the element size");
    if ((double)nbytes / (double)f.width >= 2147483648.0 - (double)n)                 // samples.js:167
        return fail(ctx, SP_ERR_UNSUPPORTED, who + "captures of 2^31 samples or more must be sliced (sample positions are int32)");
    if ((double)width * (double)n > 4e12) return fail(ctx, SP_ERR_UNSUPPORTED, who + "image too large");
    if (reply && (((uintptr_t)reply->c_hist | (uintptr_t)reply->cb_hist | (uintptr_t)reply->dbfs_minmax) & 7) != 0)
        return fail(ctx, SP_ERR_INVALID_ARG, (item ? who : "reply: ") + "c_hist, cb_hist and dbfs_minmax must be 8-byte aligned");
    return SP_OK;
}

// The request's number travels in the kernel arguments, and the frame loop's workgroups wait for workgroup 0 to publish it (the reply is
// cleared first): a captured launch replayed from a hipGraph would find the number already there.  Refused.
static int refuse_capture(sp_context *ctx, hipStream_t s, const char *entry, const char *why)
{
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone)
        return fail(ctx, SP_ERR_UNSUPPORTED, std::string(entry) + " cannot be captured into a hipGraph" + why);
    (void)hipGetLastError();
    return SP_OK;
}

// What an entry point on device operands does before it allocates or queues anything: the capture's limits (`reply` as for
// check_capture), the context's device made current, a stream under graph capture refused in the name of `entry`.
static int device_operands(sp_context *ctx, const spfmt::Format &f, int n, const void *d_bytes, size_t nbytes, int32_t width, const sp_reply *reply,
                           const char *entry)
{
    const int rc = check_capture(ctx, f, n, d_bytes, nbytes, width, reply, "");
    if (rc) return rc;
    SP_HIP(ctx, hipSetDevice(ctx->device));
    return refuse_capture(ctx, ctx->stream, entry, " (every launch carries its request's number)");
}

// the write-out may store an image in 16-byte pieces with 32-bit offsets
static bool rgba_fast(const uint8_t *rgba, int32_t width, int n)
{
    return rgba && ((uintptr_t)rgba & 15) == 0 && (width & 3) == 0 && width < (1 << 24) && (double)width * (double)n * 4.0 <= 4294967296.0;
}

// Where the frames [x_begin, x_end) lie, as the kernel reads them: in the capture at d_bytes with the request's stride, or in `src`, a
// packed copy of this range's frames with its own address, length and stride (every frame inside it).
static void frame_source_args(spk::FrameArgs &a, const sp_plan *plan, const void *d_bytes, const spgeo::Geometry &g, int32_t x_begin,
                              int32_t x_end, const PackedSource *src)
{
    const size_t nbytes = src ? src->nbytes : g.nbytes;
    a.bytes = (const uint8_t *)(src ? src->bytes : d_bytes);
    a.nbytes = (int64_t)nbytes;
    a.nelem = (int64_t)(nbytes / (size_t)plan->fmt.elem);
    a.stride = src ? src->stride : g.stride;
    a.width = g.width;
    a.in_bounds = src || g.in_bounds ? 1 : 0;
    a.frame0 = x_begin;
    a.x_end = x_end;
}

// Workgroups of a scratch-kernel launch: each owns `slabs_per_group` slabs of n doubles, all of them capped at 256 MiB; no more
// workgroups than frames or than four per CU.
static long long scratch_blocks(int slabs_per_group, int n, int32_t frames, int cu_count)
{
    long long blocks = (256ll << 20) / (8ll * slabs_per_group * n);
    if (blocks > frames) blocks = frames;
    if (blocks > 4 * cu_count) blocks = 4 * cu_count;
    return blocks < 1 ? 1 : blocks;
}

// What a scratch-kernel launch over `frames` frames needs: its workgroups (*blocks), their `slabs` slabs each in the context's scratch
// buffer (a.scratch).
static int scratch_reserve(sp_context *ctx, spk::FrameArgs &a, int slabs, int32_t frames, unsigned *blocks)
{
    *blocks = (unsigned)scratch_blocks(slabs, a.n, frames, ctx->cu_count);
    const int rc = ctx->scratch.reserve((size_t)*blocks * (size_t)slabs * (size_t)a.n * sizeof(double));
    if (rc) return fail(ctx, rc, "scratch: out of device memory");
    a.scratch = (double *)ctx->scratch.p;
    return SP_OK;
}

// ------------------------------------------------------------------------------------------------- indexed images: the render_extract path

// k_frames_index may store the index image in 16-byte pieces with 32-bit offsets: base, width, the launch's first frame and its end are
// multiples of 16 (every row piece of 16 frames then lies aligned and is whole or absent), the image is below 4 GiB
static bool index_fast(const uint8_t *index, int32_t width, int n, int32_t x_begin, int32_t x_end)
{
    return index && ((uintptr_t)index & 15) == 0 && (width & 15) == 0 && ((x_begin | x_end) & 15) == 0 && width < (1 << 24)
           && (double)width * (double)n <= 4294967296.0;
}

// frames [x_begin, x_end) of the temporary RGBA image -> the same frames of the index image (both `width` frames wide)
static int extract_index_band(sp_context *ctx, const uint8_t *d_rgba, uint8_t *d_index, int32_t width, int n, bool waterfall, int32_t x_begin,
                              int32_t x_end)
{
    const size_t W = (size_t)width, N = (size_t)n, band = (size_t)(x_end - x_begin);
    // waterfall: rows width - x_end .. width - 1 - x_begin, contiguous; spectrogram: columns x_begin .. x_end - 1 of every row
    const size_t first = waterfall ? N * (W - (size_t)x_end) : (size_t)x_begin;
    const size_t row_px = waterfall ? N * band : band, rows = waterfall ? 1 : N, pitch = waterfall ? N * band : W;
    const int rc = spk::launch_extract_index(d_rgba + 4 * first, d_index + first, row_px, rows, pitch, ctx->stream);
    if (rc) return fail(ctx, rc, "image too large for one extraction launch");
    SP_HIP(ctx, hipGetLastError());
    return SP_OK;
}

// frames [x_begin, x_end) of the index image at d_index ADDED to d_density, on the context's stream
static int density_count(sp_context *ctx, const uint8_t *d_index, int n, int32_t width, bool waterfall, int lut_len, int32_t x_begin,
                         int32_t x_end, uint32_t *d_density)
{
    if (x_end <= x_begin) return SP_OK;
    const int rc = spk::launch_density_count(d_index, n, width, waterfall, x_begin, x_end, lut_len, d_density, ctx->stream);
    if (rc) return fail(ctx, rc, "image too large for one counting launch");
    SP_HIP(ctx, hipGetLastError());
    return SP_OK;
}

// Where a request's picture goes.  kRgba: the request's kernel writes the RGBA image.  kIndexFrames: k_frames_index writes the index
// image.  kIndexExtract: the request's ordinary kernel renders through the plan's identity LUT into the context's temporary RGBA image
// and k_extract_index keeps byte 0 of every pixel of the range (the caller has run index_prepare).
struct Picture {
    enum Kind { kRgba, kIndexFrames, kIndexExtract } kind;
    uint8_t *image;   // device memory: RGBA [4 * width * n] or index [width * n]; may be null: side outputs only
};

// an indexed request's picture (`frames`: index_frames' answer for the request); without an image nothing is there to extract
static Picture index_picture(uint8_t *d_index, bool frames)
{
    return Picture{frames ? Picture::kIndexFrames : d_index ? Picture::kIndexExtract : Picture::kRgba, d_index};
}

static int plan_execute_range(sp_plan *plan, const void *d_bytes, const RequestShape &shape, int32_t x_begin, int32_t x_end, bool first,
                              bool last, const sp_reply *out, const Picture &pic, const PackedSource *src = nullptr)
{
    if (!plan || !out) return SP_ERR_INVALID_ARG;
    sp_context *ctx = plan->ctx;
    const spgeo::Geometry &g = shape.g;
    const spgeo::PeakShape &peak = shape.peak;
    const int n = plan->req.n;
    const int32_t width = g.width;
    int rc = device_operands(ctx, plan->fmt, n, d_bytes, g.nbytes, width, out, "sp_plan_execute");
    if (rc) return rc;
    hipStream_t s = ctx->stream;

    if (width == 0) {
        // nothing to draw; the reply keeps the loop's initial values (worker.js:35-36)
        if (out->c_hist) SP_HIP(ctx, hipMemsetAsync(out->c_hist, 0, (size_t)plan->req.lut_len * sizeof(uint64_t), s));
        if (out->cb_hist) SP_HIP(ctx, hipMemsetAsync(out->cb_hist, 0, SP_CB_HIST_SIZE * sizeof(uint64_t), s));
        if (out->dbfs_minmax) {
            static const double init[2] = {0.0, -200.0};
            SP_HIP(ctx, hipMemcpyAsync(out->dbfs_minmax, init, sizeof init, hipMemcpyHostToDevice, s));
            SP_HIP(ctx, hipStreamSynchronize(s));
        }
        return SP_OK;
    }

    const int which = request_kernel(plan, peak.m);
    if (src && which != kKernelFrames) return fail(ctx, SP_ERR_INVALID_ARG, "a packed source is for the frame-loop kernel only");
    rc = finishes_request(which) ? SP_OK : ctx->frame_minmax.reserve(2 * (size_t)width * sizeof(double));
    if (rc) return fail(ctx, rc, "workspace: out of device memory");
    // [0,4) k_frames: the number of the last request whose reply workgroup 0 has cleared; scratch kernel: [16,32) bit patterns of the
    // extreme |X|^2 of a request, [64, ...) colour and centi-bel histogram accumulators, back at their initial values when a request ends
    const size_t acc_bytes = 64 + (SP_MAX_LUT + SP_CB_HIST_SIZE) * sizeof(unsigned long long);
    const bool fresh_partial = ctx->partial.cap < acc_bytes;
    rc = ctx->partial.reserve(acc_bytes);
    if (rc) return fail(ctx, rc, "workspace: out of device memory");
    if (first && (fresh_partial || ctx->acc_dirty)) {
        static const unsigned long long mm_init[2] = {0x7ff0000000000000ull, 0ull};           // +inf, 0
        SP_HIP(ctx, hipMemsetAsync(ctx->partial.p, 0, ctx->partial.cap, s));
        SP_HIP(ctx, hipMemcpyAsync((char *)ctx->partial.p + 16, mm_init, sizeof mm_init, hipMemcpyHostToDevice, s));
        SP_HIP(ctx, hipStreamSynchronize(s));
    }
    ctx->acc_dirty = true;   // until this request's last launch (k_frames) or its finish kernel (scratch path) has been queued

    spk::FrameArgs a{};
    plan_frame_args(plan, a);
    frame_source_args(a, plan, d_bytes, g, x_begin, x_end, src);
    a.frame_min = (double *)ctx->frame_minmax.p;
    a.frame_max = a.frame_min + width;
    a.scratch = nullptr;
    if (first && ++ctx->seq == 0) ctx->seq = 1;
    a.first = first ? 1 : 0;
    a.seq = ctx->seq;
    a.flag = (unsigned int *)ctx->partial.p;
    a.gauge_mins = out->gauge_mins;
    a.gauge_maxs = out->gauge_maxs;
    a.gauge_amps = out->gauge_amps;
    a.out_c = (unsigned long long *)out->c_hist;
    a.out_cb = (unsigned long long *)out->cb_hist;
    a.out_minmax = out->dbfs_minmax;

    // the kernels count into the context's accumulators; the finish kernel moves the counts to the reply
    a.mm_acc = (unsigned long long *)((char *)ctx->partial.p + 16);
    a.c_hist = (unsigned long long *)((char *)ctx->partial.p + 64);
    a.cb_hist = a.c_hist + SP_MAX_LUT;
    const bool extract = pic.kind == Picture::kIndexExtract;
    a.rgba = extract ? (uint8_t *)ctx->index_rgba.p : pic.image;   // (reserved and the LUT built by the caller: index_prepare)
    a.rgba_fast = pic.kind == Picture::kIndexFrames ? index_fast(a.rgba, width, n, x_begin, x_end) : rgba_fast(a.rgba, width, n);
    if (extract) a.lut_rgba = (const uint32_t *)plan->ident_lut.p;

    const int32_t peak_nsamp = (int32_t)(peak.nsamp < 2147483647 ? peak.nsamp : 2147483647);
    rc = timed(ctx, [&]() -> int {
        int r = SP_OK;
        if (pic.kind == Picture::kIndexFrames) {
            if (which != kKernelFrames) return fail(ctx, SP_ERR_INVALID_ARG, "k_frames_index renders what k_frames renders");
            r = spk2::launch_frames_index(a, plan->req.format, plan->d_stage_tw, ctx->cu_count, ctx->device, s);
            if (r) return fail(ctx, r, "k_frames_index launch rejected the configuration");
        } else if (which == kKernelFrames) {
            r = spk2::launch_frames(a, plan->req.format, plan->d_stage_tw, ctx->cu_count, ctx->device, s);
            if (r) return fail(ctx, r, "k_frames launch rejected the configuration");
        } else if (which == kKernelFramesPeak) {
            r = spk2::launch_frames_peak(a, plan->req.format, plan->d_stage_tw, peak.m, peak_nsamp, ctx->cu_count, ctx->device, s);
            if (r) return fail(ctx, r, "k_frames_peak launch rejected the configuration");
        } else {
            // two slabs per workgroup (re, im), and for a held peak a third: the largest |X|^2 per bin over the column's sub-frames
            const bool hold = peak.m >= 2;
            unsigned blocks;
            r = scratch_reserve(ctx, a, hold ? 3 : 2, x_end - x_begin, &blocks);
            if (r) return r;
            r = spk::launch_scratch_radix2(a, plan->req.format, blocks, hold, peak.m, peak_nsamp, s);
            if (r) return fail(ctx, r, "bad format");
        }
        SP_HIP(ctx, hipGetLastError());
        if (extract && x_end > x_begin) return extract_index_band(ctx, a.rgba, pic.image, width, n, plan->req.waterfall != 0, x_begin, x_end);
        return SP_OK;
    });
    if (rc) return rc;

    if (!last) return SP_OK;
    if (finishes_request(which)) {   // k_frames / k_frames_peak has finished the request itself
        ctx->acc_dirty = false;
        return SP_OK;
    }

    spk::FinishArgs fa{};
    fa.bytes = a.bytes;
    fa.nbytes = a.nbytes;
    fa.nelem = a.nelem;
    fa.stride = a.stride;
    fa.n = n;
    fa.width = width;
    fa.format = plan->req.format;
    fa.block_norm_db = plan->block_norm_db;
    fa.gain = plan->req.gain;
    fa.range = plan->req.range;
    fa.frame_min = a.frame_min;
    fa.frame_max = a.frame_max;
    fa.gauge_mins = out->gauge_mins;
    fa.gauge_maxs = out->gauge_maxs;
    fa.gauge_amps = out->gauge_amps;
    fa.mm_acc = a.mm_acc;
    fa.out_minmax = out->dbfs_minmax;
    fa.lut_len = plan->req.lut_len;
    fa.acc_c = a.c_hist;
    fa.acc_cb = a.cb_hist;
    fa.out_c = (unsigned long long *)out->c_hist;
    fa.out_cb = (unsigned long long *)out->cb_hist;
    spk::launch_finish_frames(fa, s);
    SP_HIP(ctx, hipGetLastError());
    ctx->acc_dirty = false;
    return SP_OK;
}

extern "C" int sp_plan_execute(sp_plan *plan, const void *d_bytes, size_t nbytes, int32_t width, const sp_reply *out)
{
    if (!plan || !out) return SP_ERR_INVALID_ARG;
    return plan_execute_range(plan, d_bytes, request_shape(plan, nbytes, width), 0, width < 0 ? 0 : width, true, true, out,
                              Picture{Picture::kRgba, out->rgba});
}

// (tests) What sp_plan_execute would launch for a request of this shape on this plan's context, from the launch path's own functions:
// request_shape and request_kernel as plan_execute_range calls them, frames_prefetch_width and frames_launch_rule as launch_frames /
// launch_frames_peak call them, rgba_fast on the reply's image pointer.  Nothing is launched and nothing on the device is touched.
extern "C" int sp_plan_debug_launch(const sp_plan *plan, size_t nbytes, int32_t width, const void *rgba, int64_t *out, size_t capacity,
                                    size_t *used)
{
    if (!plan || !plan->ctx || width < 0 || !used) return SP_ERR_INVALID_ARG;
    const RequestShape shape = request_shape(plan, nbytes, width);
    const spgeo::Geometry &g = shape.g;
    const int n = plan->req.n, cu_count = plan->ctx->cu_count;
    const int which = width == 0 ? kKernelAuto : request_kernel(plan, shape.peak.m);   // (width 0: the reply is only cleared)
    spk2::FramesLaunch fl{0, 0, 0, 0};
    int prefetch = 0;
    if (finishes_request(which)) {
        prefetch = spk2::frames_prefetch_width(plan->fmt.width, g.in_bounds, g.stride, g.width);
        if (spk2::frames_launch_rule(n, plan->req.lut_len, width, cu_count, 0, fl)) return SP_ERR_UNSUPPORTED;
    }
    const int64_t v[] = {which, plan->levels, plan->req.channel_mode ? 1 : 0, prefetch, fl.gf, fl.groups, fl.grid, fl.lds_bytes,
                         rgba_fast((const uint8_t *)rgba, width, n) ? 1 : 0, shape.peak.m, cu_count};
    *used = sizeof v / sizeof v[0];
    if (*used > capacity || !out) return SP_ERR_INVALID_ARG;
    memcpy(out, v, sizeof v);
    return SP_OK;
}

// (tests) The CU count the context's launches are shaped by: 1 ... the device's own, 0 puts the device's own back.  Never more than the
// part has: the frame loop's bounded wait for workgroup 0 was reasoned for grids that are resident at once.  Plans read ctx->cu_count
// when they launch, so the next call on the context sees it.
extern "C" int sp_context_debug_set_cu_count(sp_context *ctx, int32_t cu_count)
{
    if (!ctx || cu_count < 0 || cu_count > ctx->device_cu_count) return SP_ERR_INVALID_ARG;
    ctx->cu_count = cu_count ? cu_count : ctx->device_cu_count;
    return SP_OK;
}

// (tests) The launch rule alone, without a plan or a device: frames_launch_rule's answer for `count` frames (gf_fixed = 0) or `count`
// groups of gf_fixed frames (a batch launch) on a part with cu_count CUs.
extern "C" int sp_debug_frames_launch(int32_t n, int32_t lut_len, int64_t count, int32_t cu_count, int32_t gf_fixed, int64_t *out,
                                      size_t capacity, size_t *used)
{
    if (n < 2 || sphost::log2_exact(n) < 0 || count < 1 || count > 2147483647 || cu_count < 1 || gf_fixed < 0 || !used) return SP_ERR_INVALID_ARG;
    spk2::FramesLaunch fl{0, 0, 0, 0};
    const int rc = spk2::frames_launch_rule(n, lut_len, count, cu_count, gf_fixed, fl);
    if (rc) return rc;
    const int64_t v[] = {fl.gf, fl.groups, fl.grid, fl.lds_bytes};
    *used = sizeof v / sizeof v[0];
    if (*used > capacity || !out) return SP_ERR_INVALID_ARG;
    memcpy(out, v, sizeof v);
    return SP_OK;
}

// (tests) The launch shape of the scratch kernels alone, without a plan or a device: scratch_blocks' answer for a launch over `frames`
// frames whose workgroups own `slabs` slabs of n doubles each on a part with cu_count CUs, and spk::scratch_wide's, as dispatch_scratch
// asks it.
extern "C" int sp_debug_scratch_launch(int32_t n, int32_t slabs, int32_t frames, int32_t cu_count, int64_t *out, size_t capacity, size_t *used)
{
    if (n < 2 || n > SP_MAX_N || sphost::log2_exact(n) < 0 || slabs < 1 || frames < 1 || cu_count < 1 || !used) return SP_ERR_INVALID_ARG;
    const int64_t v[] = {scratch_blocks(slabs, n, frames, cu_count), spk::scratch_wide(n) ? 1 : 0};
    *used = sizeof v / sizeof v[0];
    if (*used > capacity || !out) return SP_ERR_INVALID_ARG;
    memcpy(out, v, sizeof v);
    return SP_OK;
}

// ------------------------------------------------------------------------------------------------- merge of slice replies

extern "C" int sp_merge_replies(sp_context *ctx, const void *d_records, int32_t count, int32_t lut_len, uint64_t *d_c_hist,
                                uint64_t *d_cb_hist, double *d_dbfs_minmax)
{
    if (!ctx || !d_records || count < 1 || lut_len < 1 || lut_len > SP_MAX_LUT) return SP_ERR_INVALID_ARG;
    SP_HIP(ctx, hipSetDevice(ctx->device));
    spk::launch_merge_replies((const unsigned long long *)d_records, count, lut_len, sphost::ReplyRecord{(size_t)lut_len, 0}.words(), 1,
                              (unsigned long long *)d_c_hist, (unsigned long long *)d_cb_hist, d_dbfs_minmax, ctx->stream);
    SP_HIP(ctx, hipGetLastError());
    return SP_OK;
}

extern "C" int sp_merge_replies_batch(sp_context *ctx, const void *d_gathered, int32_t ranks, int32_t renders, int32_t lut_len, void *d_merged)
{
    if (!ctx || !d_gathered || !d_merged || ranks < 1 || renders < 1 || renders > 65535 || lut_len < 1 || lut_len > SP_MAX_LUT)
        return SP_ERR_INVALID_ARG;
    SP_HIP(ctx, hipSetDevice(ctx->device));
    const sphost::ReplyRecord rec{(size_t)lut_len, 0};
    // the merged records keep the record layout [c_hist | cB_hist | min, max]: the three outputs are one block, rec.words() per render
    const sp_reply m = rec.view(d_merged);
    spk::launch_merge_replies((const unsigned long long *)d_gathered, ranks, lut_len, (size_t)renders * rec.words(), renders,
                              (unsigned long long *)m.c_hist, (unsigned long long *)m.cb_hist, m.dbfs_minmax, ctx->stream);
    SP_HIP(ctx, hipGetLastError());
    return SP_OK;
}

// ------------------------------------------------------------------------------------------------- strip placement

extern "C" int sp_place_strips(sp_context *ctx, uint8_t *d_image, const uint8_t *d_strips, int32_t count, int32_t n, int32_t width,
                               int32_t slice_width, int32_t waterfall)
{
    if (!ctx || !d_image || !d_strips || count < 1 || n < 1 || width < 1 || slice_width < 0) return SP_ERR_INVALID_ARG;
    if ((int64_t)count * slice_width > width) return fail(ctx, SP_ERR_INVALID_ARG, "strips do not fit the image");
    if (slice_width == 0) return SP_OK;
    SP_HIP(ctx, hipSetDevice(ctx->device));
    const bool wide = (slice_width & 3) == 0 && (width & 3) == 0 && (((uintptr_t)d_image | (uintptr_t)d_strips) & 15) == 0
                      && (!waterfall || (n & 3) == 0);
    const int rc = spk::launch_place_strips(wide, d_image, d_strips, count, n, width, slice_width, waterfall, ctx->stream);
    if (rc) return fail(ctx, rc, "image too large for one placement launch");
    SP_HIP(ctx, hipGetLastError());
    return SP_OK;
}

// ------------------------------------------------------------------------------------------------- host-buffer render

// The pitched copies of one chunk, on `stream`.
static hipError_t upload_packed_chunk(const spgeo::PackedChunk &ch, int n, int sample_width, const uint8_t *bytes, size_t nbytes, uint8_t *stage,
                                      hipStream_t stream)
{
    const size_t sw = (size_t)sample_width;
    hipError_t e = hipSuccess;
    for (const spgeo::PackedBlock &b : ch.blocks) {
        int32_t j1 = b.j1;
        // the widened rows may reach past the capture's end in the request's very last rows: those travel one by one, exactly
        while (j1 > b.j0 && (size_t)(ch.first + (int64_t)(j1 - 1) * ch.F + b.dmax + n) * sw > nbytes) j1--;
        if (j1 > b.j0) {
            const size_t row_bytes = (size_t)(n + b.dmax - b.dmin) * sw;
            const uint8_t *src = bytes + (size_t)(ch.first + (int64_t)b.j0 * ch.F + b.dmin) * sw;
            uint8_t *dst = stage + ch.dev_off + (size_t)((int64_t)b.j0 * ch.P + b.dmin) * sw;
            if (j1 - b.j0 == 1) e = hipMemcpyAsync(dst, src, row_bytes, hipMemcpyHostToDevice, stream);
            else e = hipMemcpy2DAsync(dst, (size_t)ch.P * sw, src, (size_t)ch.F * sw, row_bytes, (size_t)(j1 - b.j0), hipMemcpyHostToDevice, stream);
            if (e != hipSuccess) return e;
        }
        for (int32_t j = j1; j < b.j1; j++) {
            const int32_t d = ch.drift[(size_t)j];
            e = hipMemcpyAsync(stage + ch.dev_off + (size_t)((int64_t)j * ch.P + d) * sw, bytes + (size_t)(ch.first + (int64_t)j * ch.F + d) * sw,
                               (size_t)n * sw, hipMemcpyHostToDevice, stream);
            if (e != hipSuccess) return e;
        }
    }
    return e;
}

// Frames [x0, x1) of the device image (`width` frames, rows 4 * width bytes apart) into the caller's image (rows host_pitch bytes
// apart) on `stream`: one copy where the band is contiguous on both sides (a waterfall band: rows width-1-x; the whole width of
// equally wide images), a pitched copy of columns x0 .. x1-1 of every row otherwise.
static hipError_t download_band(uint8_t *host, size_t host_pitch, const uint8_t *dev, int32_t width, size_t n, bool waterfall, int32_t x0,
                                int32_t x1, hipStream_t stream, size_t px = 4)
{
    const size_t W = (size_t)width;   // px: bytes per pixel (4: RGBA, 1: an index image)
    if (waterfall) {
        const size_t off = px * n * (W - (size_t)x1);
        return hipMemcpyAsync(host + off, dev + off, px * n * (size_t)(x1 - x0), hipMemcpyDeviceToHost, stream);
    }
    if (x0 == 0 && x1 == width && host_pitch == px * W) return hipMemcpyAsync(host, dev, px * W * n, hipMemcpyDeviceToHost, stream);
    return hipMemcpy2DAsync(host + px * (size_t)x0, host_pitch, dev + px * (size_t)x0, px * W, px * (size_t)(x1 - x0), n, hipMemcpyDeviceToHost,
                            stream);
}

// Every host-fed entry point (sp_render and its image kinds, sp_plan_execute_from_host, sp_render_density / _traces / _power and the
// plane consumers sp_render_mean / _bandpower / _track): the capture comes from HOST memory.  Large requests are
// rendered in chunks of frames: chunk k's samples travel to the device on copy_in while chunk k-1 is rendered and - where an image
// comes back - chunk k-2's part of it travels back on copy_out (PCIe is full duplex; the kernels are a few per cent of the copies).
// Chunks end on multiples of 32 frames (whole write-out groups); a chunk needs the samples up to the end of its last frame.  A request
// of one chunk does everything on the context's stream.  A sparse request (a frame-loop kernel) uploads only the samples its frames
// read.  stream_chunks is the only code that carries an UploadPlan out; a request kind brings its launch and what follows every chunk.
struct HostFeed {
    const char *who;        // the entry point, for its error texts
    const uint8_t *bytes;   // the capture, g.nbytes bytes of host memory
    spgeo::Geometry g;
    int32_t m;              // sub-frames per column: a contiguous chunk ends with its last column's last sub-frame (a plain frame loop: 1)
    bool packable;          // the request's kernel can read a packed chunk (SPECTROPLOT_HIP_NO_PACKED_UPLOAD overrides)
    bool chunkable;         // plan_upload's: the request may be pipelined ...
    size_t out_bytes;       // ... and the image that comes back over the link
    bool download;          // after_chunk copies back on copy_out: that stream and the ev_rendered events are wanted
    hipStream_t out_s;      // (set by stream_chunks) where after_chunk's copies go: copy_out, or the context's stream for one chunk
};

// a packed chunk as the kernel sees it: (virtual) sample 0 of its layout, a length that covers its last frame and one spare sample
// (3-byte samples are fetched as dwords), its stride
static PackedSource packed_source(const spgeo::PackedChunk &ch, const uint8_t *stage, int n, const spfmt::Format &f)
{
    PackedSource ps{};
    ps.bytes = stage + ch.dev_off - (size_t)ch.pos2_x0 * (size_t)f.width;
    ps.nbytes = (size_t)(ch.pos2_last + (int64_t)n + 1) * (size_t)f.width;
    ps.nbytes -= ps.nbytes % (size_t)f.elem;
    ps.stride = ch.stride2;
    return ps;
}

// The one way out of a failed host-fed request: nothing of it is left in flight, and the next request re-initialises the accumulators
// (harmless for a traces request, which has none: its workspace is cleared by every request).
static void drain_streams(sp_context *ctx)
{
    if (ctx->copy_in) (void)hipStreamSynchronize(ctx->copy_in);
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->copy_out) (void)hipStreamSynchronize(ctx->copy_out);
    ctx->acc_dirty = true;
}

// launch(x0, x1, first, last, d_in, src): the frame loop over chunk [x0, x1) on the context's stream, from the staging buffer d_in (src:
// the packed chunk, null for the contiguous upload); after_chunk(k, x0, x1): what follows chunk k's launch.  Both set the error they return.
template <typename Launch, typename AfterChunk>
static int stream_chunks(sp_context *ctx, const spfmt::Format &f, HostFeed &h, Launch &&launch, AfterChunk &&after_chunk)
{
    hipStream_t s = ctx->stream;
    const spgeo::Geometry &g = h.g;
    spgeo::UploadPlan u;
    spgeo::plan_upload(g, h.packable && !getenv("SPECTROPLOT_HIP_NO_PACKED_UPLOAD"), h.chunkable, h.out_bytes, u);
    const int chunks = (int)u.bounds.size() - 1;
    const bool overlap = chunks > 1;   // copies on copy_in / copy_out, ordered by events
    ctx->last_upload_bytes = u.link_bytes;
    ctx->last_chunks = chunks;
    int rc = ctx->in_bytes.reserve(u.dev_bytes);
    if (rc) return fail(ctx, rc, std::string(h.who) + ": out of memory");
    uint8_t *const in = (uint8_t *)ctx->in_bytes.p;
    hipError_t e = hipSuccess;
    if (overlap) {
        if (!ctx->copy_in) e = hipStreamCreateWithFlags(&ctx->copy_in, hipStreamNonBlocking);
        if (e == hipSuccess && h.download && !ctx->copy_out) e = hipStreamCreateWithFlags(&ctx->copy_out, hipStreamNonBlocking);
        for (int k = 0; k < chunks && e == hipSuccess; k++) {
            if (!ctx->ev_arrived[k]) e = hipEventCreateWithFlags(&ctx->ev_arrived[k], hipEventDisableTiming);
            if (e == hipSuccess && h.download && !ctx->ev_rendered[k]) e = hipEventCreateWithFlags(&ctx->ev_rendered[k], hipEventDisableTiming);
        }
        // whatever the stream still holds (an sp_plan_execute_from_host still reading the staging buffer, the caller's own work) comes
        // before this request's first copy; an idle stream is not waited for (that wait alone costs config 2 ~3 %)
        const bool busy = hipStreamQuery(s) != hipSuccess;
        (void)hipGetLastError();   // (hipErrorNotReady: the stream is busy, nothing failed)
        if (e == hipSuccess && busy) e = hipEventRecord(ctx->ev_arrived[0], s);
        if (e == hipSuccess && busy) e = hipStreamWaitEvent(ctx->copy_in, ctx->ev_arrived[0], 0);
    }
    hipStream_t in_s = overlap ? ctx->copy_in : s;
    h.out_s = overlap && h.download ? ctx->copy_out : s;
    size_t sent = 0;
    for (int k = 0; k < chunks && e == hipSuccess && !rc; k++) {
        const int32_t x0 = u.bounds[(size_t)k], x1 = u.bounds[(size_t)k + 1];
        PackedSource ps{};
        if (u.packed) {
            e = upload_packed_chunk(u.chunks[(size_t)k], g.n, f.width, h.bytes, g.nbytes, in, in_s);
            ps = packed_source(u.chunks[(size_t)k], in, g.n, f);
        } else {
            size_t need = g.nbytes;
            if (k + 1 < chunks) {
                need = (size_t)(g.start(x1 - 1) + (int64_t)h.m * g.n) * (size_t)f.width;
                if (need > g.nbytes) need = g.nbytes;
            }
            if (need > sent) {
                e = hipMemcpyAsync(in + sent, h.bytes + sent, need - sent, hipMemcpyHostToDevice, in_s);
                sent = need;
            }
        }
        if (e == hipSuccess && overlap) e = hipEventRecord(ctx->ev_arrived[k], in_s);
        if (e == hipSuccess && overlap) e = hipStreamWaitEvent(s, ctx->ev_arrived[k], 0);
        if (e == hipSuccess) rc = launch(x0, x1, k == 0, k + 1 == chunks, in, u.packed ? &ps : nullptr);
        if (e == hipSuccess && !rc) rc = after_chunk(k, x0, x1);
    }
    if (e != hipSuccess) rc = hip_fail(ctx, e, (std::string(h.who) + " copies").c_str());
    if (rc) drain_streams(ctx);
    return rc;
}

// stream_chunks for a request whose reply comes back chunk by chunk (feed.download): copy(x0, x1, stream) queues the copy of the frames
// [x0, x1) - never empty - on `stream`, which waits for the chunk's launch first; tail() queues what else the request has for the
// context's stream once every chunk has been launched.  Returns when everything has arrived.
template <typename Launch, typename Copy, typename Tail>
static int download_chunks(sp_context *ctx, const spfmt::Format &f, HostFeed &feed, Launch &&launch, Copy &&copy, Tail &&tail)
{
    hipStream_t s = ctx->stream;
    const auto copies_failed = [&](hipError_t e) { return hip_fail(ctx, e, (std::string(feed.who) + " copies").c_str()); };
    const int rc = stream_chunks(ctx, f, feed, launch, [&](int k, int32_t x0, int32_t x1) {
        hipError_t e = hipSuccess;
        if (feed.out_s != s) e = hipEventRecord(ctx->ev_rendered[k], s);
        if (e == hipSuccess && feed.out_s != s) e = hipStreamWaitEvent(feed.out_s, ctx->ev_rendered[k], 0);
        if (e == hipSuccess && x1 > x0) e = copy(x0, x1, feed.out_s);
        return e == hipSuccess ? (int)SP_OK : copies_failed(e);
    });
    if (rc) return rc;
    hipError_t e = tail();
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess && feed.out_s != s) e = hipStreamSynchronize(feed.out_s);
    if (e != hipSuccess) {
        drain_streams(ctx);
        return copies_failed(e);
    }
    return SP_OK;
}

// The small outputs of a request side by side in a context buffer on the device, as a reply without an image.
static int device_reply_record(DeviceBuffer &buf, const sphost::ReplyRecord &rec, sp_reply *d)
{
    const int rc = buf.reserve(rec.bytes() + 16);
    if (rc) return rc;
    *d = rec.view(buf.p);
    d->rgba = nullptr;
    return SP_OK;
}

// The image of a host-fed request.  device_out = false: the reply's pointers are host pointers; the device image lies in `dev` and
// travels back chunk by chunk, the small outputs in one copy, and the call returns when everything has arrived.  device_out = true:
// the reply's pointers and `host` are device pointers (as for sp_plan_execute); the kernels write them, nothing comes back, and the
// call returns once everything is queued.
struct HostImage {
    uint8_t *host;         // the caller's image; may be null: side outputs only
    size_t px;             // bytes per pixel: 4 (RGBA) or 1 (an index image)
    size_t host_pitch;     // bytes between rows of the caller's image
    DeviceBuffer *dev;     // the context buffer that holds the device image
    Picture::Kind kind;    // how plan_execute_range writes it
    bool device_out;
};

// A host-fed request with an image (render_rgba, sp_render_index).  `who`: the entry point, for its error texts.
static int render_image(sp_plan *plan, const char *who, const uint8_t *bytes, size_t nbytes, int32_t width, const sp_reply *reply,
                        const HostImage &im)
{
    sp_context *ctx = plan->ctx;
    const sp_request *req = &plan->req;

    const size_t W = (size_t)width, n = (size_t)req->n;
    const size_t image_bytes = im.px * W * n;
    const sphost::ReplyRecord rec{(size_t)req->lut_len, W};   // the small outputs, side by side on the device
    int rc = SP_OK;
    sp_reply d = *reply;
    Picture pic{im.kind, im.host};
    if (!im.device_out) {
        rc = im.dev->reserve(image_bytes + 16);
        if (!rc) rc = device_reply_record(ctx->render_small, rec, &d);
        if (!rc) rc = ctx->host_small.reserve(rec.bytes() + 16);
        if (rc) return fail(ctx, rc, std::string(who) + ": out of memory");
        pic.image = im.host ? (uint8_t *)im.dev->p : nullptr;
    }

    const RequestShape shape = request_shape(plan, nbytes, width);   // once, for the upload plan and every chunk's launch
    // (device_out: no image crosses the link, so the samples are the longer transfer whatever the image weighs)
    // (a peak request with M >= 2 sub-frames per column reads more than half of the capture: the contiguous upload, chunked by columns)
    HostFeed feed{who, bytes, shape.g, shape.peak.m, request_kernel(plan, shape.peak.m) == kKernelFrames,
                  im.device_out || im.host, im.device_out ? 0 : image_bytes, !im.device_out, nullptr};
    // (nothing to clear: the kernels overwrite every histogram count, both range values and every gauge byte)
    auto launch = [&](int32_t x0, int32_t x1, bool first, bool last, const uint8_t *d_in, const PackedSource *src) {
        return plan_execute_range(plan, d_in, shape, x0, x1, first, last, &d, pic, src);
    };
    if (im.device_out) return stream_chunks(ctx, plan->fmt, feed, launch, [](int, int32_t, int32_t) { return (int)SP_OK; });
    rc = download_chunks(
        ctx, plan->fmt, feed, launch,
        [&](int32_t x0, int32_t x1, hipStream_t out_s) {
            return im.host ? download_band(im.host, im.host_pitch, pic.image, width, n, req->waterfall, x0, x1, out_s, im.px) : hipSuccess;
        },
        // the small outputs sit side by side on the device: one copy into the context's page-locked block, handed out from there
        // (separate copies into pageable memory cost more than the kernels of a small request)
        [&] { return hipMemcpyAsync(ctx->host_small.p, ctx->render_small.p, rec.bytes(), hipMemcpyDeviceToHost, ctx->stream); });
    if (rc) return rc;
    rec.unpack_side(ctx->host_small.p, *reply);
    rec.unpack_gauges(ctx->host_small.p, *reply);
    return SP_OK;
}

// sp_render / sp_render_strip / sp_plan_execute_from_host.  `image_width` is the width in frames of the image reply->rgba points into
// (the strip's own width for sp_render); it only matters for the spectrogram layout, whose rows are image_width pixels apart.
static int render_rgba(sp_plan *plan, const uint8_t *bytes, size_t nbytes, int32_t width, const sp_reply *reply, int32_t image_width,
                       bool device_out)
{
    const HostImage im{reply->rgba, 4, 4 * (size_t)(plan->req.waterfall ? plan->req.n : image_width), &plan->ctx->out_rgba, Picture::kRgba, device_out};
    return render_image(plan, "sp_render", bytes, nbytes, width, reply, im);
}

// sp_render_density / sp_render_traces / plane_render (sp_render_mean, _bandpower, _track): a host-fed request without an image, whose
// small result accumulates or fills on the device over the chunks.  The samples are the only transfer and nothing follows a chunk (stream_chunks as sp_plan_execute_from_host feeds it).  A kind
// brings clear() (its result back at its initial value), launch (stream_chunks') and tail(cleared, e): what it queues on the context's
// stream once every chunk has been launched - `cleared`: clear() has run - with a failed copy's error left in e.  The call returns
// when the stream has ended.
template <typename Clear, typename Launch, typename Tail>
static int render_result(sp_context *ctx, const spfmt::Format &f, HostFeed &feed, Clear &&clear, Launch &&launch, Tail &&tail)
{
    bool cleared = false;
    // (the clear belongs to the first chunk's launch: queued earlier, it would make the stream look busy to the streamer)
    auto chunk = [&](int32_t x0, int32_t x1, bool first, bool last, const uint8_t *d_in, const PackedSource *src) {
        if (first) {
            const int r = clear();
            if (r) return r;
            cleared = true;
        }
        return launch(x0, x1, first, last, d_in, src);
    };
    int rc = stream_chunks(ctx, f, feed, chunk, [](int, int32_t, int32_t) { return (int)SP_OK; });   // (nothing follows a chunk)
    hipError_t e = hipSuccess;
    if (!rc) rc = tail(cleared, e);
    const hipError_t es = hipStreamSynchronize(ctx->stream);   // (synchronous; the samples' stream has ended before this one)
    if (rc) return rc;
    if (e != hipSuccess || es != hipSuccess) return hip_fail(ctx, e != hipSuccess ? e : es, (std::string(feed.who) + " copies").c_str());
    return SP_OK;
}

// The context's cached plan if it serves `req`, else a new one in its place.
static int cached_plan_for(sp_context *ctx, const sp_request *req, sp_plan **plan)
{
    const sp_plan *cp = ctx->cached_plan;
    if (!cp || !sphost::same_request(cp->req, cp->window, cp->lut, req)) {
        if (ctx->cached_plan) sp_plan_destroy(ctx->cached_plan);
        ctx->cached_plan = nullptr;
        const int rc = sp_plan_create(ctx, req, &ctx->cached_plan);
        if (rc) return rc;
    }
    *plan = ctx->cached_plan;
    return SP_OK;
}

// What every host entry point refuses of its capture before it touches the device, in this order; then the context's device is current.
static int check_host_capture(sp_context *ctx, const spfmt::Format &f, const uint8_t *bytes, size_t nbytes, int32_t width)
{
    if (width < 0) return fail(ctx, SP_ERR_INVALID_ARG, "width < 0");
    if (nbytes && !bytes) return fail(ctx, SP_ERR_INVALID_ARG, "bytes is null");
    // the reference constructs its typed view before anything else (worker.js:24)
    if (nbytes % (size_t)f.elem) return fail(ctx, SP_ERR_BYTE_LENGTH, "byte length is not a multiple of the element size");
    SP_HIP(ctx, hipSetDevice(ctx->device));
    return SP_OK;
}

// How every host entry point that takes a request begins: the request's validation, the kind's own refusals of the request, the
// capture's, the kind's own refusals of the capture, then the context's cached plan.
template <typename CheckRequest, typename CheckCapture>
static int host_request(sp_context *ctx, const sp_request *req, const uint8_t *bytes, size_t nbytes, int32_t width, CheckRequest &&check_request,
                        CheckCapture &&check_kind_capture, sp_plan **plan)
{
    int rc = validate_request(ctx, req);
    if (!rc) rc = check_request();
    if (!rc) rc = check_host_capture(ctx, spfmt::describe(req->format), bytes, nbytes, width);
    if (!rc) rc = check_kind_capture();
    return rc ? rc : cached_plan_for(ctx, req, plan);
}
static int no_check() { return SP_OK; }

extern "C" int sp_render_strip(sp_context *ctx, const sp_request *req, const uint8_t *bytes, size_t nbytes, int32_t width,
                               const sp_reply *reply, int32_t image_width)
{
    if (!ctx || !reply) return SP_ERR_INVALID_ARG;
    sp_plan *plan = nullptr;
    const auto check = [&] {   // (a width < 0 is refused first)
        return width >= 0 && image_width < width ? fail(ctx, SP_ERR_INVALID_ARG, "image_width < width") : (int)SP_OK;
    };
    const int rc = host_request(ctx, req, bytes, nbytes, width, check, no_check, &plan);
    return rc ? rc : render_rgba(plan, bytes, nbytes, width, reply, image_width, false);
}

extern "C" int sp_render(sp_context *ctx, const sp_request *req, const uint8_t *bytes, size_t nbytes, int32_t width, const sp_reply *reply)
{
    return sp_render_strip(ctx, req, bytes, nbytes, width, reply, width);
}

extern "C" int sp_plan_execute_from_host(sp_plan *plan, const uint8_t *bytes, size_t nbytes, int32_t width, const sp_reply *d_reply)
{
    if (!plan || !d_reply) return SP_ERR_INVALID_ARG;
    const int rc = check_host_capture(plan->ctx, plan->fmt, bytes, nbytes, width);
    return rc ? rc : render_rgba(plan, bytes, nbytes, width, d_reply, width, true);
}

extern "C" int sp_context_last_upload_bytes(const sp_context *ctx, size_t *nbytes)
{
    if (!ctx || !nbytes) return SP_ERR_INVALID_ARG;
    *nbytes = ctx->last_upload_bytes;
    return SP_OK;
}

extern "C" int sp_context_last_chunks(const sp_context *ctx, int32_t *chunks)
{
    if (!ctx || !chunks) return SP_ERR_INVALID_ARG;
    *chunks = ctx->last_chunks;
    return SP_OK;
}

// ------------------------------------------------------------------------------------------------- indexed image replies

// k_frames_index renders what k_frames renders of a sample plan, where its variant exists (frames_index_variant_built).
static bool index_frames(const sp_plan *plan, const spgeo::Geometry &g)
{
    if (plan->req.detector != SP_DETECTOR_SAMPLE || request_kernel(plan, 1) != kKernelFrames) return false;
    return spk2::frames_index_variant_built(plan->req.n, plan->req.channel_mode != 0,
                                            spk2::frames_prefetch_width(plan->fmt.width, g.in_bounds, g.stride, g.width));
}

extern "C" const char *sp_plan_index_kernel_name_for(const sp_plan *plan, size_t nbytes, int32_t width)
{
    if (!plan) return "";
    return index_frames(plan, spgeo::geometry(plan->fmt, plan->req.n, nbytes, width)) ? "frames_index" : "render_extract";
}

// what the render_extract path needs before its first launch: the temporary RGBA image and the plan's identity LUT
static int index_prepare(sp_plan *plan, Picture::Kind kind, int32_t width)
{
    if (kind != Picture::kIndexExtract || width <= 0) return SP_OK;
    sp_context *ctx = plan->ctx;
    int rc = ctx->index_rgba.reserve(4 * (size_t)width * (size_t)plan->req.n + 16);
    if (rc) return fail(ctx, rc, "index workspace: out of device memory");
    if (!plan->ident_lut.p) {
        // (a table with static storage: the asynchronous copy may read it whenever it runs, so the entry point stays asynchronous)
        static const std::vector<uint32_t> ident = [] {
            std::vector<uint32_t> t(256);
            for (uint32_t i = 0; i < 256; i++) t[i] = i | 0xff000000u;
            return t;
        }();
        rc = plan->ident_lut.reserve(ident.size() * sizeof(uint32_t));
        if (rc) return fail(ctx, rc, "identity LUT: out of device memory");
        const hipError_t e = hipMemcpyAsync(plan->ident_lut.p, ident.data(), ident.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) {
            plan->ident_lut.release();
            return hip_fail(ctx, e, "identity LUT upload");
        }
    }
    return SP_OK;
}

// what every indexed entry point refuses of a plan or request and its reply
static int check_index(sp_context *ctx, int32_t lut_len, const sp_reply *reply)
{
    if (lut_len > 256) return fail(ctx, SP_ERR_UNSUPPORTED, "an indexed image holds one byte per pixel: lut_len must be 256 at most");
    if (reply->rgba) return fail(ctx, SP_ERR_INVALID_ARG, "an indexed request's reply must not carry an RGBA image (rgba must be NULL)");
    return SP_OK;
}

static int no_object_status()
{
    int c = 0;
    return hipGetDeviceCount(&c) != hipSuccess || c <= 0 ? SP_ERR_NO_DEVICE : SP_ERR_INVALID_ARG;
}

extern "C" int sp_plan_execute_index(sp_plan *plan, const void *d_bytes, size_t nbytes, int32_t width, const sp_reply *d_reply, uint8_t *d_index)
{
    if (!plan) return no_object_status();
    if (!d_reply) return SP_ERR_INVALID_ARG;
    sp_context *ctx = plan->ctx;
    int rc = check_index(ctx, plan->req.lut_len, d_reply);
    if (rc) return rc;
    const RequestShape shape = request_shape(plan, nbytes, width);
    const Picture pic = index_picture(d_index, index_frames(plan, shape.g));
    if (pic.kind == Picture::kIndexExtract && width > 0) {
        rc = device_operands(ctx, plan->fmt, plan->req.n, d_bytes, nbytes, width, d_reply, "sp_plan_execute_index");   // (before anything is allocated)
        if (rc) return rc;
    }
    rc = index_prepare(plan, pic.kind, width);
    return rc ? rc : plan_execute_range(plan, d_bytes, shape, 0, width < 0 ? 0 : width, true, true, d_reply, pic);
}

// sp_render with an indexed image: a request kind of stream_chunks whose image travels back at 1 byte per pixel.
extern "C" int sp_render_index(sp_context *ctx, const sp_request *req, const uint8_t *bytes, size_t nbytes, int32_t width, const sp_reply *reply,
                               uint8_t *index)
{
    if (!ctx) return no_object_status();
    if (!reply) return SP_ERR_INVALID_ARG;
    sp_plan *plan = nullptr;
    int rc = host_request(ctx, req, bytes, nbytes, width, [&] { return check_index(ctx, req->lut_len, reply); }, no_check, &plan);
    if (rc) return rc;
    const bool frames = index_frames(plan, spgeo::geometry(plan->fmt, req->n, nbytes, width));
    // (the device image of a host-fed request, here 1 byte per pixel)
    const HostImage im{index, 1, req->waterfall ? (size_t)req->n : (size_t)width, &ctx->out_rgba, index_picture(index, frames).kind, false};
    rc = index_prepare(plan, im.kind, width);
    return rc ? rc : render_image(plan, "sp_render_index", bytes, nbytes, width, reply, im);
}

extern "C" int sp_index_to_rgba(sp_context *ctx, const uint8_t *d_index, size_t pixels, const uint8_t *lut_rgb, int32_t lut_len, uint8_t *d_rgba)
{
    if (!ctx) return no_object_status();
    if (!lut_rgb || lut_len < 1 || lut_len > 256 || (pixels && (!d_index || !d_rgba))) return SP_ERR_INVALID_ARG;
    if (!pixels) return SP_OK;
    SP_HIP(ctx, hipSetDevice(ctx->device));
    IndexLut lut;
    for (int i = 0; i < 256; i++)
        lut.v[i] = i < lut_len ? (uint32_t)lut_rgb[3 * i] | ((uint32_t)lut_rgb[3 * i + 1] << 8) | ((uint32_t)lut_rgb[3 * i + 2] << 16) | 0xff000000u
                               : 0xff000000u;   // an index the map does not have: opaque black
    const int rc = spk::launch_index_to_rgba(d_index, pixels, lut, d_rgba, ctx->stream);
    if (rc) return fail(ctx, rc, "image too large for one recolouring launch");
    SP_HIP(ctx, hipGetLastError());
    return SP_OK;
}

// (tests) sp_plan_debug_launch's words for the launch sp_plan_execute_index would make; word 0 is 5 for k_frames_index, and word 8 tells
// whether the write-out stores the index image in 16-byte pieces.
extern "C" int sp_plan_debug_index_launch(const sp_plan *plan, size_t nbytes, int32_t width, const void *index, int64_t *out, size_t capacity,
                                          size_t *used)
{
    int rc = sp_plan_debug_launch(plan, nbytes, width, nullptr, out, capacity, used);
    if (rc) return rc;
    if (width > 0 && index_frames(plan, spgeo::geometry(plan->fmt, plan->req.n, nbytes, width))) {
        out[0] = 5;
        out[8] = index_fast((const uint8_t *)index, width, plan->req.n, 0, width) ? 1 : 0;
    }
    return SP_OK;
}

// ------------------------------------------------------------------------------------------------- persistence spectrum

// what every density entry point refuses of its colour-map length and its output
static int check_density(sp_context *ctx, int32_t lut_len, const uint32_t *density)
{
    if (lut_len > 256) return fail(ctx, SP_ERR_UNSUPPORTED, "the density counts an indexed image's bytes: lut_len must be 256 at most");
    if (lut_len < 1) return fail(ctx, SP_ERR_INVALID_ARG, "lut_len < 1");
    if (!density || ((uintptr_t)density & 3) != 0) return fail(ctx, SP_ERR_INVALID_ARG, "density must be a 4-byte aligned array of n * lut_len counts");
    return SP_OK;
}

extern "C" int sp_density_from_index(sp_context *ctx, const uint8_t *d_index, int32_t n, int32_t width, int32_t waterfall, int32_t lut_len,
                                     uint32_t *d_density, int32_t accumulate)
{
    if (!ctx) return no_object_status();
    if (lut_len > 256) return fail(ctx, SP_ERR_INVALID_ARG, "lut_len must be 1 ... 256");   // (no request here whose map the reference allows)
    int rc = check_density(ctx, lut_len, d_density);
    if (rc) return rc;
    if (n < 1 || width < 0 || (width > 0 && !d_index)) return fail(ctx, SP_ERR_INVALID_ARG, "n >= 1, width >= 0 and an index image are needed");
    if ((double)width * (double)n > 4e12) return fail(ctx, SP_ERR_UNSUPPORTED, "image too large");
    SP_HIP(ctx, hipSetDevice(ctx->device));
    return timed(ctx, [&]() -> int {
        if (!accumulate) SP_HIP(ctx, hipMemsetAsync(d_density, 0, (size_t)n * (size_t)lut_len * sizeof(uint32_t), ctx->stream));
        return density_count(ctx, d_index, n, width, waterfall != 0, lut_len, 0, width, d_density);
    });
}

// the index image and the reply record of a density request on device operands: both the context's, ordered on its stream
static int density_prepare(sp_plan *plan, int32_t width, sp_reply *d, Picture *pic, const spgeo::Geometry &g)
{
    sp_context *ctx = plan->ctx;
    const sphost::ReplyRecord rec{(size_t)plan->req.lut_len, (size_t)width};
    int rc = ctx->density_index.reserve((size_t)width * (size_t)plan->req.n + 16);
    if (!rc) rc = device_reply_record(ctx->density_reply, rec, d);
    if (rc) return fail(ctx, rc, "density workspace: out of device memory");
    *pic = index_picture((uint8_t *)ctx->density_index.p, index_frames(plan, g));
    return index_prepare(plan, pic->kind, width);
}

extern "C" int sp_plan_execute_density(sp_plan *plan, const void *d_bytes, size_t nbytes, int32_t width, uint32_t *d_density, int32_t accumulate)
{
    if (!plan) return no_object_status();
    sp_context *ctx = plan->ctx;
    const int n = plan->req.n, lut_len = plan->req.lut_len;
    int rc = check_density(ctx, lut_len, d_density);
    if (!rc) rc = device_operands(ctx, plan->fmt, n, d_bytes, nbytes, width, nullptr, "sp_plan_execute_density");   // (before anything is allocated)
    if (rc) return rc;
    hipStream_t s = ctx->stream;
    const RequestShape shape = request_shape(plan, nbytes, width);
    sp_reply d{};
    Picture pic{};
    rc = density_prepare(plan, width, &d, &pic, shape.g);
    if (rc) return rc;
    rc = plan_execute_range(plan, d_bytes, shape, 0, width, true, true, &d, pic);
    if (rc) return rc;
    if (!accumulate) SP_HIP(ctx, hipMemsetAsync(d_density, 0, (size_t)n * (size_t)lut_len * sizeof(uint32_t), s));
    rc = density_count(ctx, pic.image, n, width, plan->req.waterfall != 0, lut_len, 0, width, d_density);
    if (rc) return rc;
    if (ctx->timing && width > 0) SP_HIP(ctx, hipEventRecord(ctx->ev1, s));   // (timing: the render's event pair now ends behind the count)
    return SP_OK;
}

// A request kind of render_result: every chunk's launch renders its frames into the index image on the device and counts them; the
// counts come back in one copy.
extern "C" int sp_render_density(sp_context *ctx, const sp_request *req, const uint8_t *bytes, size_t nbytes, int32_t width, uint32_t *density)
{
    if (!ctx) return no_object_status();
    sp_plan *plan = nullptr;
    int rc = host_request(
        ctx, req, bytes, nbytes, width, [&] { return check_density(ctx, req->lut_len, density); },
        [&] { return check_capture(ctx, spfmt::describe(req->format), req->n, bytes, nbytes, width, nullptr, ""); }, &plan);
    if (rc) return rc;

    hipStream_t s = ctx->stream;
    const int n = req->n, lut_len = req->lut_len;
    const size_t count_bytes = (size_t)n * (size_t)lut_len * sizeof(uint32_t);
    rc = ctx->render_small.reserve(count_bytes + 16);
    if (rc) return fail(ctx, rc, "sp_render_density: out of memory");
    uint32_t *const d_density = (uint32_t *)ctx->render_small.p;
    const RequestShape shape = request_shape(plan, nbytes, width);
    sp_reply d{};
    Picture pic{};
    rc = density_prepare(plan, width, &d, &pic, shape.g);
    if (rc) return rc;
    HostFeed feed{"sp_render_density", bytes, shape.g, shape.peak.m, request_kernel(plan, shape.peak.m) == kKernelFrames, true, 0, false, nullptr};
    const auto zero = [&] { return hipMemsetAsync(d_density, 0, count_bytes, s); };
    return render_result(
        ctx, plan->fmt, feed,
        [&] {
            const hipError_t e = zero();
            return e == hipSuccess ? (int)SP_OK : hip_fail(ctx, e, "sp_render_density clear");
        },
        [&](int32_t x0, int32_t x1, bool first, bool last, const uint8_t *d_in, const PackedSource *src) {
            const int r = plan_execute_range(plan, d_in, shape, x0, x1, first, last, &d, pic, src);
            return r ? r : density_count(ctx, pic.image, n, width, req->waterfall != 0, lut_len, x0, x1, d_density);
        },
        [&](bool cleared, hipError_t &e) {
            if (!cleared) e = zero();   // (no chunk ran)
            if (e == hipSuccess) e = hipMemcpyAsync(density, d_density, count_bytes, hipMemcpyDeviceToHost, s);
            return (int)SP_OK;
        });
}

// (tests) k_density_count's decomposition from the functions its launch calls: six words, then every workgroup's rectangle.
extern "C" int sp_debug_density_launch(int32_t n, int32_t width, int32_t waterfall, int32_t x_begin, int32_t x_end, int64_t *out, size_t capacity,
                                       size_t *used)
{
    if (n < 1 || width < 0 || x_begin < 0 || x_end < x_begin || x_end > width || !used) return SP_ERR_INVALID_ARG;
    const DensityShape d = density_shape(n, waterfall != 0, x_begin, x_end);
    const long long grid = d.bands * d.pieces;
    *used = 6 + 4 * (size_t)grid;
    if (!out || capacity < *used) return SP_ERR_INVALID_ARG;
    out[0] = grid;
    out[1] = d.rows;
    out[2] = d.frames;
    out[3] = (int64_t)d.rows * 256 * (int64_t)sizeof(uint32_t);
    out[4] = d.bands;
    out[5] = d.pieces;
    for (long long wg = 0; wg < grid; wg++) {
        int y0, y1, x0, x1;
        density_rect(d, n, x_begin, x_end, wg, y0, y1, x0, x1);
        int64_t *const r = out + 6 + 4 * wg;
        r[0] = y0, r[1] = y1, r[2] = x0, r[3] = x1;
    }
    return SP_OK;
}

// ------------------------------------------------------------------------------------------------- plain frame loops (traces, power planes)

// k_frames_traces and k_frames_power need what k_frames needs of the transform - a finite taper (the (1, 0) butterflies skip their
// products on integer samples) and the first-pass twiddle literals - and nothing of the picture: LUT length and edge ranges do not
// matter to a trace or a plane.
static_assert(spk2::kTracesMaxLog2N == spk2::kPowerMaxLog2N, "plan_plain_frames asks frames_traces_supports for both kernels: their limits must agree");
static bool plan_plain_frames(const sp_plan *plan)
{
    return plan->force_kernel != kKernelScratch && spk2::frames_traces_supports(plan->req.n) && plan->taper_finite && plan->tw16_ok;
}

// The two kinds of plain_range: where the kernels write (Out), the slabs of a scratch workgroup, the LUT length the frame-loop launcher
// asks for, that launcher, its refusal's text, the scratch kernel's launcher and the refusal of a peak plan.
struct TracesKind {
    using Out = unsigned long long;   // the context's workspace (traces_clear)
    static constexpr int kSlabs = 4;   // re, im, the bins' minima and maxima
    static constexpr int kLutLen = spk2::kTracesLutLen;
    static constexpr auto launch_frames = spk2::launch_frames_traces;
    static constexpr const char *kRejected = "k_frames_traces launch rejected the configuration";
    static constexpr const char *kOfPeak = "traces of a peak plan are not supported (the traces fold the sample detector's frames)";
    static constexpr auto launch_scratch = spk::launch_scratch_traces;
};
struct PowerKind {
    using Out = double;   // the plane, frame x at out + x * n
    static constexpr int kSlabs = 2;   // re, im
    static constexpr int kLutLen = spk2::kPowerLutLen;
    static constexpr auto launch_frames = spk2::launch_frames_power;
    static constexpr const char *kRejected = "k_frames_power launch rejected the configuration";
    static constexpr const char *kOfPeak = "the power plane of a peak plan is not supported (the plane holds the sample detector's frames)";
    static constexpr auto launch_scratch = spk::launch_scratch_power;
};

// The frame loop over frames [x_begin, x_end) of a traces or power request into `out` (`src`: as for plan_execute_range).  One launch.
template <typename Kind>
static int plain_range(sp_plan *plan, const void *d_bytes, const spgeo::Geometry &g, int32_t x_begin, int32_t x_end, const PackedSource *src,
                       typename Kind::Out *out)
{
    sp_context *ctx = plan->ctx;
    if (x_end <= x_begin) return SP_OK;
    const bool frames = plan_plain_frames(plan);
    if (src && !frames) return fail(ctx, SP_ERR_INVALID_ARG, "a packed source is for the frame-loop kernel only");
    spk::FrameArgs a{};
    plan_frame_args(plan, a);
    frame_source_args(a, plan, d_bytes, g, x_begin, x_end, src);
    hipStream_t s = ctx->stream;
    if (frames) {
        a.lut_len = Kind::kLutLen;   // (the shared prologue copies this many LUT and edge entries: the plan's tables hold them)
        a.cells = 0;
        const int rc = Kind::launch_frames(a, plan->req.format, plan->d_stage_tw, out, ctx->cu_count, ctx->device, s);
        if (rc) return fail(ctx, rc, Kind::kRejected);
    } else {
        unsigned blocks;
        int rc = scratch_reserve(ctx, a, Kind::kSlabs, x_end - x_begin, &blocks);
        if (rc) return rc;
        rc = Kind::launch_scratch(a, plan->req.format, blocks, out, s);
        if (rc) return fail(ctx, rc, "bad format");
    }
    SP_HIP(ctx, hipGetLastError());
    return SP_OK;
}

// What sp_plan_*_kernel_name_for tells of a plain frame loop and what runs behind it: one of two names (every shape of a plan takes the
// same kernel today).
static const char *plain_kernel_name(const sp_plan *plan, const char *frames, const char *scratch)
{
    return !plan ? "" : plan_plain_frames(plan) ? frames : scratch;
}

// what every entry point of a kind refuses of a plan's or a request's detector, format and frame size before it touches the device
template <typename Kind>
static int check_plain(sp_context *ctx, int32_t detector, const spfmt::Format &f, int n, const void *bytes, size_t nbytes, int32_t width)
{
    if (detector != SP_DETECTOR_SAMPLE) return fail(ctx, SP_ERR_UNSUPPORTED, Kind::kOfPeak);
    return check_capture(ctx, f, n, bytes, nbytes, width, nullptr, "");
}

// ------------------------------------------------------------------------------------------------- per-bin min / max traces

extern "C" const char *sp_plan_traces_kernel_name_for(const sp_plan *plan, size_t, int32_t)
{
    return plain_kernel_name(plan, "frames_traces", "scratch_traces");
}

static int traces_clear(sp_plan *plan)
{
    sp_context *ctx = plan->ctx;
    const int n = plan->req.n;
    const int rc = ctx->traces_ws.reserve(2 * (size_t)n * sizeof(unsigned long long));
    if (rc) return fail(ctx, rc, "traces workspace: out of device memory");
    spk::launch_traces_clear((unsigned long long *)ctx->traces_ws.p, n, ctx->stream);
    SP_HIP(ctx, hipGetLastError());
    return SP_OK;
}

static int traces_finish(sp_plan *plan, double *d_trace_min, double *d_trace_max)
{
    sp_context *ctx = plan->ctx;
    spk::launch_traces_finish((const unsigned long long *)ctx->traces_ws.p, plan->req.n, plan->block_norm_db, plan->req.gain, d_trace_min, d_trace_max,
                              ctx->stream);
    SP_HIP(ctx, hipGetLastError());
    return SP_OK;
}

extern "C" int sp_plan_execute_traces(sp_plan *plan, const void *d_bytes, size_t nbytes, int32_t width, double *d_trace_min,
                                      double *d_trace_max)
{
    if (!plan) return SP_ERR_INVALID_ARG;
    sp_context *ctx = plan->ctx;
    int rc = check_plain<TracesKind>(ctx, plan->req.detector, plan->fmt, plan->req.n, d_bytes, nbytes, width);
    if (rc) return rc;
    if ((((uintptr_t)d_trace_min | (uintptr_t)d_trace_max) & 7) != 0)
        return fail(ctx, SP_ERR_INVALID_ARG, "d_trace_min and d_trace_max must be 8-byte aligned");
    SP_HIP(ctx, hipSetDevice(ctx->device));
    const spgeo::Geometry g = spgeo::geometry(plan->fmt, plan->req.n, nbytes, width);
    return timed(ctx, [&] {
        int r = traces_clear(plan);
        if (!r) r = plain_range<TracesKind>(plan, d_bytes, g, 0, width, nullptr, (unsigned long long *)ctx->traces_ws.p);
        return r ? r : traces_finish(plan, d_trace_min, d_trace_max);
    });
}

// A request kind of render_result - a packed sparse upload where stride > n, chunks of frames where the request is large - whose
// extremes accumulate in the workspace over the chunks.
extern "C" int sp_render_traces(sp_context *ctx, const sp_request *req, const uint8_t *bytes, size_t nbytes, int32_t width, double *trace_min,
                                double *trace_max)
{
    if (!ctx) return SP_ERR_INVALID_ARG;
    sp_plan *plan = nullptr;
    int rc = host_request(
        ctx, req, bytes, nbytes, width, no_check,
        [&] { return check_plain<TracesKind>(ctx, req->detector, spfmt::describe(req->format), req->n, bytes, nbytes, width); }, &plan);
    if (rc) return rc;

    const size_t n = (size_t)req->n;
    hipStream_t s = ctx->stream;
    rc = ctx->render_small.reserve(2 * n * sizeof(double) + 16);
    if (rc) return fail(ctx, rc, "sp_render_traces: out of memory");
    double *const d_out = (double *)ctx->render_small.p;
    HostFeed feed{"sp_render_traces", bytes, spgeo::geometry(plan->fmt, req->n, nbytes, width), 1, plan_plain_frames(plan), true, 0, false, nullptr};
    return render_result(
        ctx, plan->fmt, feed, [&] { return traces_clear(plan); },
        [&](int32_t x0, int32_t x1, bool, bool, const uint8_t *d_in, const PackedSource *src) {
            return plain_range<TracesKind>(plan, d_in, feed.g, x0, x1, src, (unsigned long long *)ctx->traces_ws.p);
        },
        [&](bool, hipError_t &e) {
            const int r = traces_finish(plan, trace_min ? d_out : nullptr, trace_max ? d_out + n : nullptr);
            if (!r && trace_min) e = hipMemcpyAsync(trace_min, d_out, n * sizeof(double), hipMemcpyDeviceToHost, s);
            if (!r && e == hipSuccess && trace_max) e = hipMemcpyAsync(trace_max, d_out + n, n * sizeof(double), hipMemcpyDeviceToHost, s);
            return r;
        });
}

// ------------------------------------------------------------------------------------------------- power plane replies

extern "C" const char *sp_plan_power_kernel_name_for(const sp_plan *plan, size_t, int32_t)
{
    return plain_kernel_name(plan, "frames_power", "scratch_power");
}

// d_db[k] = d of d_power[k], k < count, on the context's stream (count > 0; in place where the pointers are equal)
static int power_to_db(sp_plan *plan, const double *d_power, size_t count, double *d_db)
{
    sp_context *ctx = plan->ctx;
    spk::launch_power_to_db(d_power, count, plan->block_norm_db, plan->req.gain, d_db, ctx->cu_count, ctx->stream);
    SP_HIP(ctx, hipGetLastError());
    return SP_OK;
}

extern "C" int sp_plan_execute_power(sp_plan *plan, const void *d_bytes, size_t nbytes, int32_t width, double *d_power)
{
    if (!plan) return SP_ERR_INVALID_ARG;
    sp_context *ctx = plan->ctx;
    int rc = check_plain<PowerKind>(ctx, plan->req.detector, plan->fmt, plan->req.n, d_bytes, nbytes, width);
    if (rc) return rc;
    if (width > 0 && (!d_power || ((uintptr_t)d_power & 7) != 0))
        return fail(ctx, SP_ERR_INVALID_ARG, "d_power must be an 8-byte aligned array of width * n doubles");
    if (width == 0) return SP_OK;
    SP_HIP(ctx, hipSetDevice(ctx->device));
    const spgeo::Geometry g = spgeo::geometry(plan->fmt, plan->req.n, nbytes, width);
    return timed(ctx, [&] { return plain_range<PowerKind>(plan, d_bytes, g, 0, width, nullptr, d_power); });
}

extern "C" int sp_plan_power_to_db(sp_plan *plan, const double *d_power, size_t count, double *d_db)
{
    if (!plan) return SP_ERR_INVALID_ARG;
    sp_context *ctx = plan->ctx;
    if (count && (!d_power || !d_db)) return fail(ctx, SP_ERR_INVALID_ARG, "d_power and d_db must not be null");
    if ((((uintptr_t)d_power | (uintptr_t)d_db) & 7) != 0) return fail(ctx, SP_ERR_INVALID_ARG, "d_power and d_db must be 8-byte aligned");
    if (!count) return SP_OK;
    SP_HIP(ctx, hipSetDevice(ctx->device));
    return timed(ctx, [&] { return power_to_db(plan, d_power, count, d_db); });
}

// A request kind of download_chunks - a packed sparse upload where stride > n, chunks of frames where the request is large - whose
// plane comes back chunk by chunk: rows [x0, x1) of it are one contiguous copy.
extern "C" int sp_render_power(sp_context *ctx, const sp_request *req, const uint8_t *bytes, size_t nbytes, int32_t width, int32_t db, double *power)
{
    if (!ctx) return SP_ERR_INVALID_ARG;
    sp_plan *plan = nullptr;
    int rc = host_request(
        ctx, req, bytes, nbytes, width,
        [&] {
            return width > 0 && (!power || ((uintptr_t)power & 7) != 0)
                       ? fail(ctx, SP_ERR_INVALID_ARG, "power must be an 8-byte aligned array of width * n doubles")
                       : (int)SP_OK;
        },
        [&] { return check_plain<PowerKind>(ctx, req->detector, spfmt::describe(req->format), req->n, bytes, nbytes, width); }, &plan);
    if (rc) return rc;

    const size_t n = (size_t)req->n, plane_bytes = sizeof(double) * (size_t)width * n;
    rc = ctx->power_plane.reserve(plane_bytes + 16);
    if (rc) return fail(ctx, rc, "sp_render_power: out of memory");
    double *const d_plane = (double *)ctx->power_plane.p;
    HostFeed feed{"sp_render_power", bytes, spgeo::geometry(plan->fmt, req->n, nbytes, width), 1, plan_plain_frames(plan), true, plane_bytes, true, nullptr};
    return download_chunks(
        ctx, plan->fmt, feed,
        [&](int32_t x0, int32_t x1, bool, bool, const uint8_t *d_in, const PackedSource *src) {
            int r = plain_range<PowerKind>(plan, d_in, feed.g, x0, x1, src, d_plane);
            if (!r && db && x1 > x0) r = power_to_db(plan, d_plane + (size_t)x0 * n, (size_t)(x1 - x0) * n, d_plane + (size_t)x0 * n);
            return r;
        },
        [&](int32_t x0, int32_t x1, hipStream_t out_s) {
            const size_t row0 = (size_t)x0 * n;
            return hipMemcpyAsync(power + row0, d_plane + row0, sizeof(double) * (size_t)(x1 - x0) * n, hipMemcpyDeviceToHost, out_s);
        },
        [] { return hipSuccess; });
}

// ------------------------------------------------------------------------------------------------- plane consumers (mean, band power, track)

// A plane consumer makes its reply from the f64 power plane without holding the plane whole: the power request's frame loop renders the
// frames block by block into a window of the context and the kind's launch runs behind each block.  A kind is a struct of the caller's
// arguments - its outputs are device arrays, or the host's arrays in what the host-fed entry point is given - with
//   check(p)                              what it refuses of them before the device is touched
//   empty(p)                              a request that writes nothing: SP_OK after the checks, before the device is touched
//   clear(p), finish(p)                   what it queues in front of the first block and behind the last one
//   consume(p, d_plane, frames, x_base)   its launch on the `frames` frames of the frame-major plane at d_plane, the request's frames
//                                         from x_base on, followed by SP_HIP(ctx, hipGetLastError())
// and for the host-fed form kRender (the entry point's name), small_bytes(p) of the context's render_small, on_device(p, small) - the
// kind with its outputs there, null where the host's are - and tail(plan, p, db, host, e): the dB conversion and the copies back into
// the kind `host`, a failed copy's error left in e.  Three drivers carry a kind out: plane_resident (sp_power_*), plane_capture
// (sp_plan_execute_*) and plane_render (sp_render_*); kBadPlane is how sp_power_*'s refusal of its d_power ends.  (The kinds stand in
// unnamed namespaces: their member functions are no symbols of the library.)
struct PlaneShape {
    sp_context *ctx;
    int n;           // rows of a frame
    int32_t width;   // frames of the whole request
};

// The default size of the window a request's plane passes through, block of frames by block of frames.
constexpr size_t kPlaneWindowDefault = (size_t)64 << 20;

extern "C" int sp_context_set_mean_window(sp_context *ctx, size_t bytes)
{
    if (!ctx) return SP_ERR_INVALID_ARG;
    ctx->mean_window_bytes = bytes;
    return SP_OK;
}

// (tests) k_mean_accumulate's grid for `frames` frames of n rows on a part with cu_count CUs, from the function its launch calls.
extern "C" int sp_debug_mean_launch(int32_t n, int64_t frames, int32_t cu_count, int64_t *out, size_t capacity, size_t *used)
{
    if (n < 1 || frames < 1 || cu_count < 1 || !used) return SP_ERR_INVALID_ARG;
    long long shape[3];
    spk::mean_launch_shape(n, frames, cu_count, shape);
    const int64_t v[] = {shape[0], shape[1], shape[2]};
    *used = sizeof v / sizeof v[0];
    if (*used > capacity || !out) return SP_ERR_INVALID_ARG;
    memcpy(out, v, sizeof v);
    return SP_OK;
}

// the frames of a plane of n rows that one block of the window holds: at least one
static int32_t plane_block_frames(const sp_context *ctx, int n, int32_t width)
{
    const size_t window = ctx->mean_window_bytes ? ctx->mean_window_bytes : kPlaneWindowDefault;
    size_t frames = window / (sizeof(double) * (size_t)n);
    if (frames < 1) frames = 1;
    return frames < (size_t)width ? (int32_t)frames : width;
}

// The frames [x_begin, x_end) of a plane consumer's request (`src`: as for plan_execute_range): rendered block by block into the
// context's window by the power request's frame loop, with the kind's launch on the block's frames queued behind each block.  (The
// frame loop puts frame x at base + x * n: the window stands in for the block's part of a whole plane.)
template <typename Kind>
static int plane_blocks(sp_plan *plan, const void *d_bytes, const spgeo::Geometry &g, int32_t x_begin, int32_t x_end, const PackedSource *src,
                        const PlaneShape &p, const Kind &k)
{
    sp_context *ctx = plan->ctx;
    if (x_end <= x_begin) return SP_OK;
    const int n = p.n;
    const int32_t block = plane_block_frames(ctx, n, g.width);   // (of the whole request: the window does not grow from chunk to chunk)
    int rc = ctx->plane_window.reserve(sizeof(double) * (size_t)block * (size_t)n);
    if (rc) return fail(ctx, rc, "mean window: out of device memory");
    double *const d_win = (double *)ctx->plane_window.p;
    for (int32_t x0 = x_begin; x0 < x_end && !rc; x0 += block) {
        const int32_t x1 = x_end - x0 > block ? x0 + block : x_end;
        double *const base = (double *)((uintptr_t)d_win - sizeof(double) * (size_t)x0 * (size_t)n);
        rc = plain_range<PowerKind>(plan, d_bytes, g, x0, x1, src, base);
        if (!rc) rc = k.consume(p, d_win, x1 - x0, x0);
    }
    return rc;
}

// sp_power_*: the plane is resident, `width` frames of n rows at d_power.  `who`: the entry point, for its error texts.
template <typename Kind>
static int plane_resident(sp_context *ctx, const char *who, const double *d_power, int32_t n, int32_t width, const Kind &k)
{
    if (!ctx) return SP_ERR_INVALID_ARG;
    if (n < 1 || width < 0) return fail(ctx, SP_ERR_INVALID_ARG, std::string(who) + ": n >= 1 and width >= 0 are required");
    const PlaneShape p{ctx, n, width};
    const int rc = k.check(p);
    if (rc) return rc;
    if (k.empty(p)) return SP_OK;
    if ((width > 0 && !d_power) || ((uintptr_t)d_power & 7) != 0) return fail(ctx, SP_ERR_INVALID_ARG, std::string(who) + Kind::kBadPlane);
    SP_HIP(ctx, hipSetDevice(ctx->device));
    return timed(ctx, [&] {
        int r = k.clear(p);
        if (!r) r = k.consume(p, d_power, width, 0);
        return r ? r : k.finish(p);
    });
}

// sp_plan_execute_*: the capture is resident and the plane passes through the window.
template <typename Kind>
static int plane_capture(sp_plan *plan, const void *d_bytes, size_t nbytes, int32_t width, const Kind &k)
{
    if (!plan) return SP_ERR_INVALID_ARG;
    sp_context *ctx = plan->ctx;
    const PlaneShape p{ctx, plan->req.n, width};
    int rc = check_plain<PowerKind>(ctx, plan->req.detector, plan->fmt, plan->req.n, d_bytes, nbytes, width);
    if (!rc) rc = k.check(p);
    if (rc) return rc;
    if (k.empty(p)) return SP_OK;
    SP_HIP(ctx, hipSetDevice(ctx->device));
    const spgeo::Geometry g = spgeo::geometry(plan->fmt, plan->req.n, nbytes, width);
    return timed(ctx, [&] {
        int r = k.clear(p);
        if (!r) r = plane_blocks(plan, d_bytes, g, 0, width, nullptr, p, k);
        return r ? r : k.finish(p);
    });
}

// sp_render_*: a request kind of render_result - a packed sparse upload where stride > n, chunks of frames where the request is large -
// whose reply accumulates or fills on the device over the chunks and comes back behind the last one.
template <typename Kind>
static int plane_render(sp_context *ctx, const sp_request *req, const uint8_t *bytes, size_t nbytes, int32_t width, int32_t db, const Kind &host)
{
    if (!ctx) return SP_ERR_INVALID_ARG;
    sp_plan *plan = nullptr;
    int rc = host_request(
        ctx, req, bytes, nbytes, width, [&] { return host.check(PlaneShape{ctx, req->n, width}); },
        [&] { return check_plain<PowerKind>(ctx, req->detector, spfmt::describe(req->format), req->n, bytes, nbytes, width); }, &plan);
    if (rc) return rc;
    const PlaneShape p{ctx, req->n, width};
    if (host.empty(p)) return SP_OK;

    rc = ctx->render_small.reserve(host.small_bytes(p) + 16);
    if (rc) return fail(ctx, rc, std::string(Kind::kRender) + ": out of memory");
    const Kind k = host.on_device(p, ctx->render_small.p);
    HostFeed feed{Kind::kRender, bytes, spgeo::geometry(plan->fmt, req->n, nbytes, width), 1, plan_plain_frames(plan), true, 0, false, nullptr};
    return render_result(
        ctx, plan->fmt, feed, [&] { return k.clear(p); },
        [&](int32_t x0, int32_t x1, bool, bool, const uint8_t *d_in, const PackedSource *src) {
            return plane_blocks(plan, d_in, feed.g, x0, x1, src, p, k);
        },
        [&](bool cleared, hipError_t &e) {
            int r = cleared ? (int)SP_OK : k.clear(p);   // (no chunk at all: the reply of no frames)
            if (!r) r = k.finish(p);
            return r ? r : k.tail(plan, p, db, host, e);
        });
}

// ------------------------------------------------------------------------------------------------- exact mean-power trace

extern "C" const char *sp_plan_mean_kernel_name_for(const sp_plan *plan, size_t, int32_t)
{
    return plain_kernel_name(plan, "frames_power+mean", "scratch_power+mean");
}

extern "C" int sp_debug_exact_sum(const double *values, size_t count, double *sum)
{
    if (!sum || (count && !values)) return SP_ERR_INVALID_ARG;
    std::vector<uint64_t> bits(count);
    if (count) memcpy(bits.data(), values, count * sizeof(double));
    uint64_t r = 0;
    if (!spx::exact_sum_bits(bits.data(), count, &r)) return SP_ERR_INVALID_ARG;
    memcpy(sum, &r, sizeof r);
    return SP_OK;
}

namespace {
// The exact sums accumulate in the context's workspace, (66 + 2) * 8 * n bytes that clear() zeroes on the stream, and finish() makes the
// n means of them.  No request is empty: one of no frames still gives n NaNs.
struct MeanKind {
    static constexpr const char *kRender = "sp_render_mean";
    static constexpr const char *kBadPlane = ": d_power and d_mean must be 8-byte aligned device pointers";
    double *out;           // n doubles
    const char *refusal;   // of a null or misaligned `out`: every entry point has its own sentence

    int check(const PlaneShape &p) const { return !out || ((uintptr_t)out & 7) != 0 ? fail(p.ctx, SP_ERR_INVALID_ARG, refusal) : (int)SP_OK; }
    bool empty(const PlaneShape &) const { return false; }
    int clear(const PlaneShape &p) const
    {
        const size_t bytes = (size_t)spx::kSlots * sizeof(unsigned long long) * (size_t)p.n;
        const int rc = p.ctx->mean_ws.reserve(bytes);
        if (rc) return fail(p.ctx, rc, "mean workspace: out of device memory");
        SP_HIP(p.ctx, hipMemsetAsync(p.ctx->mean_ws.p, 0, bytes, p.ctx->stream));
        return SP_OK;
    }
    int consume(const PlaneShape &p, const double *d_plane, long long frames, long long) const
    {
        if (frames <= 0) return SP_OK;
        spk::launch_mean_accumulate(d_plane, p.n, frames, (unsigned long long *)p.ctx->mean_ws.p, p.ctx->cu_count, p.ctx->stream);
        SP_HIP(p.ctx, hipGetLastError());
        return SP_OK;
    }
    int finish(const PlaneShape &p) const
    {
        spk::launch_mean_finish((const unsigned long long *)p.ctx->mean_ws.p, p.n, p.width, out, p.ctx->stream);
        SP_HIP(p.ctx, hipGetLastError());
        return SP_OK;
    }
    size_t small_bytes(const PlaneShape &p) const { return (size_t)p.n * sizeof(double); }
    MeanKind on_device(const PlaneShape &, void *small) const { return {(double *)small, refusal}; }
    int tail(sp_plan *plan, const PlaneShape &p, int32_t db, const MeanKind &host, hipError_t &e) const
    {
        const int r = db ? power_to_db(plan, out, (size_t)p.n, out) : (int)SP_OK;
        if (!r) e = hipMemcpyAsync(host.out, out, (size_t)p.n * sizeof(double), hipMemcpyDeviceToHost, p.ctx->stream);
        return r;
    }
};
}  // namespace

extern "C" int sp_power_mean(sp_context *ctx, const double *d_power, int32_t n, int32_t width, double *d_mean)
{
    const MeanKind k{d_mean, "sp_power_mean: d_power and d_mean must be 8-byte aligned device pointers"};
    return plane_resident(ctx, "sp_power_mean", d_power, n, width, k);
}

extern "C" int sp_plan_execute_mean(sp_plan *plan, const void *d_bytes, size_t nbytes, int32_t width, double *d_mean)
{
    return plane_capture(plan, d_bytes, nbytes, width, MeanKind{d_mean, "d_mean must be an 8-byte aligned array of n doubles"});
}

extern "C" int sp_render_mean(sp_context *ctx, const sp_request *req, const uint8_t *bytes, size_t nbytes, int32_t width, int32_t db, double *mean)
{
    return plane_render(ctx, req, bytes, nbytes, width, db, MeanKind{mean, "mean must be an 8-byte aligned array of n doubles"});
}

// ------------------------------------------------------------------------------------------------- averaged spectrogram

extern "C" const char *sp_plan_blockmean_kernel_name_for(const sp_plan *plan, size_t, int32_t)
{
    return plain_kernel_name(plan, "frames_power+blockmean", "scratch_power+blockmean");
}

extern "C" int32_t sp_blockmean_columns(int32_t width, int32_t group) { return (int32_t)spbm::columns(width, group); }

extern "C" int sp_context_set_blockmean_direct_max(sp_context *ctx, int32_t frames)
{
    if (!ctx) return SP_ERR_INVALID_ARG;
    if (frames < 0) return fail(ctx, SP_ERR_INVALID_ARG, "sp_context_set_blockmean_direct_max: frames >= 0 is required");
    ctx->blockmean_direct_max = frames;
    return SP_OK;
}

extern "C" int sp_debug_blockmean(const double *values, int32_t n, int32_t width, int32_t group, double *out)
{
    if (n < 1 || width < 0 || group < 1 || (width > 0 && (!values || !out))) return SP_ERR_INVALID_ARG;
    const int64_t columns = spbm::columns(width, group);
    std::vector<uint64_t> bits((size_t)width * (size_t)n);
    if (!bits.empty()) memcpy(bits.data(), values, bits.size() * sizeof(uint64_t));
    for (uint64_t b : bits)
        if ((b >> 63) && (b & 0x7fffffffffffffffull) <= spx::kInfBits) return SP_ERR_INVALID_ARG;   // (the accumulator has no subtraction)
    for (int64_t c = 0; c < columns; c++) {
        const int64_t first = c * group, end = first + group < width ? first + group : width;
        for (int32_t y = 0; y < n; y++) {
            spx::Accumulator acc;
            for (int64_t x = first; x < end; x++) acc.add(bits[(size_t)x * (size_t)n + (size_t)y]);
            const uint64_t r = acc.finish();
            double sum;
            memcpy(&sum, &r, sizeof sum);
            out[(size_t)c * (size_t)n + (size_t)y] = sum / (double)(end - first);
        }
    }
    return SP_OK;
}

extern "C" int sp_debug_blockmean_split(int64_t x_base, int64_t frames, int32_t width, int32_t group, int32_t direct_max, int64_t *out,
                                        size_t capacity, size_t *used)
{
    if (x_base < 0 || frames < 0 || width < 0 || x_base + frames > width || group < 1 || direct_max < 0 || !used) return SP_ERR_INVALID_ARG;
    const spbm::Split s = spbm::split(x_base, frames, width, group, direct_max ? direct_max : SP_BLOCKMEAN_DIRECT_FRAMES);
    const int64_t v[] = {s.head, s.body, s.tail, s.body_column, s.body_columns, s.direct};
    *used = sizeof v / sizeof v[0];
    if (*used > capacity || !out) return SP_ERR_INVALID_ARG;
    memcpy(out, v, sizeof v);
    return SP_OK;
}

// (tests) k_blockmean's grid for the whole columns of `frames` frames of n rows on a part with cu_count CUs, from the function its launch
// calls.
extern "C" int sp_debug_blockmean_launch(int32_t n, int64_t frames, int32_t group, int32_t cu_count, int64_t *out, size_t capacity, size_t *used)
{
    if (n < 1 || frames < 1 || group < 1 || cu_count < 1 || !used) return SP_ERR_INVALID_ARG;
    long long shape[3];
    spk::blockmean_launch_shape(n, frames, group, cu_count, shape);
    const int64_t v[] = {shape[0], shape[1], shape[2]};
    *used = sizeof v / sizeof v[0];
    if (*used > capacity || !out) return SP_ERR_INVALID_ARG;
    memcpy(out, v, sizeof v);
    return SP_OK;
}

extern "C" int sp_debug_gray_index(double block_norm, double gain, double range, int32_t lut_len, const double *values, size_t count,
                                   uint8_t *out)
{
    if (lut_len < 2 || lut_len > 256 || (count && (!values || !out))) return SP_ERR_INVALID_ARG;
    const sphost::Thresholds th = sphost::build_thresholds(sphost::PixelMath(block_norm, gain, range, lut_len), lut_len);
    std::vector<uint64_t> edges((size_t)lut_len);
    memcpy(edges.data(), th.gray_edge.data(), edges.size() * sizeof(uint64_t));
    for (size_t k = 0; k < count; k++) {
        uint64_t b;
        memcpy(&b, values + k, sizeof b);
        out[k] = (uint8_t)spbm::gray_index(edges.data(), lut_len, b);
    }
    return SP_OK;
}

namespace {
// The columns are made as their frames arrive (sp_blockmean_core.h): whole columns of a run by k_blockmean where the group is small,
// everything else - a column that straddles two runs, a group beyond direct_max - through the mean's own launches into the context's
// mean_ws, cleared where a column begins and finished where it ends.  mean_ws is the mean's workspace too: every request that uses it
// clears it on the stream before it adds, and a context's requests run in order on one stream, so neither sees the other's cells.  The
// frame the next run must begin with is the context's: the drivers hand a kind over by const reference.
struct BlockMeanKind {
    static constexpr const char *kRender = "sp_render_blockmean";
    static constexpr const char *kBadPlane = ": d_power and d_out must be 8-byte aligned device pointers";
    int32_t group;
    double *out;           // columns * n doubles
    const char *refusal;   // of a null or misaligned `out`: every entry point has its own sentence

    int64_t columns(const PlaneShape &p) const { return spbm::columns(p.width, group); }
    size_t total(const PlaneShape &p) const { return (size_t)columns(p) * (size_t)p.n; }
    int check(const PlaneShape &p) const
    {
        if (columns(p) > 0 && (!out || ((uintptr_t)out & 7) != 0)) return fail(p.ctx, SP_ERR_INVALID_ARG, refusal);
        if (group < 1) return fail(p.ctx, SP_ERR_INVALID_ARG, "group >= 1 is required");
        return SP_OK;
    }
    bool empty(const PlaneShape &p) const { return p.width == 0; }
    size_t ws_bytes(const PlaneShape &p) const { return (size_t)spx::kSlots * sizeof(unsigned long long) * (size_t)p.n; }
    int clear(const PlaneShape &p) const
    {
        const int rc = p.ctx->mean_ws.reserve(ws_bytes(p));
        if (rc) return fail(p.ctx, rc, "mean workspace: out of device memory");
        p.ctx->blockmean_next = 0;
        return SP_OK;
    }
    // `frames` > 0 frames from x0 on, all of one column, at `src`: the column is opened where x0 begins it and closed where they end it
    int carry(const PlaneShape &p, const double *src, int64_t x0, int64_t frames) const
    {
        sp_context *ctx = p.ctx;
        unsigned long long *const ws = (unsigned long long *)ctx->mean_ws.p;
        const int64_t c = x0 / group, first = c * (int64_t)group, end = first + group < p.width ? first + group : p.width;
        if (x0 == first) SP_HIP(ctx, hipMemsetAsync(ws, 0, ws_bytes(p), ctx->stream));
        spk::launch_mean_accumulate(src, p.n, frames, ws, ctx->cu_count, ctx->stream);
        SP_HIP(ctx, hipGetLastError());
        if (x0 + frames == end) {
            spk::launch_mean_finish(ws, p.n, (int)(end - first), out + (size_t)c * (size_t)p.n, ctx->stream);
            SP_HIP(ctx, hipGetLastError());
        }
        return SP_OK;
    }
    int consume(const PlaneShape &p, const double *d_plane, long long frames, long long x_base) const
    {
        sp_context *ctx = p.ctx;
        if (frames <= 0) return SP_OK;
        if (x_base != ctx->blockmean_next || x_base + frames > p.width)
            return fail(ctx, SP_ERR_INVALID_ARG, "block mean: a run of frames that does not continue the one before it");
        const int64_t direct_max = ctx->blockmean_direct_max ? ctx->blockmean_direct_max : SP_BLOCKMEAN_DIRECT_FRAMES;
        const spbm::Split s = spbm::split(x_base, frames, p.width, group, direct_max);
        const size_t n = (size_t)p.n;
        int rc = SP_OK;
        if (s.head) rc = carry(p, d_plane, x_base, s.head);
        const double *const body = d_plane + (size_t)s.head * n;
        const int64_t body_x = x_base + s.head;
        if (!rc && s.body) {
            if (s.direct) {
                spk::launch_blockmean(body, p.n, s.body, group, out + (size_t)s.body_column * n, ctx->cu_count, ctx->stream);
                SP_HIP(ctx, hipGetLastError());
            } else {
                for (int64_t k = 0; k < s.body_columns && !rc; k++) {
                    const int64_t at = k * (int64_t)group, count = s.body - at < group ? s.body - at : group;
                    rc = carry(p, body + (size_t)at * n, body_x + at, count);
                }
            }
        }
        if (!rc && s.tail) rc = carry(p, body + (size_t)s.body * n, body_x + s.body, s.tail);
        if (!rc) ctx->blockmean_next = x_base + frames;
        return rc;
    }
    int finish(const PlaneShape &p) const
    {
        // (every run that reaches `width` has closed the last column, the short one too: nothing is left to finish)
        return p.ctx->blockmean_next == p.width ? (int)SP_OK : fail(p.ctx, SP_ERR_INVALID_ARG, "block mean: the request's frames did not all arrive");
    }
    size_t small_bytes(const PlaneShape &p) const { return total(p) * sizeof(double); }
    BlockMeanKind on_device(const PlaneShape &, void *small) const { return {group, (double *)small, refusal}; }
    int tail(sp_plan *plan, const PlaneShape &p, int32_t db, const BlockMeanKind &host, hipError_t &e) const
    {
        const int r = db ? power_to_db(plan, out, total(p), out) : (int)SP_OK;
        if (!r) e = hipMemcpyAsync(host.out, out, total(p) * sizeof(double), hipMemcpyDeviceToHost, p.ctx->stream);
        return r;
    }
};
}  // namespace

extern "C" int sp_power_blockmean(sp_context *ctx, const double *d_power, int32_t n, int32_t width, int32_t group, double *d_out)
{
    const BlockMeanKind k{group, d_out, "sp_power_blockmean: d_power and d_out must be 8-byte aligned device pointers"};
    return plane_resident(ctx, "sp_power_blockmean", d_power, n, width, k);
}

extern "C" int sp_plan_execute_blockmean(sp_plan *plan, const void *d_bytes, size_t nbytes, int32_t width, int32_t group, double *d_out)
{
    const BlockMeanKind k{group, d_out, "d_out must be an 8-byte aligned array of columns * n doubles"};
    if (plan && width >= 0) {   // (the output's and the group's refusals come before the plan's)
        const int rc = k.check(PlaneShape{plan->ctx, plan->req.n, width});
        if (rc) return rc;
    }
    return plane_capture(plan, d_bytes, nbytes, width, k);
}

extern "C" int sp_render_blockmean(sp_context *ctx, const sp_request *req, const uint8_t *bytes, size_t nbytes, int32_t width, int32_t group,
                                   int32_t db, double *out)
{
    return plane_render(ctx, req, bytes, nbytes, width, db, BlockMeanKind{group, out, "out must be an 8-byte aligned array of columns * n doubles"});
}

extern "C" int sp_plan_power_to_index(sp_plan *plan, const double *d_power, int32_t width, uint8_t *d_index)
{
    if (!plan) return SP_ERR_INVALID_ARG;
    sp_context *ctx = plan->ctx;
    if (plan->req.lut_len > 256) return fail(ctx, SP_ERR_UNSUPPORTED, "sp_plan_power_to_index: a colour map of more than 256 entries has no index byte");
    if (width < 0) return fail(ctx, SP_ERR_INVALID_ARG, "width < 0");
    if (width == 0) return SP_OK;
    if (!d_power || ((uintptr_t)d_power & 7) != 0 || !d_index)
        return fail(ctx, SP_ERR_INVALID_ARG, "sp_plan_power_to_index: d_power must be an 8-byte aligned device pointer and d_index a device pointer");
    SP_HIP(ctx, hipSetDevice(ctx->device));
    return timed(ctx, [&] {
        const int rc = spk::launch_power_to_index(d_power, plan->req.n, width, plan->req.waterfall != 0, plan->d_gray_edge, plan->req.lut_len,
                                                  d_index, ctx->stream);
        if (rc) return fail(ctx, rc, "sp_plan_power_to_index: n is beyond what one grid covers");
        SP_HIP(ctx, hipGetLastError());
        return (int)SP_OK;
    });
}

// ------------------------------------------------------------------------------------------------- exact variance and spectral-kurtosis traces

extern "C" const char *sp_plan_variance_kernel_name_for(const sp_plan *plan, size_t, int32_t)
{
    return plain_kernel_name(plan, "frames_power+variance", "scratch_power+variance");
}

extern "C" int sp_debug_variance_sums(const double *values, size_t count, double *out3)
{
    if (!out3 || (count && !values) || (count >> 31)) return SP_ERR_INVALID_ARG;   // (a request has fewer than 2^31 frames)
    std::vector<uint64_t> bits(count);
    if (count) memcpy(bits.data(), values, count * sizeof(double));
    uint64_t r[3] = {};
    if (!spv::variance_sums_bits(bits.data(), count, r)) return SP_ERR_INVALID_ARG;
    memcpy(out3, r, sizeof r);
    return SP_OK;
}

// (tests) k_variance_accumulate's grid for `frames` frames of n rows on a part with cu_count CUs, from the function its launch calls.
extern "C" int sp_debug_variance_launch(int32_t n, int64_t frames, int32_t cu_count, int64_t *out, size_t capacity, size_t *used)
{
    if (n < 1 || frames < 1 || cu_count < 1 || !used) return SP_ERR_INVALID_ARG;
    long long shape[3];
    spk::variance_launch_shape(n, frames, cu_count, shape);
    const int64_t v[] = {shape[0], shape[1], shape[2]};
    *used = sizeof v / sizeof v[0];
    if (*used > capacity || !out) return SP_ERR_INVALID_ARG;
    memcpy(out, v, sizeof v);
    return SP_OK;
}

namespace {
// The sums and the sums of squares accumulate in a workspace of the context of their own, (66 + 132 + 2) * 8 * n bytes that clear()
// zeroes on the stream, and finish() makes the 3 * n results of them.  No request is empty: one of no frames still gives 3 * n zeros.
struct VarianceKind {
    static constexpr const char *kRender = "sp_render_variance";
    static constexpr const char *kBadPlane = ": d_power and d_out must be 8-byte aligned device pointers";
    double *out;           // 3 * n doubles
    const char *refusal;   // of a null or misaligned `out`: every entry point has its own sentence

    int check(const PlaneShape &p) const
    {
        if (p.n > SP_MAX_N) return fail(p.ctx, SP_ERR_INVALID_ARG, "variance traces need n <= SP_MAX_N");
        return !out || ((uintptr_t)out & 7) != 0 ? fail(p.ctx, SP_ERR_INVALID_ARG, refusal) : (int)SP_OK;
    }
    bool empty(const PlaneShape &) const { return false; }
    int clear(const PlaneShape &p) const
    {
        const size_t bytes = (size_t)spv::kSlots * sizeof(unsigned long long) * (size_t)p.n;
        const int rc = p.ctx->variance_ws.reserve(bytes);
        if (rc) return fail(p.ctx, rc, "variance workspace: out of device memory");
        SP_HIP(p.ctx, hipMemsetAsync(p.ctx->variance_ws.p, 0, bytes, p.ctx->stream));
        return SP_OK;
    }
    int consume(const PlaneShape &p, const double *d_plane, long long frames, long long) const
    {
        if (frames <= 0) return SP_OK;
        spk::launch_variance_accumulate(d_plane, p.n, frames, (unsigned long long *)p.ctx->variance_ws.p, p.ctx->cu_count, p.ctx->stream);
        SP_HIP(p.ctx, hipGetLastError());
        return SP_OK;
    }
    int finish(const PlaneShape &p) const
    {
        spk::launch_variance_finish((const unsigned long long *)p.ctx->variance_ws.p, p.n, p.width, out, p.ctx->stream);
        SP_HIP(p.ctx, hipGetLastError());
        return SP_OK;
    }
    size_t small_bytes(const PlaneShape &p) const { return 3 * (size_t)p.n * sizeof(double); }
    VarianceKind on_device(const PlaneShape &, void *small) const { return {(double *)small, refusal}; }
    // (no dB form: a sum of squares has none)
    int tail(sp_plan *, const PlaneShape &p, int32_t, const VarianceKind &host, hipError_t &e) const
    {
        e = hipMemcpyAsync(host.out, out, 3 * (size_t)p.n * sizeof(double), hipMemcpyDeviceToHost, p.ctx->stream);
        return SP_OK;
    }
};
}  // namespace

extern "C" int sp_power_variance(sp_context *ctx, const double *d_power, int32_t n, int32_t width, double *d_out)
{
    const VarianceKind k{d_out, "sp_power_variance: d_power and d_out must be 8-byte aligned device pointers"};
    return plane_resident(ctx, "sp_power_variance", d_power, n, width, k);
}

extern "C" int sp_plan_execute_variance(sp_plan *plan, const void *d_bytes, size_t nbytes, int32_t width, double *d_out)
{
    return plane_capture(plan, d_bytes, nbytes, width, VarianceKind{d_out, "d_out must be an 8-byte aligned array of 3 * n doubles"});
}

extern "C" int sp_render_variance(sp_context *ctx, const sp_request *req, const uint8_t *bytes, size_t nbytes, int32_t width, double *out)
{
    return plane_render(ctx, req, bytes, nbytes, width, 0, VarianceKind{out, "out must be an 8-byte aligned array of 3 * n doubles"});
}

// ------------------------------------------------------------------------------------------------- exact band-power series

extern "C" const char *sp_plan_bandpower_kernel_name_for(const sp_plan *plan, size_t, int32_t)
{
    return plain_kernel_name(plan, "frames_power+bands", "scratch_power+bands");
}

namespace {
// Every block's launch writes its columns of every band's series, `width` doubles apart: nothing to clear (every column is written
// once) and nothing to finish.
struct BandKind {
    static constexpr const char *kRender = "sp_render_bandpower";
    static constexpr const char *kBadPlane = ": d_power must be an 8-byte aligned device pointer";
    const int32_t *bands;
    int32_t count;
    double *out;   // count * width doubles

    int check(const PlaneShape &p) const
    {
        if (const char *why = spgeo::check_bands(p.n, bands, count)) return fail(p.ctx, SP_ERR_INVALID_ARG, why);
        if (count > 0 && p.width > 0 && (!out || ((uintptr_t)out & 7) != 0))
            return fail(p.ctx, SP_ERR_INVALID_ARG, "the band series must be an 8-byte aligned array of count * width doubles");
        return SP_OK;
    }
    bool empty(const PlaneShape &p) const { return p.width == 0 || count == 0; }
    int clear(const PlaneShape &) const { return SP_OK; }
    int consume(const PlaneShape &p, const double *d_plane, long long frames, long long x_base) const
    {
        if (frames <= 0 || count <= 0) return SP_OK;
        spk::launch_band_sum(d_plane, p.n, frames, bands, count, 0, out, p.width, x_base, p.ctx->stream);
        SP_HIP(p.ctx, hipGetLastError());
        return SP_OK;
    }
    int finish(const PlaneShape &) const { return SP_OK; }
    size_t total(const PlaneShape &p) const { return (size_t)count * (size_t)p.width; }
    size_t small_bytes(const PlaneShape &p) const { return total(p) * sizeof(double); }
    BandKind on_device(const PlaneShape &, void *small) const { return {bands, count, (double *)small}; }
    int tail(sp_plan *plan, const PlaneShape &p, int32_t db, const BandKind &host, hipError_t &e) const
    {
        const int r = db ? power_to_db(plan, out, total(p), out) : (int)SP_OK;
        if (!r) e = hipMemcpyAsync(host.out, out, total(p) * sizeof(double), hipMemcpyDeviceToHost, p.ctx->stream);
        return r;
    }
};
}  // namespace

extern "C" int sp_power_bands(sp_context *ctx, const double *d_power, int32_t n, int32_t width, const int32_t *bands, int32_t count,
                              double *d_band)
{
    return plane_resident(ctx, "sp_power_bands", d_power, n, width, BandKind{bands, count, d_band});
}

extern "C" int sp_plan_execute_bandpower(sp_plan *plan, const void *d_bytes, size_t nbytes, int32_t width, const int32_t *bands, int32_t count,
                                         double *d_band)
{
    return plane_capture(plan, d_bytes, nbytes, width, BandKind{bands, count, d_band});
}

extern "C" int sp_render_bandpower(sp_context *ctx, const sp_request *req, const uint8_t *bytes, size_t nbytes, int32_t width, const int32_t *bands,
                                   int32_t count, int32_t db, double *band)
{
    return plane_render(ctx, req, bytes, nbytes, width, db, BandKind{bands, count, band});
}

// ------------------------------------------------------------------------------------------------- exact spectral moments

extern "C" const char *sp_plan_moments_kernel_name_for(const sp_plan *plan, size_t, int32_t)
{
    return plain_kernel_name(plan, "frames_power+moments", "scratch_power+moments");
}

extern "C" int sp_debug_moment_sum(const double *values, size_t count, int32_t order, double *out)
{
    if (!out || (count && !values)) return SP_ERR_INVALID_ARG;
    if (count > spm::kMaxRows) return SP_ERR_INVALID_ARG;   // (before the copy: a weight stays below 2^40)
    std::vector<uint64_t> bits(count);
    if (count) memcpy(bits.data(), values, count * sizeof(double));
    uint64_t r[spm::kMaxOrder + 1] = {};
    if (!spm::moment_sum_bits(bits.data(), count, order, r)) return SP_ERR_INVALID_ARG;
    memcpy(out, r, (size_t)(order + 1) * sizeof(uint64_t));
    return SP_OK;
}

namespace {
// As BandKind with order + 1 series per band, moment-major: every block's launch writes its columns of every series, nothing to clear
// and nothing to finish.  The dB form converts m[0] alone.
struct MomentKind {
    static constexpr const char *kRender = "sp_render_moments";
    static constexpr const char *kBadPlane = BandKind::kBadPlane;
    const int32_t *bands;
    int32_t count;
    int32_t order;
    double *out;   // (order + 1) * count * width doubles

    int check(const PlaneShape &p) const
    {
        if (order < 0 || order > spm::kMaxOrder) return fail(p.ctx, SP_ERR_INVALID_ARG, "a moment order of 0, 1 or 2 is required");
        if (p.n > SP_MAX_N) return fail(p.ctx, SP_ERR_INVALID_ARG, "moments: n <= SP_MAX_N is required");
        if (const char *why = spgeo::check_bands(p.n, bands, count)) return fail(p.ctx, SP_ERR_INVALID_ARG, why);
        if (count > 0 && p.width > 0 && (!out || ((uintptr_t)out & 7) != 0))
            return fail(p.ctx, SP_ERR_INVALID_ARG, "the moment series must be an 8-byte aligned array of (order + 1) * count * width doubles");
        return SP_OK;
    }
    bool empty(const PlaneShape &p) const { return p.width == 0 || count == 0; }
    int clear(const PlaneShape &) const { return SP_OK; }
    int consume(const PlaneShape &p, const double *d_plane, long long frames, long long x_base) const
    {
        if (frames <= 0 || count <= 0) return SP_OK;
        spk::launch_band_sum(d_plane, p.n, frames, bands, count, order, out, p.width, x_base, p.ctx->stream);   // (order 0: the band sum)
        SP_HIP(p.ctx, hipGetLastError());
        return SP_OK;
    }
    int finish(const PlaneShape &) const { return SP_OK; }
    size_t series(const PlaneShape &p) const { return (size_t)count * (size_t)p.width; }   // the values of one moment
    size_t total(const PlaneShape &p) const { return (size_t)(order + 1) * series(p); }
    size_t small_bytes(const PlaneShape &p) const { return total(p) * sizeof(double); }
    MomentKind on_device(const PlaneShape &, void *small) const { return {bands, count, order, (double *)small}; }
    int tail(sp_plan *plan, const PlaneShape &p, int32_t db, const MomentKind &host, hipError_t &e) const
    {
        const int r = db ? power_to_db(plan, out, series(p), out) : (int)SP_OK;   // (m[0] only: a higher moment has no dB form)
        if (!r) e = hipMemcpyAsync(host.out, out, total(p) * sizeof(double), hipMemcpyDeviceToHost, p.ctx->stream);
        return r;
    }
};
}  // namespace

extern "C" int sp_power_moments(sp_context *ctx, const double *d_power, int32_t n, int32_t width, const int32_t *bands, int32_t count,
                                int32_t order, double *d_out)
{
    return plane_resident(ctx, "sp_power_moments", d_power, n, width, MomentKind{bands, count, order, d_out});
}

extern "C" int sp_plan_execute_moments(sp_plan *plan, const void *d_bytes, size_t nbytes, int32_t width, const int32_t *bands, int32_t count,
                                       int32_t order, double *d_out)
{
    return plane_capture(plan, d_bytes, nbytes, width, MomentKind{bands, count, order, d_out});
}

extern "C" int sp_render_moments(sp_context *ctx, const sp_request *req, const uint8_t *bytes, size_t nbytes, int32_t width, const int32_t *bands,
                                 int32_t count, int32_t order, int32_t db, double *out)
{
    return plane_render(ctx, req, bytes, nbytes, width, db, MomentKind{bands, count, order, out});
}

// ------------------------------------------------------------------------------------------------- peak track

extern "C" const char *sp_plan_track_kernel_name_for(const sp_plan *plan, size_t, int32_t)
{
    return plain_kernel_name(plan, "frames_power+track", "scratch_power+track");
}

extern "C" int sp_debug_band_peak(const double *values, int32_t n, int32_t y0, int32_t y1, int32_t *row, double *peak)
{
    if (!values || n < 1 || y0 < 0 || y1 < y0 || y1 > n || (!row && !peak)) return SP_ERR_INVALID_ARG;
    std::vector<uint64_t> bits((size_t)n);
    memcpy(bits.data(), values, (size_t)n * sizeof(double));
    const spt::Best best = spt::band_peak(bits.data(), y0, y1);
    const uint64_t p = spt::peak_bits_of(best);
    if (row) *row = spt::row_of(best);
    if (peak) memcpy(peak, &p, sizeof p);
    return SP_OK;
}

namespace {
// As BandKind, with two arrays of count * width elements, either of which may be null: not written.  In render_small the doubles lie in
// front of the rows.
struct TrackKind {
    static constexpr const char *kRender = "sp_render_track";
    static constexpr const char *kBadPlane = BandKind::kBadPlane;
    const int32_t *bands;
    int32_t count;
    int32_t *row;
    double *peak;

    int check(const PlaneShape &p) const
    {
        if (const char *why = spgeo::check_bands(p.n, bands, count)) return fail(p.ctx, SP_ERR_INVALID_ARG, why);
        if (count > 0 && p.width > 0) {
            if (!row && !peak) return fail(p.ctx, SP_ERR_INVALID_ARG, "a track needs a row array or a peak array");
            if (((uintptr_t)row & 3) != 0)
                return fail(p.ctx, SP_ERR_INVALID_ARG, "the track's rows must be a 4-byte aligned array of count * width int32");
            if (((uintptr_t)peak & 7) != 0)
                return fail(p.ctx, SP_ERR_INVALID_ARG, "the track's peaks must be an 8-byte aligned array of count * width doubles");
        }
        return SP_OK;
    }
    bool empty(const PlaneShape &p) const { return p.width == 0 || count == 0; }
    int clear(const PlaneShape &) const { return SP_OK; }
    int consume(const PlaneShape &p, const double *d_plane, long long frames, long long x_base) const
    {
        if (frames <= 0 || count <= 0) return SP_OK;
        spk::launch_track_max(d_plane, p.n, frames, bands, count, row, peak, p.width, x_base, p.ctx->stream);
        SP_HIP(p.ctx, hipGetLastError());
        return SP_OK;
    }
    int finish(const PlaneShape &) const { return SP_OK; }
    size_t total(const PlaneShape &p) const { return (size_t)count * (size_t)p.width; }
    size_t small_bytes(const PlaneShape &p) const { return total(p) * (sizeof(double) + sizeof(int32_t)); }
    TrackKind on_device(const PlaneShape &p, void *small) const
    {
        return {bands, count, row ? (int32_t *)((double *)small + total(p)) : nullptr, peak ? (double *)small : nullptr};
    }
    int tail(sp_plan *plan, const PlaneShape &p, int32_t db, const TrackKind &host, hipError_t &e) const
    {
        const int r = db && peak ? power_to_db(plan, peak, total(p), peak) : (int)SP_OK;
        if (!r && row) e = hipMemcpyAsync(host.row, row, total(p) * sizeof(int32_t), hipMemcpyDeviceToHost, p.ctx->stream);
        if (!r && e == hipSuccess && peak) e = hipMemcpyAsync(host.peak, peak, total(p) * sizeof(double), hipMemcpyDeviceToHost, p.ctx->stream);
        return r;
    }
};
}  // namespace

extern "C" int sp_power_tracks(sp_context *ctx, const double *d_power, int32_t n, int32_t width, const int32_t *bands, int32_t count,
                               int32_t *d_row, double *d_peak)
{
    return plane_resident(ctx, "sp_power_tracks", d_power, n, width, TrackKind{bands, count, d_row, d_peak});
}

extern "C" int sp_plan_execute_track(sp_plan *plan, const void *d_bytes, size_t nbytes, int32_t width, const int32_t *bands, int32_t count,
                                     int32_t *d_row, double *d_peak)
{
    return plane_capture(plan, d_bytes, nbytes, width, TrackKind{bands, count, d_row, d_peak});
}

extern "C" int sp_render_track(sp_context *ctx, const sp_request *req, const uint8_t *bytes, size_t nbytes, int32_t width, const int32_t *bands,
                               int32_t count, int32_t db, int32_t *row, double *peak)
{
    return plane_render(ctx, req, bytes, nbytes, width, db, TrackKind{bands, count, row, peak});
}

// ------------------------------------------------------------------------------------------------- occupancy counts

extern "C" const char *sp_plan_occupancy_kernel_name_for(const sp_plan *plan, size_t, int32_t)
{
    return plain_kernel_name(plan, "frames_power+occupancy", "scratch_power+occupancy");
}

extern "C" int sp_debug_occupancy(const double *values, const double *thresholds, int32_t n, int32_t y0, int32_t y1, uint32_t *count)
{
    if (!values || !thresholds || !count || n < 1 || y0 < 0 || y1 < y0 || y1 > n) return SP_ERR_INVALID_ARG;
    std::vector<uint64_t> v((size_t)n), t((size_t)n);
    memcpy(v.data(), values, (size_t)n * sizeof(double));
    memcpy(t.data(), thresholds, (size_t)n * sizeof(double));
    *count = spo::band_count(v.data(), t.data(), y0, y1);
    return SP_OK;
}

namespace {
// Two arrays of counts, rows (n words, over all frames) and frames (count * width words, band-major), either of which may be null: not
// touched.  Every block's launch ADDS its hits, so clear() zeroes both on the stream.  A non-null `rows` makes a request of no frames one
// that still writes (n zeros), as the mean's does.  The thresholds are n device doubles; the host-fed form holds its own in `upload`
// and clear() sends them to render_small, where they lie in front of the rows and the rows in front of the frames.
struct OccupancyKind {
    static constexpr const char *kRender = "sp_render_occupancy";
    static constexpr const char *kBadPlane = BandKind::kBadPlane;
    const double *threshold;
    const int32_t *bands;
    int32_t count;
    uint32_t *rows;
    uint32_t *frames;
    const double *upload;   // the host's thresholds where `threshold` is render_small's copy of them, else null

    bool fills_frames(const PlaneShape &p) const { return frames && count > 0 && p.width > 0; }
    int check(const PlaneShape &p) const
    {
        if (p.n > SP_MAX_N) return fail(p.ctx, SP_ERR_INVALID_ARG, "occupancy counts need n <= SP_MAX_N");
        if (const char *why = spgeo::check_bands(p.n, bands, count)) return fail(p.ctx, SP_ERR_INVALID_ARG, why);
        if (!rows && !frames) return fail(p.ctx, SP_ERR_INVALID_ARG, "occupancy counts need a rows array or a frames array");
        if (!threshold || ((uintptr_t)threshold & 7) != 0)
            return fail(p.ctx, SP_ERR_INVALID_ARG, "the thresholds must be an 8-byte aligned array of n doubles");
        if (((uintptr_t)rows & 3) != 0) return fail(p.ctx, SP_ERR_INVALID_ARG, "the row counts must be a 4-byte aligned array of n uint32");
        if (((uintptr_t)frames & 3) != 0)
            return fail(p.ctx, SP_ERR_INVALID_ARG, "the frame counts must be a 4-byte aligned array of count * width uint32");
        return SP_OK;
    }
    bool empty(const PlaneShape &p) const { return !rows && !fills_frames(p); }
    int clear(const PlaneShape &p) const
    {
        if (upload)
            SP_HIP(p.ctx, hipMemcpyAsync((void *)threshold, upload, (size_t)p.n * sizeof(double), hipMemcpyHostToDevice, p.ctx->stream));
        if (rows) SP_HIP(p.ctx, hipMemsetAsync(rows, 0, (size_t)p.n * sizeof(uint32_t), p.ctx->stream));
        if (fills_frames(p)) SP_HIP(p.ctx, hipMemsetAsync(frames, 0, total(p) * sizeof(uint32_t), p.ctx->stream));
        return SP_OK;
    }
    int consume(const PlaneShape &p, const double *d_plane, long long frames_, long long x_base) const
    {
        if (frames_ <= 0) return SP_OK;
        spk::launch_occupancy_count(d_plane, p.n, frames_, threshold, bands, count, rows, fills_frames(p) ? frames : nullptr, p.width, x_base,
                                    p.ctx->stream);
        SP_HIP(p.ctx, hipGetLastError());
        return SP_OK;
    }
    int finish(const PlaneShape &) const { return SP_OK; }
    size_t total(const PlaneShape &p) const { return (size_t)count * (size_t)p.width; }
    size_t small_bytes(const PlaneShape &p) const { return (size_t)p.n * (sizeof(double) + sizeof(uint32_t)) + total(p) * sizeof(uint32_t); }
    OccupancyKind on_device(const PlaneShape &p, void *small) const
    {
        uint32_t *const words = (uint32_t *)((double *)small + p.n);
        return {(const double *)small, bands, count, rows ? words : nullptr, frames ? words + p.n : nullptr, threshold};
    }
    int tail(sp_plan *, const PlaneShape &p, int32_t, const OccupancyKind &host, hipError_t &e) const
    {
        if (rows) e = hipMemcpyAsync(host.rows, rows, (size_t)p.n * sizeof(uint32_t), hipMemcpyDeviceToHost, p.ctx->stream);
        if (e == hipSuccess && fills_frames(p))
            e = hipMemcpyAsync(host.frames, frames, total(p) * sizeof(uint32_t), hipMemcpyDeviceToHost, p.ctx->stream);
        return SP_OK;
    }
};
}  // namespace

extern "C" int sp_power_occupancy(sp_context *ctx, const double *d_power, int32_t n, int32_t width, const double *d_threshold,
                                  const int32_t *bands, int32_t count, uint32_t *d_rows, uint32_t *d_frames)
{
    return plane_resident(ctx, "sp_power_occupancy", d_power, n, width, OccupancyKind{d_threshold, bands, count, d_rows, d_frames, nullptr});
}

extern "C" int sp_plan_execute_occupancy(sp_plan *plan, const void *d_bytes, size_t nbytes, int32_t width, const double *d_threshold,
                                         const int32_t *bands, int32_t count, uint32_t *d_rows, uint32_t *d_frames)
{
    return plane_capture(plan, d_bytes, nbytes, width, OccupancyKind{d_threshold, bands, count, d_rows, d_frames, nullptr});
}

extern "C" int sp_render_occupancy(sp_context *ctx, const sp_request *req, const uint8_t *bytes, size_t nbytes, int32_t width,
                                   const double *threshold, const int32_t *bands, int32_t count, uint32_t *rows, uint32_t *frames)
{
    return plane_render(ctx, req, bytes, nbytes, width, 0, OccupancyKind{threshold, bands, count, rows, frames, nullptr});
}

// ------------------------------------------------------------------------------------------------- percentile traces

extern "C" const char *sp_plan_quantile_kernel_name_for(const sp_plan *plan, size_t, int32_t)
{
    return plain_kernel_name(plan, "frames_power+quantile", "scratch_power+quantile");
}

extern "C" int32_t sp_quantile_rank(int32_t width, double q)
{
    if (width < 1 || !(q >= 0.0 && q <= 1.0)) return -1;   // (a NaN q fails both compares)
    return (int32_t)std::floor(q * (double)(width - 1));
}

extern "C" int sp_debug_quantile(const double *values, int32_t count, int32_t rank, double *out)
{
    if (!values || !out || count < 1 || rank < 0 || rank >= count) return SP_ERR_INVALID_ARG;
    std::vector<uint64_t> bits((size_t)count);
    memcpy(bits.data(), values, (size_t)count * sizeof(double));
    const uint64_t r = spq::reply_bits(spq::select(bits.data(), (uint32_t)count, (uint32_t)rank));
    memcpy(out, &r, sizeof r);
    return SP_OK;
}

namespace {
// The one consumer that keeps the request's plane: clear() reserves the context's workspace u64 keys[n][width], every block's launch
// transposes its frames into it as keys and finish() selects the ranks of every row from it.  No request is empty: one of no frames
// still gives count * n NaNs (the select's launch writes them; nothing was gathered and nothing is read).
struct QuantileKind {
    static constexpr const char *kRender = "sp_render_quantile";
    static constexpr const char *kBadPlane = ": d_power and d_out must be 8-byte aligned device pointers";
    const int32_t *ranks;
    int32_t count;
    double *out;   // count * n doubles, rank-major

    int check(const PlaneShape &p) const
    {
        if (p.n > SP_MAX_N) return fail(p.ctx, SP_ERR_INVALID_ARG, "percentile traces need n <= SP_MAX_N");
        if (!ranks || count < 1 || count > SP_MAX_RANKS) return fail(p.ctx, SP_ERR_INVALID_ARG, "percentile traces need 1 .. SP_MAX_RANKS ranks");
        if (p.width > 0)
            for (int32_t r = 0; r < count; r++)
                if (ranks[r] < 0 || ranks[r] >= p.width) return fail(p.ctx, SP_ERR_INVALID_ARG, "a rank must satisfy 0 <= k < width");
        if (!out || ((uintptr_t)out & 7) != 0)
            return fail(p.ctx, SP_ERR_INVALID_ARG, "the percentile traces must be an 8-byte aligned array of count * n doubles");
        return SP_OK;
    }
    bool empty(const PlaneShape &) const { return false; }
    int clear(const PlaneShape &p) const
    {
        const int rc = p.ctx->quantile_ws.reserve(sizeof(unsigned long long) * (size_t)p.n * (size_t)(p.width > 0 ? p.width : 0));
        return rc ? fail(p.ctx, rc, "percentile workspace: out of device memory") : (int)SP_OK;
    }
    int consume(const PlaneShape &p, const double *d_plane, long long frames, long long x_base) const
    {
        if (frames <= 0) return SP_OK;
        spk::launch_quantile_gather(d_plane, p.n, frames, (unsigned long long *)p.ctx->quantile_ws.p, p.width, x_base, p.ctx->stream);
        SP_HIP(p.ctx, hipGetLastError());
        return SP_OK;
    }
    int finish(const PlaneShape &p) const
    {
        spk::launch_quantile_select((const unsigned long long *)p.ctx->quantile_ws.p, p.n, p.width, ranks, count, out, p.ctx->stream);
        SP_HIP(p.ctx, hipGetLastError());
        return SP_OK;
    }
    size_t total(const PlaneShape &p) const { return (size_t)count * (size_t)p.n; }
    size_t small_bytes(const PlaneShape &p) const { return total(p) * sizeof(double); }
    QuantileKind on_device(const PlaneShape &, void *small) const { return {ranks, count, (double *)small}; }
    int tail(sp_plan *plan, const PlaneShape &p, int32_t db, const QuantileKind &host, hipError_t &e) const
    {
        const int r = db ? power_to_db(plan, out, total(p), out) : (int)SP_OK;
        if (!r) e = hipMemcpyAsync(host.out, out, total(p) * sizeof(double), hipMemcpyDeviceToHost, p.ctx->stream);
        return r;
    }
};
}  // namespace

extern "C" int sp_power_quantile(sp_context *ctx, const double *d_power, int32_t n, int32_t width, const int32_t *ranks, int32_t count,
                                 double *d_out)
{
    return plane_resident(ctx, "sp_power_quantile", d_power, n, width, QuantileKind{ranks, count, d_out});
}

extern "C" int sp_plan_execute_quantile(sp_plan *plan, const void *d_bytes, size_t nbytes, int32_t width, const int32_t *ranks, int32_t count,
                                        double *d_out)
{
    return plane_capture(plan, d_bytes, nbytes, width, QuantileKind{ranks, count, d_out});
}

extern "C" int sp_render_quantile(sp_context *ctx, const sp_request *req, const uint8_t *bytes, size_t nbytes, int32_t width, int32_t db,
                                  const int32_t *ranks, int32_t count, double *out)
{
    return plane_render(ctx, req, bytes, nbytes, width, db, QuantileKind{ranks, count, out});
}

// ------------------------------------------------------------------------------------------------- burst lists

extern "C" const char *sp_plan_bursts_kernel_name_for(const sp_plan *plan, size_t, int32_t)
{
    return plain_kernel_name(plan, "frames_power+bursts", "scratch_power+bursts");
}

namespace {
// What every burst entry point refuses of its thresholds - nullptr where they are in order - and their keys into hi_key[count] and
// lo_key[count] where those are not null.
const char *burst_keys(const double *hi, const double *lo, int32_t count, uint64_t *hi_key, uint64_t *lo_key)
{
    if (count > 0 && (!hi || !lo)) return "burst lists need hi and lo, count doubles each";
    for (int32_t b = 0; b < count; b++) {
        uint64_t hb, lb;
        memcpy(&hb, hi + b, sizeof hb);
        memcpy(&lb, lo + b, sizeof lb);
        const uint64_t hk = spo::threshold_key(hb), lk = spo::threshold_key(lb);
        if (hk == spo::kNoHitKey || lk == spo::kNoHitKey) return "a burst threshold must not be a NaN";
        if (lk > hk) return "burst lists need lo <= hi for every band";
        if (hi_key) hi_key[b] = hk;
        if (lo_key) lo_key[b] = lk;
    }
    return nullptr;
}

// ... and of its outputs
const char *burst_outputs(int32_t count, int32_t max_bursts, const uint32_t *counts, const int32_t *edges)
{
    if (max_bursts < 0) return "max_bursts >= 0 is required";
    if (2ll * (long long)max_bursts * (long long)(count > 0 ? count : 0) > 0x7fffffffll) return "2 * max_bursts * count must fit 31 bits";
    if (!counts && !(edges && max_bursts > 0)) return "burst lists need a counts array or an edges array with max_bursts > 0";
    if (((uintptr_t)counts & 3) != 0) return "the burst counts must be a 4-byte aligned array of count uint32";
    if (((uintptr_t)edges & 3) != 0) return "the burst edges must be a 4-byte aligned array of count * 2 * max_bursts int32";
    return nullptr;
}

// The three launches on a band-major series of the device and the 0xFF fill in front of them; `records`: spk::burst_record_bytes.
int burst_scan(sp_context *ctx, const double *d_series, int32_t count, int32_t width, const double *hi, const double *lo, int32_t max_bursts,
               void *records, uint32_t *counts, int32_t *edges)
{
    uint64_t hi_key[SP_MAX_BANDS], lo_key[SP_MAX_BANDS];
    (void)burst_keys(hi, lo, count, hi_key, lo_key);   // (checked before)
    spk::launch_bursts(d_series, count, width, hi_key, lo_key, max_bursts, (unsigned long long *)records, counts, edges, ctx->stream);
    SP_HIP(ctx, hipGetLastError());
    return SP_OK;
}

// The first consumer whose reply depends on the order of the frames: clear() reserves the context's workspace - the band series
// f64[count][width] and the segments' records behind it - and fills `edges` with -1; every block's launch is the band-power series'
// own, its columns at x_base of the workspace series, so that the series is the same whatever the window; finish() is the three
// launches on it.  A request without a band writes nothing; one without a frame still writes (count zeros and the fill).
struct BurstKind {
    static constexpr const char *kRender = "sp_render_bursts";
    static constexpr const char *kBadPlane = BandKind::kBadPlane;
    const int32_t *bands;
    int32_t count;
    const double *hi, *lo;   // host arrays
    int32_t max_bursts;
    uint32_t *counts;        // count words, or null
    int32_t *edges;          // count * 2 * max_bursts words, or null

    bool lists() const { return edges && max_bursts > 0; }
    size_t series_bytes(const PlaneShape &p) const { return sizeof(double) * (size_t)count * (size_t)p.width; }
    size_t edge_bytes() const { return sizeof(int32_t) * 2 * (size_t)max_bursts * (size_t)count; }
    int check(const PlaneShape &p) const
    {
        if (const char *why = spgeo::check_bands(p.n, bands, count)) return fail(p.ctx, SP_ERR_INVALID_ARG, why);
        if (const char *why = burst_keys(hi, lo, count, nullptr, nullptr)) return fail(p.ctx, SP_ERR_INVALID_ARG, why);
        if (const char *why = burst_outputs(count, max_bursts, counts, edges)) return fail(p.ctx, SP_ERR_INVALID_ARG, why);
        return SP_OK;
    }
    bool empty(const PlaneShape &) const { return count == 0; }
    int clear(const PlaneShape &p) const
    {
        const int rc = p.ctx->burst_ws.reserve(series_bytes(p) + spk::burst_record_bytes(count, p.width));
        if (rc) return fail(p.ctx, rc, "burst workspace: out of device memory");
        if (lists()) SP_HIP(p.ctx, hipMemsetAsync(edges, 0xFF, edge_bytes(), p.ctx->stream));
        return SP_OK;
    }
    int consume(const PlaneShape &p, const double *d_plane, long long frames, long long x_base) const
    {
        if (frames <= 0) return SP_OK;
        spk::launch_band_sum(d_plane, p.n, frames, bands, count, 0, (double *)p.ctx->burst_ws.p, p.width, x_base, p.ctx->stream);
        SP_HIP(p.ctx, hipGetLastError());
        return SP_OK;
    }
    int finish(const PlaneShape &p) const
    {
        return burst_scan(p.ctx, (const double *)p.ctx->burst_ws.p, count, p.width, hi, lo, max_bursts,
                          (char *)p.ctx->burst_ws.p + series_bytes(p), counts, lists() ? edges : nullptr);
    }
    size_t small_bytes(const PlaneShape &) const { return sizeof(uint32_t) * (size_t)count + edge_bytes(); }
    BurstKind on_device(const PlaneShape &, void *small) const
    {
        return {bands, count, hi, lo, max_bursts, counts ? (uint32_t *)small : nullptr, lists() ? (int32_t *)small + count : nullptr};
    }
    int tail(sp_plan *, const PlaneShape &p, int32_t, const BurstKind &host, hipError_t &e) const
    {
        if (counts) e = hipMemcpyAsync(host.counts, counts, sizeof(uint32_t) * (size_t)count, hipMemcpyDeviceToHost, p.ctx->stream);
        if (e == hipSuccess && lists()) e = hipMemcpyAsync(host.edges, edges, edge_bytes(), hipMemcpyDeviceToHost, p.ctx->stream);
        return SP_OK;
    }
};
}  // namespace

extern "C" int sp_power_bursts(sp_context *ctx, const double *d_power, int32_t n, int32_t width, const int32_t *bands, int32_t count,
                               const double *hi, const double *lo, int32_t max_bursts, uint32_t *d_counts, int32_t *d_edges)
{
    return plane_resident(ctx, "sp_power_bursts", d_power, n, width, BurstKind{bands, count, hi, lo, max_bursts, d_counts, d_edges});
}

extern "C" int sp_plan_execute_bursts(sp_plan *plan, const void *d_bytes, size_t nbytes, int32_t width, const int32_t *bands, int32_t count,
                                      const double *hi, const double *lo, int32_t max_bursts, uint32_t *d_counts, int32_t *d_edges)
{
    return plane_capture(plan, d_bytes, nbytes, width, BurstKind{bands, count, hi, lo, max_bursts, d_counts, d_edges});
}

extern "C" int sp_render_bursts(sp_context *ctx, const sp_request *req, const uint8_t *bytes, size_t nbytes, int32_t width, const int32_t *bands,
                                int32_t count, const double *hi, const double *lo, int32_t max_bursts, uint32_t *counts, int32_t *edges)
{
    return plane_render(ctx, req, bytes, nbytes, width, 0, BurstKind{bands, count, hi, lo, max_bursts, counts, edges});
}

extern "C" int sp_series_bursts(sp_context *ctx, const double *d_series, int32_t count, int32_t width, const double *hi, const double *lo,
                                int32_t max_bursts, uint32_t *d_counts, int32_t *d_edges)
{
    if (!ctx) return SP_ERR_INVALID_ARG;
    if (count < 0 || count > SP_MAX_BANDS || width < 0)
        return fail(ctx, SP_ERR_INVALID_ARG, "sp_series_bursts: count within 0 .. SP_MAX_BANDS and width >= 0 are required");
    if (const char *why = burst_keys(hi, lo, count, nullptr, nullptr)) return fail(ctx, SP_ERR_INVALID_ARG, why);
    if (const char *why = burst_outputs(count, max_bursts, d_counts, d_edges)) return fail(ctx, SP_ERR_INVALID_ARG, why);
    if (count == 0) return SP_OK;
    if ((width > 0 && !d_series) || ((uintptr_t)d_series & 7) != 0)
        return fail(ctx, SP_ERR_INVALID_ARG, "sp_series_bursts: d_series must be an 8-byte aligned device pointer");
    SP_HIP(ctx, hipSetDevice(ctx->device));
    const bool lists = d_edges && max_bursts > 0;
    return timed(ctx, [&] {
        const int rc = ctx->burst_ws.reserve(spk::burst_record_bytes(count, width));
        if (rc) return fail(ctx, rc, "burst workspace: out of device memory");
        if (lists)
            SP_HIP(ctx, hipMemsetAsync(d_edges, 0xFF, sizeof(int32_t) * 2 * (size_t)max_bursts * (size_t)count, ctx->stream));
        return burst_scan(ctx, d_series, count, width, hi, lo, max_bursts, ctx->burst_ws.p, d_counts, lists ? d_edges : nullptr);
    });
}

extern "C" int sp_debug_bursts(const double *values, int32_t width, double hi, double lo, int32_t max_bursts, uint32_t *count_out,
                               int32_t *edges_out)
{
    if (width < 0 || (width > 0 && !values)) return SP_ERR_INVALID_ARG;
    uint64_t hi_key = 0, lo_key = 0;
    if (burst_keys(&hi, &lo, 1, &hi_key, &lo_key) || burst_outputs(1, max_bursts, count_out, edges_out)) return SP_ERR_INVALID_ARG;
    std::vector<uint64_t> bits((size_t)width);
    if (width) memcpy(bits.data(), values, (size_t)width * sizeof(double));
    const uint32_t total = spb::scan(bits.data(), width, hi_key, lo_key, max_bursts, max_bursts > 0 ? edges_out : nullptr);
    if (count_out) *count_out = total;
    return SP_OK;
}

// ------------------------------------------------------------------------------------------------- burst measurements

extern "C" const char *sp_plan_pulses_kernel_name_for(const sp_plan *plan, size_t, int32_t)
{
    return plain_kernel_name(plan, "frames_power+pulses", "scratch_power+pulses");
}

namespace {
// The per-burst outputs of a measurement request, each count * max_bursts values, each may be null.
struct PulseOut {
    double *energy, *peak;
    int32_t *peak_at;
    bool any() const { return energy || peak || peak_at; }
};

// What every measurement entry point refuses of its outputs: burst_outputs' refusals in burst_outputs' order, with the three per-burst
// arrays counted among what may be asked for, and their alignment behind.
const char *pulse_outputs(int32_t count, int32_t max_bursts, const uint32_t *counts, const int32_t *edges, const PulseOut &o)
{
    if (max_bursts < 0) return "max_bursts >= 0 is required";
    if (2ll * (long long)max_bursts * (long long)(count > 0 ? count : 0) > 0x7fffffffll) return "2 * max_bursts * count must fit 31 bits";
    if (!counts && !((edges || o.any()) && max_bursts > 0))
        return "burst measurements need a counts array or, with max_bursts > 0, an edges, energy, peak or peak_at array";
    if (((uintptr_t)counts & 3) != 0) return "the burst counts must be a 4-byte aligned array of count uint32";
    if (((uintptr_t)edges & 3) != 0) return "the burst edges must be a 4-byte aligned array of count * 2 * max_bursts int32";
    if (((uintptr_t)o.energy & 7) != 0 || ((uintptr_t)o.peak & 7) != 0)
        return "the burst energy and peak must be 8-byte aligned arrays of count * max_bursts doubles";
    if (((uintptr_t)o.peak_at & 3) != 0) return "the burst peak_at must be a 4-byte aligned array of count * max_bursts int32";
    return nullptr;
}

// The context's measurement workspace for `count` bands of max_bursts bursts: the launcher's work area and count uint32 behind it.
int pulse_reserve(sp_context *ctx, int32_t count, int32_t max_bursts)
{
    const int rc = ctx->pulse_ws.reserve(spk::pulse_work_bytes(count, max_bursts) + sizeof(uint32_t) * (size_t)count);
    return rc ? fail(ctx, rc, "burst measurement workspace: out of device memory") : (int)SP_OK;
}

// The 0xFF fill of the per-burst outputs, on the stream in front of the launches.
int pulse_fill(sp_context *ctx, int32_t count, int32_t max_bursts, int32_t *edges, const PulseOut &o)
{
    const size_t bursts = (size_t)count * (size_t)max_bursts;
    if (!bursts) return SP_OK;
    if (edges) SP_HIP(ctx, hipMemsetAsync(edges, 0xFF, sizeof(int32_t) * 2 * bursts, ctx->stream));
    if (o.energy) SP_HIP(ctx, hipMemsetAsync(o.energy, 0xFF, sizeof(double) * bursts, ctx->stream));
    if (o.peak) SP_HIP(ctx, hipMemsetAsync(o.peak, 0xFF, sizeof(double) * bursts, ctx->stream));
    if (o.peak_at) SP_HIP(ctx, hipMemsetAsync(o.peak_at, 0xFF, sizeof(int32_t) * bursts, ctx->stream));
    return SP_OK;
}

// The burst launches (burst_scan, unchanged) and the measurement behind them on a band-major series of the device.  Where the caller
// has no counts array the bursts are counted into the workspace: k_pulse_finish reads how many are listed.
int pulse_scan(sp_context *ctx, const double *d_series, int32_t count, int32_t width, const double *hi, const double *lo, int32_t max_bursts,
               void *records, uint32_t *counts, int32_t *edges, const PulseOut &o)
{
    const bool measured = o.any() && max_bursts > 0;
    uint32_t *const ws_counts = (uint32_t *)((char *)ctx->pulse_ws.p + spk::pulse_work_bytes(count, max_bursts));
    uint32_t *const total = counts || !measured ? counts : ws_counts;
    const int rc = burst_scan(ctx, d_series, count, width, hi, lo, max_bursts, records, total, max_bursts > 0 ? edges : nullptr);
    if (rc || !measured) return rc;
    uint64_t hi_key[SP_MAX_BANDS], lo_key[SP_MAX_BANDS];
    (void)burst_keys(hi, lo, count, hi_key, lo_key);   // (checked before)
    SP_HIP(ctx, spk::launch_pulses(d_series, count, width, hi_key, lo_key, max_bursts, (const unsigned long long *)records, total,
                                   ctx->pulse_ws.p, o.energy, o.peak, o.peak_at, ctx->stream));
    return SP_OK;
}

// The burst lists' kind with three more outputs: the series is made as BurstKind makes it, the workspace of the measurement is reserved
// beside burst_ws, the fill covers the per-burst arrays, and finish() runs the measurement behind the three burst launches.
struct PulseKind {
    static constexpr const char *kRender = "sp_render_pulses";
    static constexpr const char *kBadPlane = BandKind::kBadPlane;
    BurstKind b;
    PulseOut o;

    bool per_burst() const { return b.max_bursts > 0; }
    size_t bursts() const { return (size_t)b.count * (size_t)b.max_bursts; }
    int check(const PlaneShape &p) const
    {
        if (const char *why = spgeo::check_bands(p.n, b.bands, b.count)) return fail(p.ctx, SP_ERR_INVALID_ARG, why);
        if (const char *why = burst_keys(b.hi, b.lo, b.count, nullptr, nullptr)) return fail(p.ctx, SP_ERR_INVALID_ARG, why);
        if (const char *why = pulse_outputs(b.count, b.max_bursts, b.counts, b.edges, o)) return fail(p.ctx, SP_ERR_INVALID_ARG, why);
        return SP_OK;
    }
    bool empty(const PlaneShape &p) const { return b.empty(p); }
    int clear(const PlaneShape &p) const
    {
        int rc = p.ctx->burst_ws.reserve(b.series_bytes(p) + spk::burst_record_bytes(b.count, p.width));
        if (rc) return fail(p.ctx, rc, "burst workspace: out of device memory");
        rc = pulse_reserve(p.ctx, b.count, b.max_bursts);
        return rc ? rc : pulse_fill(p.ctx, b.count, b.max_bursts, b.edges, o);
    }
    int consume(const PlaneShape &p, const double *d_plane, long long frames, long long x_base) const { return b.consume(p, d_plane, frames, x_base); }
    int finish(const PlaneShape &p) const
    {
        return pulse_scan(p.ctx, (const double *)p.ctx->burst_ws.p, b.count, p.width, b.hi, b.lo, b.max_bursts,
                          (char *)p.ctx->burst_ws.p + b.series_bytes(p), b.counts, b.edges, o);
    }
    // render_small: the doubles in front (8-byte aligned), then counts, edges and peak_at
    size_t small_bytes(const PlaneShape &) const
    {
        return (2 * sizeof(double) + 3 * sizeof(int32_t)) * bursts() + sizeof(uint32_t) * (size_t)b.count;
    }
    PulseKind on_device(const PlaneShape &, void *small) const
    {
        double *const d = (double *)small;
        int32_t *const w = (int32_t *)(d + 2 * bursts());
        const bool per = per_burst();
        return {{b.bands, b.count, b.hi, b.lo, b.max_bursts, b.counts ? (uint32_t *)w : nullptr, per && b.edges ? w + b.count : nullptr},
                {per && o.energy ? d : nullptr, per && o.peak ? d + bursts() : nullptr,
                 per && o.peak_at ? w + b.count + 2 * bursts() : nullptr}};
    }
    int tail(sp_plan *, const PlaneShape &p, int32_t, const PulseKind &host, hipError_t &e) const
    {
        hipStream_t st = p.ctx->stream;
        if (b.counts) e = hipMemcpyAsync(host.b.counts, b.counts, sizeof(uint32_t) * (size_t)b.count, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && b.edges) e = hipMemcpyAsync(host.b.edges, b.edges, sizeof(int32_t) * 2 * bursts(), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && o.energy) e = hipMemcpyAsync(host.o.energy, o.energy, sizeof(double) * bursts(), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && o.peak) e = hipMemcpyAsync(host.o.peak, o.peak, sizeof(double) * bursts(), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && o.peak_at) e = hipMemcpyAsync(host.o.peak_at, o.peak_at, sizeof(int32_t) * bursts(), hipMemcpyDeviceToHost, st);
        return SP_OK;
    }
};

// the kind of an entry point's arguments (a per-burst array with max_bursts == 0 counts as absent: pulse_fill, pulse_scan, on_device)
PulseKind pulse_kind(const int32_t *bands, int32_t count, const double *hi, const double *lo, int32_t max_bursts, uint32_t *counts,
                     int32_t *edges, double *energy, double *peak, int32_t *peak_at)
{
    return {{bands, count, hi, lo, max_bursts, counts, edges}, {energy, peak, peak_at}};
}
}  // namespace

extern "C" int sp_power_pulses(sp_context *ctx, const double *d_power, int32_t n, int32_t width, const int32_t *bands, int32_t count,
                               const double *hi, const double *lo, int32_t max_bursts, uint32_t *d_counts, int32_t *d_edges, double *d_energy,
                               double *d_peak, int32_t *d_peak_at)
{
    return plane_resident(ctx, "sp_power_pulses", d_power, n, width,
                          pulse_kind(bands, count, hi, lo, max_bursts, d_counts, d_edges, d_energy, d_peak, d_peak_at));
}

extern "C" int sp_plan_execute_pulses(sp_plan *plan, const void *d_bytes, size_t nbytes, int32_t width, const int32_t *bands, int32_t count,
                                      const double *hi, const double *lo, int32_t max_bursts, uint32_t *d_counts, int32_t *d_edges,
                                      double *d_energy, double *d_peak, int32_t *d_peak_at)
{
    return plane_capture(plan, d_bytes, nbytes, width, pulse_kind(bands, count, hi, lo, max_bursts, d_counts, d_edges, d_energy, d_peak, d_peak_at));
}

extern "C" int sp_render_pulses(sp_context *ctx, const sp_request *req, const uint8_t *bytes, size_t nbytes, int32_t width, const int32_t *bands,
                                int32_t count, const double *hi, const double *lo, int32_t max_bursts, uint32_t *counts, int32_t *edges,
                                double *energy, double *peak, int32_t *peak_at)
{
    return plane_render(ctx, req, bytes, nbytes, width, 0, pulse_kind(bands, count, hi, lo, max_bursts, counts, edges, energy, peak, peak_at));
}

extern "C" int sp_series_pulses(sp_context *ctx, const double *d_series, int32_t count, int32_t width, const double *hi, const double *lo,
                                int32_t max_bursts, uint32_t *d_counts, int32_t *d_edges, double *d_energy, double *d_peak, int32_t *d_peak_at)
{
    if (!ctx) return SP_ERR_INVALID_ARG;
    if (count < 0 || count > SP_MAX_BANDS || width < 0)
        return fail(ctx, SP_ERR_INVALID_ARG, "sp_series_pulses: count within 0 .. SP_MAX_BANDS and width >= 0 are required");
    const PulseOut o{d_energy, d_peak, d_peak_at};
    if (const char *why = burst_keys(hi, lo, count, nullptr, nullptr)) return fail(ctx, SP_ERR_INVALID_ARG, why);
    if (const char *why = pulse_outputs(count, max_bursts, d_counts, d_edges, o)) return fail(ctx, SP_ERR_INVALID_ARG, why);
    if (count == 0) return SP_OK;
    if ((width > 0 && !d_series) || ((uintptr_t)d_series & 7) != 0)
        return fail(ctx, SP_ERR_INVALID_ARG, "sp_series_pulses: d_series must be an 8-byte aligned device pointer");
    SP_HIP(ctx, hipSetDevice(ctx->device));
    return timed(ctx, [&] {
        int rc = ctx->burst_ws.reserve(spk::burst_record_bytes(count, width));
        if (rc) return fail(ctx, rc, "burst workspace: out of device memory");
        rc = pulse_reserve(ctx, count, max_bursts);
        if (!rc) rc = pulse_fill(ctx, count, max_bursts, d_edges, o);
        return rc ? rc : pulse_scan(ctx, d_series, count, width, hi, lo, max_bursts, ctx->burst_ws.p, d_counts, d_edges, o);
    });
}

extern "C" int sp_debug_pulses(const double *values, int32_t width, double hi, double lo, int32_t max_bursts, uint32_t *count_out,
                               int32_t *edges_out, double *energy_out, double *peak_out, int32_t *peak_at_out)
{
    if (width < 0 || (width > 0 && !values)) return SP_ERR_INVALID_ARG;
    uint64_t hi_key = 0, lo_key = 0;
    if (burst_keys(&hi, &lo, 1, &hi_key, &lo_key) || pulse_outputs(1, max_bursts, count_out, edges_out, PulseOut{energy_out, peak_out, peak_at_out}))
        return SP_ERR_INVALID_ARG;
    std::vector<uint64_t> bits((size_t)width);
    if (width) memcpy(bits.data(), values, (size_t)width * sizeof(double));
    std::vector<int32_t> own_edges(edges_out ? 0 : 2 * (size_t)max_bursts);
    const uint32_t total = spp::measure(bits.data(), width, hi_key, lo_key, max_bursts, edges_out ? edges_out : own_edges.data(),
                                        (uint64_t *)energy_out, (uint64_t *)peak_out, peak_at_out);
    if (count_out) *count_out = total;
    return SP_OK;
}

// ------------------------------------------------------------------------------------------------- exact lagged covariances

extern "C" const char *sp_plan_lagcov_kernel_name_for(const sp_plan *plan, size_t, int32_t)
{
    return plain_kernel_name(plan, "frames_power+lagcov", "scratch_power+lagcov");
}

extern "C" int sp_debug_lagcov(const double *a, const double *b, int32_t width, int32_t lags, double *out)
{
    if (!out || width < 0 || (width > 0 && (!a || !b)) || lags < 1 || lags > SP_MAX_LAGS) return SP_ERR_INVALID_ARG;
    std::vector<uint64_t> ba((size_t)width), bb((size_t)width), r(3 * (size_t)lags);
    if (width) memcpy(ba.data(), a, (size_t)width * sizeof(double)), memcpy(bb.data(), b, (size_t)width * sizeof(double));
    if (!spl::lagcov_bits(ba.data(), bb.data(), width, lags, r.data())) return SP_ERR_INVALID_ARG;
    memcpy(out, r.data(), r.size() * sizeof(uint64_t));
    return SP_OK;
}

// (tests) k_lagcov_accumulate's grid for `terms` terms of npairs pairs and `lags` lags on a part with cu_count CUs, from the function
// its launch calls.
extern "C" int sp_debug_lagcov_launch(int32_t npairs, int32_t lags, int64_t terms, int32_t cu_count, int64_t *out, size_t capacity,
                                      size_t *used)
{
    if (npairs < 1 || npairs > SP_MAX_LAG_PAIRS || lags < 1 || lags > SP_MAX_LAGS || terms < 1 || cu_count < 1 || !used)
        return SP_ERR_INVALID_ARG;
    long long shape[3];
    spk::lagcov_launch_shape(npairs, lags, terms, cu_count, shape);
    const int64_t v[] = {shape[0], shape[1], shape[2]};
    *used = sizeof v / sizeof v[0];
    if (*used > capacity || !out) return SP_ERR_INVALID_ARG;
    memcpy(out, v, sizeof v);
    return SP_OK;
}

namespace {
static_assert(SP_MAX_LAG_PAIRS == spl::kMaxPairs && SP_MAX_LAGS == spl::kMaxLags, "the limits of the header are the core's");

// What every lagged-covariance entry point refuses of its pairs, lags and output - nullptr where they are in order.
const char *lagcov_args(int32_t count, const int32_t *pairs, int32_t npairs, int32_t lags, const double *out)
{
    if (npairs < 0 || npairs > SP_MAX_LAG_PAIRS) return "npairs within 0 .. SP_MAX_LAG_PAIRS is required";
    if (lags < 1 || lags > SP_MAX_LAGS) return "lags within 1 .. SP_MAX_LAGS is required";
    if (npairs > 0 && !pairs) return "lagged covariances need pairs, 2 * npairs int32";
    for (int32_t k = 0; k < 2 * npairs; k++)
        if (pairs[k] < 0 || pairs[k] >= count) return "a pair's index must lie within [0, count)";
    if (npairs > 0 && (!out || ((uintptr_t)out & 7) != 0)) return "the reply must be an 8-byte aligned array of 3 * npairs * lags doubles";
    return nullptr;
}

// The memset and the two launches on a band-major series of the device; `work`: spk::lagcov_work_bytes.
int lagcov_scan(sp_context *ctx, const double *d_series, int32_t width, const int32_t *pairs, int32_t npairs, int32_t lags, void *work,
                double *out)
{
    SP_HIP(ctx, spk::launch_lagcov(d_series, width, pairs, npairs, lags, work, out, ctx->cu_count, ctx->stream));
    SP_HIP(ctx, hipGetLastError());
    return SP_OK;
}

// BurstKind's way to a whole series: clear() reserves the context's workspace of its own - the band series f64[count][width] and the
// cells behind it - every block's launch is the band-power series' own, its columns at x_base of the workspace series, so that the
// series is the same whatever the window; finish() zeroes the cells and runs the two launches on it.  A request without a pair or
// without a band writes nothing.
struct LagcovKind {
    static constexpr const char *kRender = "sp_render_lagcov";
    static constexpr const char *kBadPlane = BandKind::kBadPlane;
    const int32_t *bands;
    int32_t count;
    const int32_t *pairs;   // host array
    int32_t npairs, lags;
    double *out;            // 3 * npairs * lags doubles

    size_t series_bytes(const PlaneShape &p) const { return sizeof(double) * (size_t)count * (size_t)p.width; }
    size_t reply_bytes() const { return sizeof(double) * 3 * (size_t)npairs * (size_t)lags; }
    int check(const PlaneShape &p) const
    {
        if (const char *why = spgeo::check_bands(p.n, bands, count)) return fail(p.ctx, SP_ERR_INVALID_ARG, why);
        if (const char *why = lagcov_args(count, pairs, npairs, lags, out)) return fail(p.ctx, SP_ERR_INVALID_ARG, why);
        return SP_OK;
    }
    bool empty(const PlaneShape &) const { return npairs == 0 || count == 0; }
    int clear(const PlaneShape &p) const
    {
        const int rc = p.ctx->lagcov_ws.reserve(series_bytes(p) + spk::lagcov_work_bytes(npairs, lags));
        return rc ? fail(p.ctx, rc, "lagged covariance workspace: out of device memory") : (int)SP_OK;
    }
    int consume(const PlaneShape &p, const double *d_plane, long long frames, long long x_base) const
    {
        if (frames <= 0) return SP_OK;
        spk::launch_band_sum(d_plane, p.n, frames, bands, count, 0, (double *)p.ctx->lagcov_ws.p, p.width, x_base, p.ctx->stream);
        SP_HIP(p.ctx, hipGetLastError());
        return SP_OK;
    }
    int finish(const PlaneShape &p) const
    {
        return lagcov_scan(p.ctx, (const double *)p.ctx->lagcov_ws.p, p.width, pairs, npairs, lags, (char *)p.ctx->lagcov_ws.p + series_bytes(p),
                           out);
    }
    size_t small_bytes(const PlaneShape &) const { return reply_bytes(); }
    LagcovKind on_device(const PlaneShape &, void *small) const { return {bands, count, pairs, npairs, lags, (double *)small}; }
    // (no dB form: a covariance has a sign)
    int tail(sp_plan *, const PlaneShape &p, int32_t, const LagcovKind &host, hipError_t &e) const
    {
        e = hipMemcpyAsync(host.out, out, reply_bytes(), hipMemcpyDeviceToHost, p.ctx->stream);
        return SP_OK;
    }
};
}  // namespace

extern "C" int sp_power_lagcov(sp_context *ctx, const double *d_power, int32_t n, int32_t width, const int32_t *bands, int32_t count,
                               const int32_t *pairs, int32_t npairs, int32_t lags, double *d_out)
{
    return plane_resident(ctx, "sp_power_lagcov", d_power, n, width, LagcovKind{bands, count, pairs, npairs, lags, d_out});
}

extern "C" int sp_plan_execute_lagcov(sp_plan *plan, const void *d_bytes, size_t nbytes, int32_t width, const int32_t *bands, int32_t count,
                                      const int32_t *pairs, int32_t npairs, int32_t lags, double *d_out)
{
    return plane_capture(plan, d_bytes, nbytes, width, LagcovKind{bands, count, pairs, npairs, lags, d_out});
}

extern "C" int sp_render_lagcov(sp_context *ctx, const sp_request *req, const uint8_t *bytes, size_t nbytes, int32_t width, const int32_t *bands,
                                int32_t count, const int32_t *pairs, int32_t npairs, int32_t lags, double *out)
{
    return plane_render(ctx, req, bytes, nbytes, width, 0, LagcovKind{bands, count, pairs, npairs, lags, out});
}

extern "C" int sp_series_lagcov(sp_context *ctx, const double *d_series, int32_t count, int32_t width, const int32_t *pairs, int32_t npairs,
                                int32_t lags, double *d_out)
{
    if (!ctx) return SP_ERR_INVALID_ARG;
    if (count < 0 || count > SP_MAX_BANDS || width < 0)
        return fail(ctx, SP_ERR_INVALID_ARG, "sp_series_lagcov: count within 0 .. SP_MAX_BANDS and width >= 0 are required");
    if (const char *why = lagcov_args(count, pairs, npairs, lags, d_out)) return fail(ctx, SP_ERR_INVALID_ARG, why);
    if (npairs == 0 || count == 0) return SP_OK;
    if ((width > 0 && !d_series) || ((uintptr_t)d_series & 7) != 0)
        return fail(ctx, SP_ERR_INVALID_ARG, "sp_series_lagcov: d_series must be an 8-byte aligned device pointer");
    SP_HIP(ctx, hipSetDevice(ctx->device));
    return timed(ctx, [&] {
        const int rc = ctx->lagcov_ws.reserve(spk::lagcov_work_bytes(npairs, lags));
        if (rc) return fail(ctx, rc, "lagged covariance workspace: out of device memory");
        return lagcov_scan(ctx, d_series, width, pairs, npairs, lags, ctx->lagcov_ws.p, d_out);
    });
}

// ------------------------------------------------------------------------------------------------- requests by name

extern "C" int sp_named_resolve(const char *window, const char *cmap, const char **window_name, const char **cmap_key, int32_t *lut_len)
{
    // lookup(windows, name) || blackmanHarrisWindow (lib/spectroplot.js:241); lookup(cmaps, name) || cube1_cmap (:252-264)
    if (window_name) *window_name = sphost::window_by_name(window ? window : "");
    int ci = cmap_index(cmap ? cmap : "");
    if (ci < 0) ci = 0;
    if (cmap_key) *cmap_key = spcmap::kEntries[ci].key;
    if (lut_len) *lut_len = spcmap::kEntries[ci].length;
    return SP_OK;
}

extern "C" int sp_render_named(sp_context *ctx, const sp_named_request *nr, const uint8_t *bytes, size_t nbytes, int32_t width,
                               const sp_reply *reply)
{
    return sp_render_named_ex(ctx, nr, SP_DETECTOR_SAMPLE, bytes, nbytes, width, reply);
}

extern "C" int sp_render_named_ex(sp_context *ctx, const sp_named_request *nr, int32_t detector, const uint8_t *bytes, size_t nbytes,
                                  int32_t width, const sp_reply *reply)
{
    if (!ctx || !nr || !reply) return SP_ERR_INVALID_ARG;
    if (detector != SP_DETECTOR_SAMPLE && detector != SP_DETECTOR_PEAK)
        return fail(ctx, SP_ERR_INVALID_ARG, "detector must be SP_DETECTOR_SAMPLE or SP_DETECTOR_PEAK");
    if (nr->n < 1 || sphost::log2_exact(nr->n) < 0) return fail(ctx, SP_ERR_NOT_POW2, "Length is not a power of 2");
    if (nr->n > SP_MAX_N) return fail(ctx, SP_ERR_UNSUPPORTED, "n exceeds SP_MAX_N");
    NamedRequest &nm = ctx->named;
    if (!ctx->cached_plan || !nm.same(*nr)) {
        // the caller's message assembly (lib/spectroplot.js:1113-1146)
        nm.windowc.assign((size_t)nr->n, 0.0);
        double weight = 0.0;
        if (!sphost::window(sphost::window_by_name(NamedRequest::str(nr->window).c_str()), nr->n, nm.windowc.data(), &weight))
            return fail(ctx, SP_ERR_INVALID_ARG, "window");
        nm.block_norm = 1.0 / weight;
        int ci = cmap_index(NamedRequest::str(nr->cmap).c_str());
        if (ci < 0) ci = 0;                                              // cube1 (lib/spectroplot.js:252-264)
        const spcmap::Entry &e = spcmap::kEntries[ci];
        nm.lut.assign(3 * (size_t)e.length, 0);
        cmap_bytes(ci, nm.lut.data());
        for (int k = 0; k < 3; k++) {                                    // ends forced to black / white (:1129-1130)
            nm.lut[(size_t)k] = 0;
            nm.lut[3 * (size_t)(e.length - 1) + (size_t)k] = 255;
        }
        nm.format = NamedRequest::str(nr->format);
        nm.window = NamedRequest::str(nr->window);
        nm.cmap = NamedRequest::str(nr->cmap);
        nm.n = nr->n;
        nm.channel_mode = nr->channel_mode ? 1 : 0;
        nm.waterfall = nr->waterfall ? 1 : 0;
        nm.gain = nr->gain;
        nm.range = nr->range;
    }
    sp_request r{};
    r.format = sphost::parse_format(nm.format.c_str());
    r.n = nr->n;
    r.channel_mode = nr->channel_mode;
    r.waterfall = nr->waterfall;
    r.lut_len = (int32_t)(nm.lut.size() / 3);
    r.detector = detector;
    r.block_norm = nm.block_norm;
    r.gain = nr->gain;
    r.range = nr->range;
    r.windowc = nm.windowc.data();
    r.lut_rgb = nm.lut.data();
    // same names and numbers: sp_render finds the cached plan by value (same arrays), nothing is rebuilt or uploaded
    const int rc = sp_render(ctx, &r, bytes, nbytes, width, reply);
    if (rc) nm.windowc.clear();   // a failed render forgets the identity
    return rc;
}

// ------------------------------------------------------------------------------------------------- batches of captures

// How a batch is rendered with one plan: every item's frames in groups of one size, in one of two launches of k_frames_batch -
// launch 0 with the format's prefetching loader (every frame of the item inside its capture: launch_frames' conditions, per item),
// launch 1 with the generic loaders - or, for a plan k_frames does not cover, item by item through sp_plan_execute's path.
enum BatchLaunch { kBatchPrefetch = 0, kBatchGeneric = 1, kBatchFallback = 2, kBatchEmpty = 3 };
struct BatchWork {
    int gf = 0;                        // frames per group
    int groups[2] = {0, 0};            // groups of launch 0 / 1
    std::vector<int> launch;           // per item: BatchLaunch (kBatchEmpty: width 0, the reply is only cleared)
    std::vector<int32_t> first_group;  // per item: its first group in its launch
    std::vector<int32_t> group_count;
    std::vector<double> stride;        // per item: the kernel's stride (0 for one frame) and whether every frame is inside the capture
    std::vector<int> in_bounds;
};

static void plan_batch(const spfmt::Format &f, int n, int lut_len, bool frames_plan, int cu_count, const size_t *nbytes, const int32_t *widths,
                       int count, BatchWork &w)
{
    w.launch.assign((size_t)count, kBatchFallback);
    w.first_group.assign((size_t)count, 0);
    w.group_count.assign((size_t)count, 0);
    w.stride.assign((size_t)count, 0.0);
    w.in_bounds.assign((size_t)count, 0);
    w.gf = 0;
    w.groups[0] = w.groups[1] = 0;
    int64_t total = 0;
    for (int i = 0; i < count; i++) {
        const spgeo::Geometry g = spgeo::geometry(f, n, nbytes[i], widths[i]);
        w.stride[(size_t)i] = g.stride;
        w.in_bounds[(size_t)i] = g.in_bounds ? 1 : 0;
        total += widths[i] > 0 ? widths[i] : 0;
    }
    spk2::FramesLaunch fl;   // (only the group size: the groups are dealt per item and launch below)
    if (!frames_plan || n > (1 << spk2::kBatchMaxLog2N) || spk2::frames_launch_rule(n, lut_len, total, cu_count, 0, fl)) return;
    const int gf = w.gf = fl.gf;
    for (int i = 0; i < count; i++) {
        const int32_t W = widths[i];
        if (W == 0) {
            w.launch[(size_t)i] = kBatchEmpty;
            continue;
        }
        const int l = spk2::frames_prefetch_width(f.width, w.in_bounds[(size_t)i], w.stride[(size_t)i], W) ? kBatchPrefetch : kBatchGeneric;
        w.launch[(size_t)i] = l;
        w.first_group[(size_t)i] = w.groups[l];
        w.group_count[(size_t)i] = (W + gf - 1) / gf;
        w.groups[l] += w.group_count[(size_t)i];
    }
}

extern "C" int sp_debug_batch_plan(int32_t format, int32_t n, int32_t lut_len, int32_t cu_count, const size_t *nbytes, const int32_t *widths,
                                   int32_t count, int64_t *out, size_t capacity, size_t *used)
{
    if (format < 0 || format >= SP_FMT_COUNT || n < 2 || sphost::log2_exact(n) < 0 || lut_len < 1 || cu_count < 1 || count < 0 || !used
        || (count > 0 && (!nbytes || !widths)))
        return SP_ERR_INVALID_ARG;
    for (int i = 0; i < count; i++)
        if (widths[i] < 0) return SP_ERR_INVALID_ARG;
    BatchWork w;
    plan_batch(spfmt::describe(format), n, lut_len, true, cu_count, nbytes, widths, count, w);
    std::vector<int64_t> v{w.gf, spk2::frames_grid(w.groups[0], cu_count), spk2::frames_grid(w.groups[1], cu_count), w.groups[0], w.groups[1]};
    for (int i = 0; i < count; i++) {
        v.push_back(w.launch[(size_t)i]);
        v.push_back(w.first_group[(size_t)i]);
        v.push_back(w.group_count[(size_t)i]);
    }
    *used = v.size();
    if (v.size() > capacity || !out) return SP_ERR_INVALID_ARG;
    memcpy(out, v.data(), v.size() * 8);
    return SP_OK;
}

static int batch_check_items(sp_context *ctx, const spfmt::Format &f, int n, const sp_batch_item *items, int32_t count, bool device)
{
    for (int i = 0; i < count; i++) {
        const int rc = check_capture(ctx, f, n, items[i].bytes, items[i].nbytes, items[i].width, device ? &items[i].reply : nullptr, "batch item: ");
        if (rc) return rc;
    }
    return SP_OK;
}

extern "C" int sp_plan_execute_batch(sp_plan *plan, const sp_batch_item *items, int32_t count)
{
    if (count < 0 || (!items && count > 0)) return SP_ERR_INVALID_ARG;
    if (!plan) return no_object_status();
    if (count == 0) return SP_OK;
    sp_context *ctx = plan->ctx;
    if (plan->req.detector != SP_DETECTOR_SAMPLE)
        return fail(ctx, SP_ERR_UNSUPPORTED, "sp_plan_execute_batch: the peak detector is not supported in batches (render the items one by one)");
    const int n = plan->req.n;
    int rc = batch_check_items(ctx, plan->fmt, n, items, count, true);
    if (rc) return rc;
    SP_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    rc = refuse_capture(ctx, s, "sp_plan_execute_batch", "");
    if (rc) return rc;
    std::vector<size_t> nb((size_t)count);
    std::vector<int32_t> wd((size_t)count);
    for (int i = 0; i < count; i++) {
        nb[(size_t)i] = items[i].nbytes;
        wd[(size_t)i] = items[i].width;
    }
    BatchWork w;
    plan_batch(plan->fmt, n, plan->req.lut_len, plan_kernel(plan) == kKernelFrames, ctx->cu_count, nb.data(), wd.data(), count, w);
    if (w.gf == 0) {
        // a plan outside k_frames: the items one by one, as sp_plan_execute renders them
        for (int i = 0; i < count; i++) {
            rc = plan_execute_range(plan, items[i].bytes, request_shape(plan, items[i].nbytes, items[i].width), 0, items[i].width, true, true,
                                    &items[i].reply, Picture{Picture::kRgba, items[i].reply.rgba});
            if (rc) return rc;
        }
        return SP_OK;
    }

    // the work list: item records of launch 0, of launch 1, of the empty items (cleared only), then the group -> item maps
    std::vector<int> order;
    for (int l : {kBatchPrefetch, kBatchGeneric, kBatchEmpty})
        for (int i = 0; i < count; i++)
            if (w.launch[(size_t)i] == l) order.push_back(i);
    const size_t nrec = order.size(), rec_bytes = nrec * sizeof(spk2::BatchItem);
    const size_t map_off = (rec_bytes + 15) & ~(size_t)15;
    const size_t total = map_off + ((size_t)w.groups[0] + (size_t)w.groups[1]) * sizeof(int32_t);
    if (ctx->ev_batch) SP_HIP(ctx, hipEventSynchronize(ctx->ev_batch));   // the previous batch's copy has read the page-locked table
    else SP_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_batch, hipEventDisableTiming));
    rc = ctx->batch_host.reserve(total);
    if (!rc) rc = ctx->batch_dev.reserve(total);
    if (rc) return fail(ctx, rc, "sp_plan_execute_batch: out of memory");
    uint8_t *h = (uint8_t *)ctx->batch_host.p;
    spk2::BatchItem *rec = (spk2::BatchItem *)h;
    int32_t *map = (int32_t *)(h + map_off);
    int rec_first[2] = {0, 0};   // the launch's first record
    for (int i = 0; i < count; i++) rec_first[1] += w.launch[(size_t)i] == kBatchPrefetch ? 1 : 0;
    for (size_t r = 0; r < nrec; r++) {
        const int i = order[r];
        const sp_batch_item &it = items[i];
        const int l = w.launch[(size_t)i];
        spk2::BatchItem &b = rec[r];
        b = spk2::BatchItem{};
        b.bytes = (const uint8_t *)it.bytes;
        b.nbytes = (int64_t)it.nbytes;
        b.nelem = (int64_t)(it.nbytes / (size_t)plan->fmt.elem);
        b.stride = w.stride[(size_t)i];
        b.rgba = it.reply.rgba;
        b.gauge_mins = it.reply.gauge_mins;
        b.gauge_maxs = it.reply.gauge_maxs;
        b.gauge_amps = it.reply.gauge_amps;
        b.out_c = (unsigned long long *)it.reply.c_hist;
        b.out_cb = (unsigned long long *)it.reply.cb_hist;
        b.out_minmax = it.reply.dbfs_minmax;
        b.width = it.width;
        b.in_bounds = w.in_bounds[(size_t)i];
        b.rgba_fast = rgba_fast(it.reply.rgba, it.width, n);
        b.first_group = w.first_group[(size_t)i];
        if (l == kBatchEmpty) continue;
        // launch 1's map follows launch 0's; its records are indexed from the launch's own first record
        int32_t *m = map + (l == kBatchGeneric ? w.groups[0] : 0);
        const int32_t local = (int32_t)r - (l == kBatchGeneric ? rec_first[1] : 0);
        for (int32_t g = 0; g < w.group_count[(size_t)i]; g++) m[b.first_group + g] = local;
    }
    uint8_t *d = (uint8_t *)ctx->batch_dev.p;
    // the previous batch's kernels may still read the table - on another stream, if the caller has switched since
    if (ctx->ev_batch_done) SP_HIP(ctx, hipStreamWaitEvent(s, ctx->ev_batch_done, 0));
    else SP_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_batch_done, hipEventDisableTiming));
    SP_HIP(ctx, hipMemcpyAsync(d, h, total, hipMemcpyHostToDevice, s));
    SP_HIP(ctx, hipEventRecord(ctx->ev_batch, s));
    const spk2::BatchItem *d_rec = (const spk2::BatchItem *)d;
    const int32_t *d_map = (const int32_t *)(d + map_off);
    spk::launch_batch_clear(d_rec, (unsigned)nrec, plan->req.lut_len, s);
    SP_HIP(ctx, hipGetLastError());

    spk::FrameArgs a{};
    plan_frame_args(plan, a);
    return timed(ctx, [&]() -> int {
        for (int l = 0; l < 2; l++) {
            if (!w.groups[l]) continue;
            const int r = spk2::launch_frames_batch(a, plan->req.format, plan->d_stage_tw, w.gf, w.groups[l], l == 0 ? plan->fmt.width : 0,
                                                    d_rec + rec_first[l], d_map + (l ? w.groups[0] : 0), ctx->cu_count, ctx->device, s);
            if (r) return fail(ctx, r, "k_frames_batch launch rejected the configuration");
            SP_HIP(ctx, hipGetLastError());
        }
        SP_HIP(ctx, hipEventRecord(ctx->ev_batch_done, s));
        return SP_OK;
    });
}

// sp_render_batch's device memory per sub-batch (captures, images and reply records together); a larger batch is rendered in several
// sub-batches, an item larger than this alone
static constexpr size_t kBatchBudget = (size_t)256 << 20;

extern "C" int sp_render_batch(sp_context *ctx, const sp_request *req, const sp_batch_item *items, int32_t count)
{
    if (count < 0 || (!items && count > 0)) return SP_ERR_INVALID_ARG;
    if (!ctx) return no_object_status();
    int rc = validate_request(ctx, req);
    if (rc) return rc;
    if (req->detector != SP_DETECTOR_SAMPLE)
        return fail(ctx, SP_ERR_UNSUPPORTED, "sp_render_batch: the peak detector is not supported in batches (render the items one by one)");
    const spfmt::Format f = spfmt::describe(req->format);
    rc = batch_check_items(ctx, f, req->n, items, count, false);
    if (rc) return rc;
    if (count == 0) return SP_OK;
    SP_HIP(ctx, hipSetDevice(ctx->device));
    sp_plan *plan = nullptr;
    rc = cached_plan_for(ctx, req, &plan);
    if (rc) return rc;
    size_t uploaded = 0;
    if (plan_kernel(plan) != kKernelFrames) {
        // a plan outside k_frames: item by item through sp_render's path
        for (int i = 0; i < count; i++) {
            rc = render_rgba(plan, (const uint8_t *)items[i].bytes, items[i].nbytes, items[i].width, &items[i].reply, items[i].width, false);
            if (rc) return rc;
            uploaded += ctx->last_upload_bytes;
        }
        ctx->last_upload_bytes = uploaded;
        return SP_OK;
    }
    hipStream_t s = ctx->stream;
    // the staging buffers below may be in use by work still queued (sp_plan_execute_from_host): this request starts behind it
    SP_HIP(ctx, hipStreamSynchronize(s));
    const size_t n = (size_t)req->n;
    auto a16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
    std::vector<sp_batch_item> dev((size_t)count);
    std::vector<size_t> in_off((size_t)count), img_off((size_t)count), rec_off((size_t)count);
    for (int i0 = 0; i0 < count;) {
        // the sub-batch [i0, i1): captures, images and records side by side in the context's staging buffers
        size_t in_sz = 0, img_sz = 0, rec_sz = 0;
        int i1 = i0;
        while (i1 < count) {
            const sp_batch_item &it = items[i1];
            const sphost::ReplyRecord rr{(size_t)req->lut_len, (size_t)it.width};
            const size_t img = it.reply.rgba ? a16(4 * (size_t)it.width * n) : 0;
            if (i1 > i0 && in_sz + img_sz + rec_sz + a16(it.nbytes) + img + a16(rr.bytes()) > kBatchBudget) break;
            in_off[(size_t)i1] = in_sz;
            img_off[(size_t)i1] = img_sz;
            rec_off[(size_t)i1] = rec_sz;
            in_sz += a16(it.nbytes);
            img_sz += img;
            rec_sz += a16(rr.bytes());
            i1++;
        }
        rc = ctx->in_bytes.reserve(in_sz + 16);
        if (!rc) rc = ctx->out_rgba.reserve(img_sz + 16);
        if (!rc) rc = ctx->render_small.reserve(rec_sz + 16);
        if (!rc) rc = ctx->host_small.reserve(rec_sz + 16);
        if (rc) return fail(ctx, rc, "sp_render_batch: out of memory");
        uint8_t *const din = (uint8_t *)ctx->in_bytes.p, *const dimg = (uint8_t *)ctx->out_rgba.p, *const drec = (uint8_t *)ctx->render_small.p;
        hipError_t e = hipSuccess;
        for (int i = i0; i < i1 && e == hipSuccess; i++) {
            const sp_batch_item &it = items[i];
            const sphost::ReplyRecord rr{(size_t)req->lut_len, (size_t)it.width};
            sp_batch_item &di = dev[(size_t)i];
            di = it;
            di.bytes = din + in_off[(size_t)i];
            di.reply = rr.view(drec + rec_off[(size_t)i]);
            di.reply.rgba = it.reply.rgba ? dimg + img_off[(size_t)i] : nullptr;
            if (it.nbytes) e = hipMemcpyAsync(din + in_off[(size_t)i], it.bytes, it.nbytes, hipMemcpyHostToDevice, s);
            uploaded += it.nbytes;
        }
        if (e != hipSuccess) rc = hip_fail(ctx, e, "sp_render_batch upload");
        if (!rc) rc = sp_plan_execute_batch(plan, dev.data() + i0, i1 - i0);
        if (!rc) {
            // the records of the sub-batch come back in one copy, each image in one
            e = hipMemcpyAsync(ctx->host_small.p, drec, rec_sz, hipMemcpyDeviceToHost, s);
            for (int i = i0; i < i1 && e == hipSuccess; i++)
                if (items[i].reply.rgba && items[i].width)
                    e = hipMemcpyAsync(items[i].reply.rgba, dimg + img_off[(size_t)i], 4 * (size_t)items[i].width * n, hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) rc = hip_fail(ctx, e, "sp_render_batch download");
        }
        if (rc) {
            (void)hipStreamSynchronize(s);
            return rc;
        }
        for (int i = i0; i < i1; i++) {
            const sphost::ReplyRecord rr{(size_t)req->lut_len, (size_t)items[i].width};
            const uint8_t *hb = (const uint8_t *)ctx->host_small.p + rec_off[(size_t)i];
            rr.unpack_side(hb, items[i].reply);
            rr.unpack_gauges(hb, items[i].reply);
        }
        i0 = i1;
    }
    ctx->last_upload_bytes = uploaded;
    return SP_OK;
}
