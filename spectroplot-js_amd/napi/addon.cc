// addon.cc — N-API binding of the C ABI (include/spectroplot_hip.h) for Node.js.
//
// The JavaScript class HipWorker (js/hip_worker.js) is what the reference library receives through its
// `workerOrUrl` option (lib/spectroplot.js:100-116); this file only moves typed-array pointers across the
// language boundary.  No compute happens here and there is no fallback: every entry point that needs a device
// throws when the HIP library reports an error.
//
// Exports
//   deviceCount()                                  -> number
//   parseFormat(name)                              -> {id, sampleWidth}
//   window(name, n)                                -> {window: Float64Array, weight}
//   sliceBounds(nbytes, sampleWidth, index, count) -> [begin, end]
//   poolStats()                                    -> {fresh, recycled, recycledPinned, freeBytes, pinnedBytes, pinRefused, keepLimit,
//                                                      pinnedLimit, replyWeightCap} of the reply-image pool
//   cmap(name)                                     -> Uint8Array of r,g,b triples (the reference's map under its lookup rules) or null
//   cmapKeys()                                     -> the reference's colour-map keys in its table order
//   allocBuffer(nbytes)                            -> ArrayBuffer in page-locked host memory (sp_host_alloc): a request whose `buffer`
//                                                     is one of these goes to the device at the full rate of the host link
//   createContext(device)                          -> external handle
//   destroyContext(handle)                         -> releases the device context as soon as no render is in flight on it
//   render(handle, req, cb)   req = {format:int, buffer:ArrayBuffer, n, windowc:Float64Array, block_norm, gain, range,
//                                    lut:Uint8Array, width, channelMode, waterfall}
//       runs sp_render on a libuv worker thread and calls cb(err, {rgba, gauge_mins, gauge_maxs, gauge_amps: ArrayBuffer,
//       c_hist, cB_hist: Float64Array, dBfs_min, dBfs_max}) on the main thread
//   renderSync(handle, req)                        -> the same reply object, synchronously
//   renderTraces(handle, req, cb) / renderTracesSync(handle, req) -> {trace_min, trace_max}: per-bin min / max traces, no image
//   renderPower(handle, req, cb) / renderPowerSync(handle, req) -> {power, width, n}: |X|^2 (or dB) per frame and bin as f64, no image
//   renderMean(handle, req, cb) / renderMeanSync(handle, req) -> {mean, width, n}: the exact mean of |X|^2 over the frames per row (or its dB)
//   renderBandPower(handle, req, cb) / renderBandPowerSync(handle, req) -> {bands, count, width, n}: the exact sum of |X|^2 over bands of
//     rows per frame (or its dB)
//   renderTrack(handle, req, cb) / renderTrackSync(handle, req) -> {rows, peaks, count, width, n}: the strongest row of bands of rows per
//     frame and its |X|^2 (or its dB)
//   renderOccupancy(handle, req, cb) / renderOccupancySync(handle, req) -> {rows, frames, count, width, n}: the frames per row, and the
//     rows per band and frame, whose |X|^2 reaches the row's threshold
//   renderDensity(handle, req, cb) / renderDensitySync(handle, req) -> {density, n, lutLen, width}: the persistence spectrum, a
//       Uint32Array(n * lutLen) of per-row colour-index counts (sp_render_density); the request is renderIndex's
//   renderIndex(handle, req, cb) / renderIndexSync(handle, req)   -> render's reply with `index`, a Uint8Array(width * n) of colour
//                                    indices, in place of `rgba` (sp_render_index); req as for render
//   renderNamed(handle, req, cb) / renderNamedSync(handle, req)   req = {format, window, cmap: strings, buffer, n, gain, range, width,
//                                    channelMode, waterfall}: sp_render_named - the library resolves the names as the reference's caller
//                                    does (lib/spectroplot.js:238-264, 1113-1146) and keeps the plan while they repeat
//   namedResolve(window, cmap)                     -> {window, cmap, lutLength}: what the two option names resolve to (sp_named_resolve)
//   planCreations(handle)                          -> how many plans this context has built (sp_context_plan_creations)
//   createGroup(devices: number[])                 -> external handle of an sp_group: one member context per listed device
//   destroyGroup(handle)                           -> like destroyContext
//   groupRender(handle, req, cb) / groupRenderSync(handle, req)   req as for render, `width` = frames of the WHOLE image, plus
//       `gather`: 'device' (default) | 'host' (sp_group_render_ex); the result carries transport, transportNote and timings:
//       sp_group_render - the caller's sliced render (lib/spectroplot.js:1206-1244) with the strips gathered device to device (RCCL or
//       peer copies) and merged on the root; the reply is the merged result (rgba = the whole image, gauges [width]) plus
//       {sliceWidth, members, transport: 'none' | 'rccl' | 'peer'}
//   renderBatch(handle, req, items, cb) / renderBatchSync(handle, req, items)   req as for render without buffer and width; items =
//       [{buffer: ArrayBuffer, width}]: sp_render_batch, one reply per item shaped as render's
// One render at a time per handle: a second render on a handle whose first is still in flight throws (HipWorker serialises its own).
#include <node_api.h>

#include <chrono>
#include <cmath>

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <mutex>
#include <new>
#include <sys/mman.h>
#include <string>
#include <vector>

#include "../../include/spectroplot_hip.h"

namespace {

#define NAPI_OK(env, call)                                                         \
    do {                                                                           \
        if ((call) != napi_ok) {                                                   \
            napi_throw_error((env), nullptr, "N-API call failed: " #call);        \
            return nullptr;                                                        \
        }                                                                          \
    } while (0)

napi_value throw_status(napi_env env, int status, const char *msg)
{
    std::string m = (msg && *msg) ? msg : sp_status_string(status);
    napi_value err, text, code;
    napi_create_string_utf8(env, m.c_str(), NAPI_AUTO_LENGTH, &text);
    napi_create_error(env, nullptr, text, &err);
    napi_create_int32(env, status, &code);
    napi_set_named_property(env, err, "status", code);
    napi_throw(env, err);
    return nullptr;
}

bool get_named(napi_env env, napi_value obj, const char *name, napi_value *out)
{
    return napi_get_named_property(env, obj, name, out) == napi_ok;
}

double get_double(napi_env env, napi_value obj, const char *name)
{
    napi_value v;
    double d = 0;
    if (get_named(env, obj, name, &v)) napi_get_value_double(env, v, &d);
    return d;
}

bool get_bool(napi_env env, napi_value obj, const char *name)
{
    napi_value v, b;
    bool r = false;
    if (get_named(env, obj, name, &v) && napi_coerce_to_bool(env, v, &b) == napi_ok) napi_get_value_bool(env, b, &r);
    return r;
}

// One device context as JavaScript sees it.  Renders run on libuv worker threads, so the sp_context must outlive every job that
// was queued on it: jobs count themselves in `inflight` (main thread only), destroyContext / the finalizer only mark the
// context closed, and whoever brings the count to zero on a closed context destroys it.
struct Ctx {
    sp_context *c = nullptr;
    sp_group *g = nullptr;    // a group handle instead (createGroup): the renders go to sp_group_render
    int inflight = 0;
    bool closed = false;
    bool collected = false;   // the JS handle is gone: the struct itself may be deleted
};

void ctx_release(Ctx *x)
{
    if (x->closed && x->inflight == 0 && x->c) {
        sp_context_destroy(x->c);
        x->c = nullptr;
    }
    if (x->closed && x->inflight == 0 && x->g) {
        sp_group_destroy(x->g);
        x->g = nullptr;
    }
    if (x->collected && x->inflight == 0) delete x;
}

// Image buffers of replies are recycled: a block that JavaScript has dropped (its ArrayBuffer was collected) serves a later reply
// of the same size.  Fresh memory is the slow part of a reply (the kernel zero-fills every page the copy from the device touches
// for the first time); a recycled block takes the copy at the rate of the host link.  V8 is told the size of every block it
// holds (napi_adjust_external_memory), so dropped replies are collected under memory pressure like any large ArrayBuffer.
// A block that comes round a second time is page-locked (on the worker thread, once): copies into it then run asynchronously at
// the rate of the host link, which is what lets sp_render overlap the image's way back with the samples' way in.
// Limits, each read once from the environment (MiB): SPECTROPLOT_HIP_POOL_KEEP_MB bounds the dropped blocks kept for reuse (default
// 3072), SPECTROPLOT_HIP_POOL_PINNED_MB the page-locked bytes of pool blocks, free or held by JavaScript (default 2048 - ten to twelve
// 64-MiB replies are alive between two collections, and a reply in a block that is not page-locked takes 4.0 instead of 2.7 ms; 0 = never
// page-lock), SPECTROPLOT_HIP_REPLY_WEIGHT_MB what V8 is told a reply weighs at most (below).
inline size_t env_mib(const char *name, size_t dflt_mib)
{
    const char *e = getenv(name);
    if (!e || !*e) return dflt_mib << 20;
    char *end = nullptr;
    const unsigned long long v = strtoull(e, &end, 10);
    return (end && *end == 0) ? (size_t)v << 20 : dflt_mib << 20;
}
enum PinState : int { kUnpinned = 0, kPinned = 1, kPinRefused = 2 };   // kPinRefused: hipHostRegister failed for this block; not retried
struct HostPool {
    struct Block { void *p; size_t size; int pin; };
    std::mutex m;
    std::vector<Block> free_blocks;
    size_t free_bytes = 0, pinned_bytes = 0;
    size_t n_fresh = 0, n_recycled = 0, n_recycled_pinned = 0, n_pin_refused = 0;   // poolStats()
    const size_t keep_bytes = env_mib("SPECTROPLOT_HIP_POOL_KEEP_MB", 3072);
    const size_t pinned_limit = env_mib("SPECTROPLOT_HIP_POOL_PINNED_MB", 2048);
    void *take(size_t size, int *pin)
    {
        *pin = kUnpinned;
        {
            std::unique_lock<std::mutex> g(m);
            for (size_t i = 0; i < free_blocks.size(); i++)
                if (free_blocks[i].size == size) {
                    void *p = free_blocks[i].p;
                    *pin = free_blocks[i].pin;
                    n_recycled++;
                    if (*pin == kPinned) n_recycled_pinned++;
                    free_bytes -= size;
                    free_blocks.erase(free_blocks.begin() + (long)i);
                    const bool try_pin = *pin == kUnpinned && size >= ((size_t)1 << 20) && pinned_bytes + size <= pinned_limit;
                    if (try_pin) pinned_bytes += size;   // reserved under the lock, returned below if the registration fails
                    g.unlock();
                    if (try_pin) {
                        if (sp_host_register(p, size) == SP_OK) *pin = kPinned;
                        else {
                            *pin = kPinRefused;
                            std::lock_guard<std::mutex> g2(m);
                            pinned_bytes -= size;
                            n_pin_refused++;
                        }
                    }
                    return p;
                }
        }
        {
            std::lock_guard<std::mutex> g(m);
            n_fresh++;
        }
        // large blocks on 2 MiB boundaries with transparent huge pages requested: the first touch of a fresh block then costs one
        // fault per 2 MiB instead of one per 4 KiB
        void *p = nullptr;
        const size_t align = size >= ((size_t)4 << 20) ? ((size_t)2 << 20) : 4096;
        if (posix_memalign(&p, align, size ? size : 1) != 0) return nullptr;
#ifdef MADV_HUGEPAGE
        if (align > 4096) (void)madvise(p, size, MADV_HUGEPAGE);
#endif
        return p;
    }
    void give(void *p, size_t size, int pin)
    {
        std::lock_guard<std::mutex> g(m);
        if (free_bytes + size > keep_bytes) {
            if (pin == kPinned) {
                sp_host_unregister(p);
                pinned_bytes -= size;
            }
            free(p);
            return;
        }
        free_blocks.push_back({p, size, pin});
        free_bytes += size;
    }
};
HostPool g_pool;

// What V8 is told a reply image weighs: its size up to 6 MiB.  At full weight a config-2 reply (64 MiB) reaches the collector's
// external-memory limit by itself: one mark-sweep per message (1.2 ms each, `node --trace-gc tools/js_dropin_bench.js`).  Capped at
// 16 MiB (rounds 2-4) the collector still ran about every fourth large reply, and its marking steps land in whatever allocates next:
// 0.25-0.3 ms of an average config-2 message, seen as `_request` taking 280-350 us instead of 40 (tools/js_message_stages.js cfg2,
// profiles/r05_host_path.txt).  At 6 MiB it runs about every tenth reply and the pool holds ten to twelve blocks (0.7 GiB of host
// memory for 64-MiB replies) instead of five or six; the blocks still return by collection only.
// The cap grows with the reply beyond 60 MiB - weight = max(cap, size / 10) - so that the collector still runs about every tenth reply
// whatever a reply weighs: with a flat 6 MiB, ten 2-GiB replies (config 5) would be 20 GiB of garbage before V8 looked.
// SPECTROPLOT_HIP_REPLY_WEIGHT_MB changes the cap (a caller that holds many replies at once can raise it to their real size).
const size_t g_reply_weight_cap = env_mib("SPECTROPLOT_HIP_REPLY_WEIGHT_MB", 6);
inline int64_t reply_weight(size_t size)
{
    const size_t floor_w = size < g_reply_weight_cap ? size : g_reply_weight_cap;
    return (int64_t)(size / 10 > floor_w ? size / 10 : floor_w);
}
struct PoolTag { size_t size; int pin; };
void pool_free_cb(napi_env env, void *data, void *hint)
{
    PoolTag *t = (PoolTag *)hint;
    int64_t total = 0;
    napi_adjust_external_memory(env, -reply_weight(t->size), &total);
    g_pool.give(data, t->size, t->pin);
    delete t;
}

// What every request kind has: the context it runs on, its outcome, and - for an asynchronous one - the work item and the references
// that keep its callback (refs[0]) and whatever the worker thread reads (the handle, the input buffers) alive until the callback.
// A kind adds its parsed request, run() for the worker thread and result() for a job that ended with SP_OK; its destructor gives back
// the buffers that did not go to JavaScript.
struct JobBase {
    Ctx *owner = nullptr;
    int status = SP_OK;
    std::string error;
    napi_async_work work = nullptr;
    std::vector<napi_ref> refs;
    virtual ~JobBase() = default;
    virtual void run() = 0;
    virtual napi_value result(napi_env env) = 0;
};

struct Job;
void run_job(Job *j);
napi_value make_reply(napi_env env, Job *j);

struct Job : JobBase {
    sp_context *ctx = nullptr;
    sp_group *group = nullptr;   // a group handle's job
    int32_t gather = SP_GROUP_GATHER_DEVICE;   // ... and where its strips meet (req.gather: 'device' | 'host')
    std::string transport, note;
    double t_render = 0, t_gather = 0, t_download = 0;
    // where the job's time went on the worker thread (microseconds): reply buffers from the pool, the library call
    double us_take = 0, us_native = 0;
    sp_request req{};
    std::vector<double> window;
    std::vector<uint8_t> lut;
    // a request by option names (renderNamed): the library evaluates taper and colour map itself
    bool named = false;
    std::string nformat, nwindow, ncmap;
    const uint8_t *bytes = nullptr;
    size_t nbytes = 0;
    int32_t width = 0;
    // outputs: the image in a recycled block, the gauges malloc'd; handed to JS as external ArrayBuffers
    uint8_t *rgba = nullptr, *gmin = nullptr, *gmax = nullptr, *gamp = nullptr;
    size_t rgba_size = 0;
    int rgba_pin = kUnpinned;
    std::vector<uint64_t> c_hist, cb_hist;
    double minmax[2] = {0.0, -200.0};
    void run() override { run_job(this); }
    napi_value result(napi_env env) override { return make_reply(env, this); }
    // a checked kind's own request fields, read behind the shared ones (parse_checked); false: it has thrown
    virtual bool parse_own(napi_env, napi_value) { return true; }
    ~Job() override;
};

void free_cb(napi_env, void *data, void *) { free(data); }

std::string get_string(napi_env env, napi_value obj, const char *name)
{
    napi_value v, sv;
    if (!get_named(env, obj, name, &v) || napi_coerce_to_string(env, v, &sv) != napi_ok) return "";
    size_t len = 0;
    napi_get_value_string_utf8(env, sv, nullptr, 0, &len);
    std::string out(len, '\0');
    napi_get_value_string_utf8(env, sv, &out[0], len + 1, &len);
    return out;
}

// `detector` of a request object: absent / undefined = SP_DETECTOR_SAMPLE; otherwise the number 0 or 1 (the JS layer maps the names).
// Read with every status checked - anything else throws, so no request ever renders with a value left over from elsewhere.
bool read_detector(napi_env env, napi_value req, int32_t *out)
{
    *out = SP_DETECTOR_SAMPLE;
    bool has = false;
    napi_value v;
    napi_valuetype t;
    if (napi_has_named_property(env, req, "detector", &has) != napi_ok) {
        napi_throw_type_error(env, nullptr, "request must be an object");
        return false;
    }
    if (!has) return true;
    if (napi_get_named_property(env, req, "detector", &v) != napi_ok || napi_typeof(env, v, &t) != napi_ok) {
        napi_throw_type_error(env, nullptr, "detector could not be read");
        return false;
    }
    if (t == napi_undefined) return true;
    double d = -1;
    if (t != napi_number || napi_get_value_double(env, v, &d) != napi_ok || !(d == SP_DETECTOR_SAMPLE || d == SP_DETECTOR_PEAK)) {
        napi_throw_range_error(env, nullptr, "detector must be 0 (sample) or 1 (peak)");
        return false;
    }
    *out = (int32_t)d;
    return true;
}

bool parse_request(napi_env env, napi_value handle, napi_value req, Job *j, bool named = false)
{
    void *p = nullptr;
    if (napi_get_value_external(env, handle, &p) != napi_ok || !p) {
        napi_throw_type_error(env, nullptr, "context handle expected");
        return false;
    }
    j->owner = (Ctx *)p;
    if (j->owner->closed || (!j->owner->c && !j->owner->g)) {
        napi_throw_error(env, nullptr, "context has been destroyed");
        return false;
    }
    j->ctx = j->owner->c;
    j->group = j->owner->g;
    napi_value v;
    int32_t i32 = 0;
    j->named = named;
    if (named) {
        j->nformat = get_string(env, req, "format");
        j->nwindow = get_string(env, req, "window");
        j->ncmap = get_string(env, req, "cmap");
    } else {
        get_named(env, req, "format", &v); napi_get_value_int32(env, v, &i32); j->req.format = i32;
    }
    get_named(env, req, "n", &v); napi_get_value_int32(env, v, &i32); j->req.n = i32;
    get_named(env, req, "width", &v); napi_get_value_int32(env, v, &i32); j->width = i32;
    if (j->group && get_string(env, req, "gather") == "host") j->gather = SP_GROUP_GATHER_HOST;
    j->req.channel_mode = get_bool(env, req, "channelMode");
    j->req.waterfall = get_bool(env, req, "waterfall");
    if (!read_detector(env, req, &j->req.detector)) return false;
    j->req.block_norm = get_double(env, req, "block_norm");
    j->req.gain = get_double(env, req, "gain");
    j->req.range = get_double(env, req, "range");

    void *data = nullptr;
    size_t len = 0;
    get_named(env, req, "buffer", &v);
    if (napi_get_arraybuffer_info(env, v, &data, &len) != napi_ok) {
        napi_throw_type_error(env, nullptr, "buffer must be an ArrayBuffer");
        return false;
    }
    j->bytes = (const uint8_t *)data;
    j->nbytes = len;
    if (named) {
        int32_t lut_len = 0;
        sp_named_resolve(j->nwindow.c_str(), j->ncmap.c_str(), nullptr, nullptr, &lut_len);   // sizes the reply's c_hist
        j->req.lut_len = lut_len;
        return true;
    }

    napi_typedarray_type tt;
    napi_value ab;
    size_t off = 0;
    get_named(env, req, "windowc", &v);
    if (napi_get_typedarray_info(env, v, &tt, &len, &data, &ab, &off) != napi_ok || tt != napi_float64_array) {
        napi_throw_type_error(env, nullptr, "windowc must be a Float64Array");
        return false;
    }
    j->window.assign((const double *)data, (const double *)data + len);
    get_named(env, req, "lut", &v);
    if (napi_get_typedarray_info(env, v, &tt, &len, &data, &ab, &off) != napi_ok || (tt != napi_uint8_array && tt != napi_uint8_clamped_array)) {
        napi_throw_type_error(env, nullptr, "lut must be a Uint8Array");
        return false;
    }
    j->lut.assign((const uint8_t *)data, (const uint8_t *)data + len);
    j->req.lut_len = (int32_t)(len / 3);
    if ((size_t)j->req.n != j->window.size() && j->req.n > 0 && j->window.size() < (size_t)j->req.n) {
        napi_throw_range_error(env, nullptr, "windowc is shorter than n");
        return false;
    }
    j->req.windowc = j->window.data();
    j->req.lut_rgb = j->lut.data();
    return true;
}

inline double now_us()
{
    return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

void run_job_inner(Job *j);
void run_job(Job *j)
{
    const double t0 = now_us();
    run_job_inner(j);
    j->us_native = now_us() - t0 - j->us_take;
}

void run_job_inner(Job *j)
{
    const double t_take0 = now_us();
    const size_t W = j->width > 0 ? (size_t)j->width : 0, n = j->req.n > 0 ? (size_t)j->req.n : 0;
    j->rgba_size = 4 * W * n + 1;
    j->rgba = (uint8_t *)g_pool.take(j->rgba_size, &j->rgba_pin);
    j->gmin = (uint8_t *)calloc(W + 1, 1);
    j->gmax = (uint8_t *)calloc(W + 1, 1);
    j->gamp = (uint8_t *)calloc(W + 1, 1);
    j->c_hist.assign(j->req.lut_len > 0 ? (size_t)j->req.lut_len : 0, 0);
    j->cb_hist.assign(SP_CB_HIST_SIZE, 0);
    j->us_take = now_us() - t_take0;
    if (!j->rgba || !j->gmin || !j->gmax || !j->gamp) {
        j->status = SP_ERR_NOMEM;
        j->error = "out of host memory";
        return;
    }
    sp_reply r{};
    r.rgba = j->rgba; r.gauge_mins = j->gmin; r.gauge_maxs = j->gmax; r.gauge_amps = j->gamp;
    r.c_hist = j->c_hist.data(); r.cb_hist = j->cb_hist.data(); r.dbfs_minmax = j->minmax;
    if (j->group) {
        j->status = sp_group_render_ex(j->group, &j->req, j->bytes, j->nbytes, j->width, &r, j->gather);
        if (j->status != SP_OK) j->error = sp_group_last_error(j->group);
        // (read here, on the worker thread that owns the group for the duration of the job)
        j->transport = sp_group_transport(j->group);
        j->note = sp_group_transport_note(j->group);
        sp_group_last_timings(j->group, &j->t_render, &j->t_gather, &j->t_download);
        return;
    }
    if (j->named) {
        sp_named_request nr{};
        nr.format = j->nformat.c_str();
        nr.window = j->nwindow.c_str();
        nr.cmap = j->ncmap.c_str();
        nr.n = j->req.n;
        nr.channel_mode = j->req.channel_mode;
        nr.waterfall = j->req.waterfall;
        nr.gain = j->req.gain;
        nr.range = j->req.range;
        j->status = sp_render_named_ex(j->ctx, &nr, j->req.detector, j->bytes, j->nbytes, j->width, &r);
    } else {
        j->status = sp_render(j->ctx, &j->req, j->bytes, j->nbytes, j->width, &r);
    }
    if (j->status != SP_OK) j->error = sp_last_error(j->ctx);
}

napi_value make_reply(napi_env env, Job *j)
{
    const size_t W = j->width > 0 ? (size_t)j->width : 0, n = (size_t)j->req.n;
    napi_value out, v;
    NAPI_OK(env, napi_create_object(env, &out));
    auto put_ab = [&](const char *name, uint8_t *&p, size_t len) {
        napi_value ab;
        if (napi_create_external_arraybuffer(env, p, len, free_cb, nullptr, &ab) == napi_ok) {
            p = nullptr;   // owned by the ArrayBuffer now
            napi_set_named_property(env, out, name, ab);
        }
    };
    {
        napi_value ab;
        PoolTag *tag = new PoolTag{j->rgba_size, j->rgba_pin};
        if (napi_create_external_arraybuffer(env, j->rgba, 4 * W * n, pool_free_cb, tag, &ab) == napi_ok) {
            int64_t total = 0;
            napi_adjust_external_memory(env, reply_weight(j->rgba_size), &total);
            j->rgba = nullptr;
            napi_set_named_property(env, out, "rgba", ab);
        } else {
            delete tag;
        }
    }
    put_ab("gauge_mins", j->gmin, W);
    put_ab("gauge_maxs", j->gmax, W);
    put_ab("gauge_amps", j->gamp, W);
    auto put_hist = [&](const char *name, const std::vector<uint64_t> &h) {
        napi_value ab, ta;
        void *data;
        if (napi_create_arraybuffer(env, h.size() * 8, &data, &ab) != napi_ok) return;
        for (size_t i = 0; i < h.size(); i++) ((double *)data)[i] = (double)h[i];
        napi_create_typedarray(env, napi_float64_array, h.size(), ab, 0, &ta);
        napi_set_named_property(env, out, name, ta);
    };
    put_hist("c_hist", j->c_hist);
    put_hist("cB_hist", j->cb_hist);
    {
        napi_value st;
        napi_create_object(env, &st);
        napi_create_double(env, j->us_take, &v); napi_set_named_property(env, st, "take_us", v);
        napi_create_double(env, j->us_native, &v); napi_set_named_property(env, st, "native_us", v);
        napi_set_named_property(env, out, "stages", st);
    }
    napi_create_double(env, j->minmax[0], &v); napi_set_named_property(env, out, "dBfs_min", v);
    napi_create_double(env, j->minmax[1], &v); napi_set_named_property(env, out, "dBfs_max", v);
    if (j->group) {
        const int members = sp_group_size(j->group);
        napi_create_int32(env, members, &v); napi_set_named_property(env, out, "members", v);
        napi_create_int32(env, members > 0 ? j->width / members : 0, &v); napi_set_named_property(env, out, "sliceWidth", v);
        napi_create_string_utf8(env, j->transport.c_str(), NAPI_AUTO_LENGTH, &v); napi_set_named_property(env, out, "transport", v);
        napi_create_string_utf8(env, j->note.c_str(), NAPI_AUTO_LENGTH, &v); napi_set_named_property(env, out, "transportNote", v);
        napi_value t;
        napi_create_object(env, &t);
        napi_create_double(env, j->t_render, &v); napi_set_named_property(env, t, "render_ms", v);
        napi_create_double(env, j->t_gather, &v); napi_set_named_property(env, t, "gather_ms", v);
        napi_create_double(env, j->t_download, &v); napi_set_named_property(env, t, "download_ms", v);
        napi_set_named_property(env, out, "timings", t);
    }
    return out;
}

Job::~Job()
{
    if (rgba) g_pool.give(rgba, rgba_size, rgba_pin);
    free(gmin); free(gmax); free(gamp);
}

void free_job(napi_env env, JobBase *j)
{
    for (napi_ref r : j->refs) napi_delete_reference(env, r);
    if (j->work) napi_delete_async_work(env, j->work);
    delete j;
}

napi_value make_error(napi_env env, const JobBase *j)
{
    napi_value err, text, code;
    const std::string m = j->error.empty() ? sp_status_string(j->status) : j->error;
    napi_create_string_utf8(env, m.c_str(), NAPI_AUTO_LENGTH, &text);
    napi_create_error(env, nullptr, text, &err);
    napi_create_int32(env, j->status, &code);
    napi_set_named_property(env, err, "status", code);
    return err;
}

// An sp_context is one stream with one set of staging buffers: one request at a time.  HipWorker's promise queue already serialises
// its requests; a second one on a handle whose first is still on a libuv thread is refused here rather than left to race.
bool refuse_in_flight(napi_env env, JobBase *j)
{
    if (j->owner->inflight == 0) return false;
    free_job(env, j);
    napi_throw_error(env, nullptr, "a render is already in flight on this context");
    return true;
}

// A parsed job on the calling thread: its result, or its error thrown.
napi_value run_sync(napi_env env, JobBase *j)
{
    if (refuse_in_flight(env, j)) return nullptr;
    j->owner->inflight++;
    j->run();
    j->owner->inflight--;
    ctx_release(j->owner);
    napi_value out = nullptr;
    if (j->status != SP_OK) napi_throw(env, make_error(env, j));
    else out = j->result(env);
    free_job(env, j);
    return out;
}

void exec_cb(napi_env, void *data) { ((JobBase *)data)->run(); }

void done_cb(napi_env env, napi_status, void *data)
{
    JobBase *j = (JobBase *)data;
    j->owner->inflight--;
    ctx_release(j->owner);
    napi_value cb, global, argv[2], ignored;
    napi_get_reference_value(env, j->refs[0], &cb);
    napi_get_global(env, &global);
    if (j->status != SP_OK) {
        argv[0] = make_error(env, j);
        napi_get_undefined(env, &argv[1]);
    } else {
        napi_get_null(env, &argv[0]);
        argv[1] = j->result(env);
    }
    napi_call_function(env, global, cb, 2, argv, &ignored);
    free_job(env, j);
}

// A parsed job onto a libuv thread.  `keep`: the callback first, then the handle (and with it the Ctx) and the inputs the worker thread
// reads; `name`: the async resource; `could_not`: what is thrown if the job cannot be queued.
napi_value queue_async(napi_env env, JobBase *j, std::initializer_list<napi_value> keep, const char *name, const char *could_not)
{
    if (refuse_in_flight(env, j)) return nullptr;
    bool ok = true;
    for (napi_value v : keep) {
        napi_ref r = nullptr;
        ok = ok && napi_create_reference(env, v, 1, &r) == napi_ok;
        if (r) j->refs.push_back(r);
    }
    napi_value res;
    ok = ok && napi_create_string_utf8(env, name, NAPI_AUTO_LENGTH, &res) == napi_ok;
    ok = ok && napi_create_async_work(env, nullptr, res, exec_cb, done_cb, j, &j->work) == napi_ok;
    if (ok) {
        // counted only once the work is certain to run: done_cb is what takes the count down again
        j->owner->inflight++;
        if (napi_queue_async_work(env, j->work) != napi_ok) {
            j->owner->inflight--;
            ok = false;
        }
    }
    if (!ok) {
        Ctx *owner = j->owner;
        free_job(env, j);          // references, the work item, the buffers
        ctx_release(owner);        // a context closed meanwhile is destroyed here if nothing else holds it
        napi_throw_error(env, nullptr, could_not);
    }
    return nullptr;
}

napi_value render_sync(napi_env env, napi_callback_info info, bool named)
{
    size_t argc = 2;
    napi_value argv[2];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    Job *j = new Job;
    if (!parse_request(env, argv[0], argv[1], j, named)) { free_job(env, j); return nullptr; }
    return run_sync(env, j);
}
napi_value RenderSync(napi_env env, napi_callback_info info) { return render_sync(env, info, false); }
napi_value RenderNamedSync(napi_env env, napi_callback_info info) { return render_sync(env, info, true); }

napi_value render_async(napi_env env, napi_callback_info info, bool named)
{
    size_t argc = 3;
    napi_value argv[3];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    Job *j = new Job;
    if (!parse_request(env, argv[0], argv[1], j, named)) { free_job(env, j); return nullptr; }
    napi_value buf = nullptr;   // (left null, it fails the queueing)
    napi_get_named_property(env, argv[1], "buffer", &buf);
    return queue_async(env, j, {argv[2], argv[0], buf}, "spectroplot_hip.render", "could not queue the render");
}
napi_value Render(napi_env env, napi_callback_info info) { return render_async(env, info, false); }
napi_value RenderNamed(napi_env env, napi_callback_info info) { return render_async(env, info, true); }

// ---- batches: renderBatch(handle, req, [{buffer, width}], cb) / renderBatchSync(handle, req, items) -------------------------------
// req is render's request without buffer and width; every item gets its own reply, shaped as render's (sp_render_batch).  Every
// value is read with its status checked: a missing or non-numeric field throws instead of leaving a stale value behind.
struct BatchJob;
void run_batch(BatchJob *b);
napi_value batch_result(napi_env env, BatchJob *b);

struct BatchJob : JobBase {
    sp_request req{};
    std::vector<double> window;
    std::vector<uint8_t> lut;
    std::vector<Job *> items;
    void run() override { run_batch(this); }
    napi_value result(napi_env env) override { return batch_result(env, this); }
    ~BatchJob() override { for (Job *j : items) delete j; }
};

bool checked_number(napi_env env, napi_value obj, const char *name, double *out)
{
    napi_value v;
    napi_valuetype t;
    if (napi_get_named_property(env, obj, name, &v) != napi_ok || napi_typeof(env, v, &t) != napi_ok || t != napi_number
        || napi_get_value_double(env, v, out) != napi_ok) {
        napi_throw_type_error(env, nullptr, (std::string(name) + " must be a number").c_str());
        return false;
    }
    return true;
}

bool checked_int32(napi_env env, napi_value obj, const char *name, int32_t *out)
{
    double d = 0;
    if (!checked_number(env, obj, name, &d)) return false;
    if (!(d >= -2147483648.0 && d <= 2147483647.0) || d != (double)(int32_t)d) {
        napi_throw_range_error(env, nullptr, (std::string(name) + " must be a 32-bit integer").c_str());
        return false;
    }
    *out = (int32_t)d;
    return true;
}

bool checked_bool(napi_env env, napi_value obj, const char *name, int32_t *out)
{
    napi_value v, b;
    bool r = false;
    if (napi_get_named_property(env, obj, name, &v) != napi_ok || napi_coerce_to_bool(env, v, &b) != napi_ok
        || napi_get_value_bool(env, b, &r) != napi_ok) {
        napi_throw_type_error(env, nullptr, (std::string(name) + " must be a boolean").c_str());
        return false;
    }
    *out = r ? 1 : 0;
    return true;
}

bool parse_batch(napi_env env, napi_value handle, napi_value req, napi_value items, BatchJob *b)
{
    void *p = nullptr;
    if (napi_get_value_external(env, handle, &p) != napi_ok || !p) {
        napi_throw_type_error(env, nullptr, "context handle expected");
        return false;
    }
    b->owner = (Ctx *)p;
    if (b->owner->closed || !b->owner->c) {
        napi_throw_error(env, nullptr, b->owner->g ? "renderBatch takes a context handle, not a group" : "context has been destroyed");
        return false;
    }
    double d = 0;
    if (!checked_int32(env, req, "format", &b->req.format) || !checked_int32(env, req, "n", &b->req.n)) return false;
    if (!checked_bool(env, req, "channelMode", &b->req.channel_mode) || !checked_bool(env, req, "waterfall", &b->req.waterfall)) return false;
    if (!read_detector(env, req, &b->req.detector)) return false;   // (a peak batch is refused by the library: SP_ERR_UNSUPPORTED)
    if (!checked_number(env, req, "block_norm", &b->req.block_norm) || !checked_number(env, req, "gain", &b->req.gain)) return false;
    if (!checked_number(env, req, "range", &d)) return false;
    b->req.range = d;
    napi_value v, ab;
    napi_typedarray_type tt;
    size_t len = 0, off = 0;
    void *data = nullptr;
    if (napi_get_named_property(env, req, "windowc", &v) != napi_ok
        || napi_get_typedarray_info(env, v, &tt, &len, &data, &ab, &off) != napi_ok || tt != napi_float64_array) {
        napi_throw_type_error(env, nullptr, "windowc must be a Float64Array");
        return false;
    }
    if (b->req.n > 0 && len < (size_t)b->req.n) {
        napi_throw_range_error(env, nullptr, "windowc is shorter than n");
        return false;
    }
    b->window.assign((const double *)data, (const double *)data + len);
    if (napi_get_named_property(env, req, "lut", &v) != napi_ok || napi_get_typedarray_info(env, v, &tt, &len, &data, &ab, &off) != napi_ok
        || (tt != napi_uint8_array && tt != napi_uint8_clamped_array)) {
        napi_throw_type_error(env, nullptr, "lut must be a Uint8Array");
        return false;
    }
    b->lut.assign((const uint8_t *)data, (const uint8_t *)data + len);
    b->req.lut_len = (int32_t)(len / 3);
    b->req.windowc = b->window.data();
    b->req.lut_rgb = b->lut.data();
    bool is_array = false;
    uint32_t count = 0;
    if (napi_is_array(env, items, &is_array) != napi_ok || !is_array || napi_get_array_length(env, items, &count) != napi_ok) {
        napi_throw_type_error(env, nullptr, "items must be an array of {buffer, width}");
        return false;
    }
    for (uint32_t k = 0; k < count; k++) {
        napi_value it, buf;
        napi_valuetype t;
        if (napi_get_element(env, items, k, &it) != napi_ok || napi_typeof(env, it, &t) != napi_ok || t != napi_object) {
            napi_throw_type_error(env, nullptr, "items must be an array of {buffer, width}");
            return false;
        }
        Job *j = new Job;
        b->items.push_back(j);
        j->owner = b->owner;
        j->ctx = b->owner->c;
        j->req = b->req;
        if (!checked_int32(env, it, "width", &j->width)) return false;
        if (j->width < 0) {
            napi_throw_range_error(env, nullptr, "width must not be negative");
            return false;
        }
        if (napi_get_named_property(env, it, "buffer", &buf) != napi_ok || napi_get_arraybuffer_info(env, buf, &data, &len) != napi_ok) {
            napi_throw_type_error(env, nullptr, "buffer must be an ArrayBuffer");
            return false;
        }
        j->bytes = (const uint8_t *)data;
        j->nbytes = len;
    }
    return true;
}

void run_batch(BatchJob *b)
{
    std::vector<sp_batch_item> items(b->items.size());
    for (size_t k = 0; k < b->items.size(); k++) {
        Job *j = b->items[k];
        const size_t W = (size_t)j->width, n = (size_t)j->req.n;
        j->rgba_size = 4 * W * n + 1;
        j->rgba = (uint8_t *)g_pool.take(j->rgba_size, &j->rgba_pin);
        j->gmin = (uint8_t *)calloc(W + 1, 1);
        j->gmax = (uint8_t *)calloc(W + 1, 1);
        j->gamp = (uint8_t *)calloc(W + 1, 1);
        j->c_hist.assign(j->req.lut_len > 0 ? (size_t)j->req.lut_len : 0, 0);
        j->cb_hist.assign(SP_CB_HIST_SIZE, 0);
        if (!j->rgba || !j->gmin || !j->gmax || !j->gamp) {
            b->status = SP_ERR_NOMEM;
            b->error = "out of host memory";
            return;
        }
        sp_batch_item &it = items[k];
        it.bytes = j->bytes;
        it.nbytes = j->nbytes;
        it.width = j->width;
        it.reply.rgba = j->rgba; it.reply.gauge_mins = j->gmin; it.reply.gauge_maxs = j->gmax; it.reply.gauge_amps = j->gamp;
        it.reply.c_hist = j->c_hist.data(); it.reply.cb_hist = j->cb_hist.data(); it.reply.dbfs_minmax = j->minmax;
    }
    b->status = sp_render_batch(b->owner->c, &b->req, items.data(), (int32_t)items.size());
    if (b->status != SP_OK) b->error = sp_last_error(b->owner->c);
}

napi_value batch_result(napi_env env, BatchJob *b)
{
    napi_value arr;
    if (napi_create_array_with_length(env, b->items.size(), &arr) != napi_ok) return nullptr;
    for (size_t k = 0; k < b->items.size(); k++) {
        napi_value r = make_reply(env, b->items[k]);
        if (!r || napi_set_element(env, arr, (uint32_t)k, r) != napi_ok) return nullptr;
    }
    return arr;
}

napi_value RenderBatchSync(napi_env env, napi_callback_info info)
{
    size_t argc = 3;
    napi_value argv[3];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    if (argc < 3) {
        napi_throw_type_error(env, nullptr, "renderBatchSync(handle, request, items)");
        return nullptr;
    }
    BatchJob *b = new BatchJob;
    if (!parse_batch(env, argv[0], argv[1], argv[2], b)) { free_job(env, b); return nullptr; }
    return run_sync(env, b);
}

napi_value RenderBatch(napi_env env, napi_callback_info info)
{
    size_t argc = 4;
    napi_value argv[4];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    napi_valuetype t = napi_undefined;
    if (argc < 4 || napi_typeof(env, argv[3], &t) != napi_ok || t != napi_function) {
        napi_throw_type_error(env, nullptr, "renderBatch(handle, request, items, callback)");
        return nullptr;
    }
    BatchJob *b = new BatchJob;
    if (!parse_batch(env, argv[0], argv[1], argv[2], b)) { free_job(env, b); return nullptr; }
    // (the items array keeps their buffers alive)
    return queue_async(env, b, {argv[3], argv[0], argv[2]}, "spectroplot_hip.renderBatch", "could not queue the batch");
}

// ---- checked requests: traces, indexed images, persistence spectrum ----------------------------------------------------------------------
// Every value of such a request is read into a variable of its own with its status checked, as for a batch: a request that cannot be
// read throws and never renders.  What differs between the kinds: the names in their texts, and whether the request carries a picture
// (`waterfall`, `detector`, `lut`); one without gets the sample detector and a 2-entry map (the plan wants one).
struct CheckedKind {
    const char *who;   // in "<who> takes a context handle, not a group"
    bool picture;
    const char *sync_usage, *async_usage, *resource, *could_not_queue;
};

bool parse_checked(napi_env env, napi_value handle, napi_value req, Job *t, const CheckedKind &kind)
{
    void *p = nullptr;
    if (napi_get_value_external(env, handle, &p) != napi_ok || !p) {
        napi_throw_type_error(env, nullptr, "context handle expected");
        return false;
    }
    t->owner = (Ctx *)p;
    if (t->owner->closed || !t->owner->c) {
        napi_throw_error(env, nullptr, t->owner->g ? (std::string(kind.who) + " takes a context handle, not a group").c_str() : "context has been destroyed");
        return false;
    }
    t->ctx = t->owner->c;
    if (!checked_int32(env, req, "format", &t->req.format) || !checked_int32(env, req, "n", &t->req.n)) return false;
    if (!checked_int32(env, req, "width", &t->width)) return false;
    if (!checked_bool(env, req, "channelMode", &t->req.channel_mode)) return false;
    t->req.detector = SP_DETECTOR_SAMPLE;
    if (kind.picture && (!checked_bool(env, req, "waterfall", &t->req.waterfall) || !read_detector(env, req, &t->req.detector))) return false;
    if (!checked_number(env, req, "block_norm", &t->req.block_norm) || !checked_number(env, req, "gain", &t->req.gain)) return false;
    if (!checked_number(env, req, "range", &t->req.range)) return false;
    if (t->req.n < 1 || t->width < 0) {
        napi_throw_range_error(env, nullptr, "n must be positive and width must not be negative");
        return false;
    }
    napi_value v_win, v_lut, v_buf, ab_win, ab_lut;
    napi_typedarray_type tt_win, tt_lut;
    size_t len_win = 0, off_win = 0, len_lut = 0, off_lut = 0, len_buf = 0;
    void *data_win = nullptr, *data_lut = nullptr, *data_buf = nullptr;
    if (napi_get_named_property(env, req, "windowc", &v_win) != napi_ok
        || napi_get_typedarray_info(env, v_win, &tt_win, &len_win, &data_win, &ab_win, &off_win) != napi_ok || tt_win != napi_float64_array) {
        napi_throw_type_error(env, nullptr, "windowc must be a Float64Array");
        return false;
    }
    if (len_win < (size_t)t->req.n) {
        napi_throw_range_error(env, nullptr, "windowc is shorter than n");
        return false;
    }
    t->window.assign((const double *)data_win, (const double *)data_win + len_win);
    t->lut = {0, 0, 0, 255, 255, 255};   // (a request without a picture has no colours; the plan wants a map)
    if (kind.picture) {
        if (napi_get_named_property(env, req, "lut", &v_lut) != napi_ok
            || napi_get_typedarray_info(env, v_lut, &tt_lut, &len_lut, &data_lut, &ab_lut, &off_lut) != napi_ok
            || (tt_lut != napi_uint8_array && tt_lut != napi_uint8_clamped_array) || len_lut < 3) {
            napi_throw_type_error(env, nullptr, "lut must be a Uint8Array of r, g, b triples");
            return false;
        }
        t->lut.assign((const uint8_t *)data_lut, (const uint8_t *)data_lut + len_lut);
    }
    if (napi_get_named_property(env, req, "buffer", &v_buf) != napi_ok || napi_get_arraybuffer_info(env, v_buf, &data_buf, &len_buf) != napi_ok) {
        napi_throw_type_error(env, nullptr, "buffer must be an ArrayBuffer");
        return false;
    }
    t->bytes = (const uint8_t *)data_buf;
    t->nbytes = len_buf;
    t->req.lut_len = (int32_t)(t->lut.size() / 3);
    t->req.windowc = t->window.data();
    t->req.lut_rgb = t->lut.data();
    return true;
}

// The entry pair of a checked kind whose job is a J: <kind>Sync(handle, req) and <kind>(handle, req, cb).
template <typename J>
napi_value checked_sync(napi_env env, napi_callback_info info, const CheckedKind &kind)
{
    size_t argc = 2;
    napi_value argv[2];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    if (argc < 2) {
        napi_throw_type_error(env, nullptr, kind.sync_usage);
        return nullptr;
    }
    J *t = new J;
    if (!parse_checked(env, argv[0], argv[1], t, kind) || !t->parse_own(env, argv[1])) { free_job(env, t); return nullptr; }
    return run_sync(env, t);
}

template <typename J>
napi_value checked_async(napi_env env, napi_callback_info info, const CheckedKind &kind)
{
    size_t argc = 3;
    napi_value argv[3];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    napi_valuetype ty = napi_undefined;
    if (argc < 3 || napi_typeof(env, argv[2], &ty) != napi_ok || ty != napi_function) {
        napi_throw_type_error(env, nullptr, kind.async_usage);
        return nullptr;
    }
    J *t = new J;
    if (!parse_checked(env, argv[0], argv[1], t, kind) || !t->parse_own(env, argv[1])) { free_job(env, t); return nullptr; }
    napi_value buf = nullptr;   // (left null, it fails the queueing)
    napi_get_named_property(env, argv[1], "buffer", &buf);
    return queue_async(env, t, {argv[2], argv[0], buf}, kind.resource, kind.could_not_queue);
}

// ---- traces: renderTraces(handle, req, cb) / renderTracesSync(handle, req) ---------------------------------------------------------
// req: {format, n, width, channelMode, block_norm, gain, range, windowc, buffer} -> {trace_min, trace_max}, two Float64Array(n) in image
// row order (sp_render_traces).
const CheckedKind kTraces{"renderTraces", false, "renderTracesSync(handle, request)", "renderTraces(handle, request, callback)",
                          "spectroplot_hip.renderTraces", "could not queue the traces request"};

struct TracesJob : Job {
    std::vector<double> out;   // trace_min, then trace_max
    void run() override;
    napi_value result(napi_env env) override;
};

void TracesJob::run()
{
    const size_t n = (size_t)req.n;
    out.assign(2 * n, 0.0);
    status = sp_render_traces(ctx, &req, bytes, nbytes, width, out.data(), out.data() + n);
    if (status != SP_OK) error = sp_last_error(ctx);
}

napi_value TracesJob::result(napi_env env)
{
    const size_t n = (size_t)req.n;
    napi_value obj, ab, ta;
    void *data = nullptr;
    if (napi_create_object(env, &obj) != napi_ok || napi_create_arraybuffer(env, 2 * n * 8, &data, &ab) != napi_ok) return nullptr;
    memcpy(data, out.data(), 2 * n * 8);
    if (napi_create_typedarray(env, napi_float64_array, n, ab, 0, &ta) != napi_ok || napi_set_named_property(env, obj, "trace_min", ta) != napi_ok)
        return nullptr;
    if (napi_create_typedarray(env, napi_float64_array, n, ab, n * 8, &ta) != napi_ok || napi_set_named_property(env, obj, "trace_max", ta) != napi_ok)
        return nullptr;
    return obj;
}

napi_value RenderTracesSync(napi_env env, napi_callback_info info) { return checked_sync<TracesJob>(env, info, kTraces); }
napi_value RenderTraces(napi_env env, napi_callback_info info) { return checked_async<TracesJob>(env, info, kTraces); }

// ---- indexed images: renderIndex(handle, req, cb) / renderIndexSync(handle, req) -------------------------------------------------------
// req as for render plus `detector` -> render's reply with `index` - a Uint8Array(width * n), one colour-index byte per pixel in the RGBA
// image's pixel order, in a page-locked block of the reply pool - in place of `rgba` (sp_render_index).
const CheckedKind kIndex{"renderIndex", true, "renderIndexSync(handle, request)", "renderIndex(handle, request, callback)",
                         "spectroplot_hip.renderIndex", "could not queue the indexed request"};

struct IndexJob : Job {
    void run() override;
    napi_value result(napi_env env) override;
};

void IndexJob::run()
{
    const size_t W = (size_t)width, n = (size_t)req.n;
    rgba_size = W * n + 1;                                   // (Job's image block: here one byte per pixel)
    rgba = (uint8_t *)g_pool.take(rgba_size, &rgba_pin);
    gmin = (uint8_t *)calloc(W + 1, 1);
    gmax = (uint8_t *)calloc(W + 1, 1);
    gamp = (uint8_t *)calloc(W + 1, 1);
    c_hist.assign((size_t)req.lut_len, 0);
    cb_hist.assign(SP_CB_HIST_SIZE, 0);
    if (!rgba || !gmin || !gmax || !gamp) {
        status = SP_ERR_NOMEM;
        error = "out of host memory";
        return;
    }
    sp_reply r{};
    r.gauge_mins = gmin; r.gauge_maxs = gmax; r.gauge_amps = gamp;
    r.c_hist = c_hist.data(); r.cb_hist = cb_hist.data(); r.dbfs_minmax = minmax;
    status = sp_render_index(ctx, &req, bytes, nbytes, width, &r, rgba);
    if (status != SP_OK) error = sp_last_error(ctx);
}

napi_value IndexJob::result(napi_env env)
{
    const size_t W = (size_t)width, n = (size_t)req.n;
    napi_value out, ab, ta, v;
    if (napi_create_object(env, &out) != napi_ok) return nullptr;
    PoolTag *tag = new PoolTag{rgba_size, rgba_pin};
    if (napi_create_external_arraybuffer(env, rgba, W * n, pool_free_cb, tag, &ab) != napi_ok) {
        delete tag;
        return nullptr;
    }
    int64_t total = 0;
    napi_adjust_external_memory(env, reply_weight(rgba_size), &total);
    rgba = nullptr;   // owned by the ArrayBuffer now
    if (napi_create_typedarray(env, napi_uint8_array, W * n, ab, 0, &ta) != napi_ok || napi_set_named_property(env, out, "index", ta) != napi_ok)
        return nullptr;
    const auto put_gauge = [&](const char *name, uint8_t *&p) {
        napi_value gab;
        if (napi_create_external_arraybuffer(env, p, W, free_cb, nullptr, &gab) != napi_ok) return false;
        p = nullptr;
        return napi_set_named_property(env, out, name, gab) == napi_ok;
    };
    if (!put_gauge("gauge_mins", gmin) || !put_gauge("gauge_maxs", gmax) || !put_gauge("gauge_amps", gamp)) return nullptr;
    const auto put_hist = [&](const char *name, const std::vector<uint64_t> &h) {
        napi_value hab, hta;
        void *data = nullptr;
        if (napi_create_arraybuffer(env, h.size() * 8, &data, &hab) != napi_ok) return false;
        for (size_t i = 0; i < h.size(); i++) ((double *)data)[i] = (double)h[i];
        return napi_create_typedarray(env, napi_float64_array, h.size(), hab, 0, &hta) == napi_ok
               && napi_set_named_property(env, out, name, hta) == napi_ok;
    };
    if (!put_hist("c_hist", c_hist) || !put_hist("cB_hist", cb_hist)) return nullptr;
    if (napi_create_double(env, minmax[0], &v) != napi_ok || napi_set_named_property(env, out, "dBfs_min", v) != napi_ok) return nullptr;
    if (napi_create_double(env, minmax[1], &v) != napi_ok || napi_set_named_property(env, out, "dBfs_max", v) != napi_ok) return nullptr;
    return out;
}

napi_value RenderIndexSync(napi_env env, napi_callback_info info) { return checked_sync<IndexJob>(env, info, kIndex); }
napi_value RenderIndex(napi_env env, napi_callback_info info) { return checked_async<IndexJob>(env, info, kIndex); }

// ---- persistence spectrum: renderDensity(handle, req, cb) / renderDensitySync(handle, req) ----------------------------------------------
// req as for renderIndex -> {density, n, lutLen, width}: density a Uint32Array(n * lutLen), row y at y * lutLen - how many of the
// request's frames showed colour index g in image row y (sp_render_density).
const CheckedKind kDensity{"renderDensity", true, "renderDensitySync(handle, request)", "renderDensity(handle, request, callback)",
                           "spectroplot_hip.renderDensity", "could not queue the density request"};

struct DensityJob : IndexJob {
    std::vector<uint32_t> counts;
    void run() override;
    napi_value result(napi_env env) override;
};

void DensityJob::run()
{
    // (a map the library refuses gets no array: its n * lut_len could be anything)
    if (req.lut_len >= 1 && req.lut_len <= 256) {
        try {
            counts.assign((size_t)req.n * (size_t)req.lut_len, 0u);
        } catch (const std::bad_alloc &) {
            status = SP_ERR_NOMEM;
            error = "out of host memory";
            return;
        }
    }
    uint32_t none = 0;
    status = sp_render_density(ctx, &req, bytes, nbytes, width, counts.empty() ? &none : counts.data());
    if (status != SP_OK) error = sp_last_error(ctx);
}

napi_value DensityJob::result(napi_env env)
{
    napi_value out, ab, ta, v;
    void *data = nullptr;
    if (napi_create_object(env, &out) != napi_ok || napi_create_arraybuffer(env, counts.size() * 4, &data, &ab) != napi_ok) return nullptr;
    memcpy(data, counts.data(), counts.size() * 4);
    if (napi_create_typedarray(env, napi_uint32_array, counts.size(), ab, 0, &ta) != napi_ok || napi_set_named_property(env, out, "density", ta) != napi_ok)
        return nullptr;
    if (napi_create_int32(env, req.n, &v) != napi_ok || napi_set_named_property(env, out, "n", v) != napi_ok) return nullptr;
    if (napi_create_int32(env, req.lut_len, &v) != napi_ok || napi_set_named_property(env, out, "lutLen", v) != napi_ok) return nullptr;
    if (napi_create_int32(env, width, &v) != napi_ok || napi_set_named_property(env, out, "width", v) != napi_ok) return nullptr;
    return out;
}

napi_value RenderDensitySync(napi_env env, napi_callback_info info) { return checked_sync<DensityJob>(env, info, kDensity); }
napi_value RenderDensity(napi_env env, napi_callback_info info) { return checked_async<DensityJob>(env, info, kDensity); }

// ---- power plane: renderPower(handle, req, cb) / renderPowerSync(handle, req) ----------------------------------------------------------
// req as for renderTraces plus `db` (boolean) -> {power, width, n}: power a Float64Array(width * n), frame-major - |X|^2 of frame x at
// image row y in power[x * n + y], or its dB plane with db - in a page-locked block of the reply pool (sp_render_power).
const CheckedKind kPower{"renderPower", false, "renderPowerSync(handle, request)", "renderPower(handle, request, callback)",
                         "spectroplot_hip.renderPower", "could not queue the power request"};

struct PowerJob : Job {
    int32_t db = 0;
    bool parse_own(napi_env env, napi_value r) override { return checked_bool(env, r, "db", &db); }
    void run() override;
    napi_value result(napi_env env) override;
};

void PowerJob::run()
{
    const size_t W = (size_t)width, n = (size_t)req.n;
    rgba_size = W * n * sizeof(double) + 8;                  // (Job's image block: here one f64 per frame and bin)
    rgba = (uint8_t *)g_pool.take(rgba_size, &rgba_pin);
    if (!rgba) {
        status = SP_ERR_NOMEM;
        error = "out of host memory";
        return;
    }
    status = sp_render_power(ctx, &req, bytes, nbytes, width, db, (double *)rgba);
    if (status != SP_OK) error = sp_last_error(ctx);
}

napi_value PowerJob::result(napi_env env)
{
    const size_t W = (size_t)width, n = (size_t)req.n;
    napi_value out, ab, ta, v;
    if (napi_create_object(env, &out) != napi_ok) return nullptr;
    PoolTag *tag = new PoolTag{rgba_size, rgba_pin};
    if (napi_create_external_arraybuffer(env, rgba, W * n * sizeof(double), pool_free_cb, tag, &ab) != napi_ok) {
        delete tag;
        return nullptr;
    }
    int64_t total = 0;
    napi_adjust_external_memory(env, reply_weight(rgba_size), &total);
    rgba = nullptr;   // owned by the ArrayBuffer now
    if (napi_create_typedarray(env, napi_float64_array, W * n, ab, 0, &ta) != napi_ok || napi_set_named_property(env, out, "power", ta) != napi_ok)
        return nullptr;
    if (napi_create_int32(env, width, &v) != napi_ok || napi_set_named_property(env, out, "width", v) != napi_ok) return nullptr;
    if (napi_create_int32(env, req.n, &v) != napi_ok || napi_set_named_property(env, out, "n", v) != napi_ok) return nullptr;
    return out;
}

napi_value RenderPowerSync(napi_env env, napi_callback_info info) { return checked_sync<PowerJob>(env, info, kPower); }
napi_value RenderPower(napi_env env, napi_callback_info info) { return checked_async<PowerJob>(env, info, kPower); }

// ---- exact mean-power trace: renderMean(handle, req, cb) / renderMeanSync(handle, req) -------------------------------------------------
// req as for renderPower -> {mean, width, n}: mean a Float64Array(n) in image row order - the correctly rounded sum of |X|^2 over the
// request's frames divided by width, or the dB of it with db (sp_render_mean).
const CheckedKind kMean{"renderMean", false, "renderMeanSync(handle, request)", "renderMean(handle, request, callback)",
                        "spectroplot_hip.renderMean", "could not queue the mean request"};

struct MeanJob : PowerJob {
    std::vector<double> out;
    void run() override;
    napi_value result(napi_env env) override;
};

void MeanJob::run()
{
    out.assign((size_t)req.n, 0.0);
    status = sp_render_mean(ctx, &req, bytes, nbytes, width, db, out.data());
    if (status != SP_OK) error = sp_last_error(ctx);
}

napi_value MeanJob::result(napi_env env)
{
    const size_t n = (size_t)req.n;
    napi_value obj, ab, ta, v;
    void *data = nullptr;
    if (napi_create_object(env, &obj) != napi_ok || napi_create_arraybuffer(env, n * 8, &data, &ab) != napi_ok) return nullptr;
    memcpy(data, out.data(), n * 8);
    if (napi_create_typedarray(env, napi_float64_array, n, ab, 0, &ta) != napi_ok || napi_set_named_property(env, obj, "mean", ta) != napi_ok)
        return nullptr;
    if (napi_create_int32(env, width, &v) != napi_ok || napi_set_named_property(env, obj, "width", v) != napi_ok) return nullptr;
    if (napi_create_int32(env, req.n, &v) != napi_ok || napi_set_named_property(env, obj, "n", v) != napi_ok) return nullptr;
    return obj;
}

napi_value RenderMeanSync(napi_env env, napi_callback_info info) { return checked_sync<MeanJob>(env, info, kMean); }
napi_value RenderMean(napi_env env, napi_callback_info info) { return checked_async<MeanJob>(env, info, kMean); }

// ---- exact band-power series: renderBandPower(handle, req, cb) / renderBandPowerSync(handle, req) -------------------------------------
// req as for renderPower plus `bands`, an Int32Array of y0, y1 pairs (half-open ranges of image rows) -> {bands, count, width, n}:
// bands a Float64Array(count * width), band-major - per band and frame the correctly rounded sum of |X|^2 over the band's rows, or the
// dB of it with db (sp_render_bandpower).  The library refuses bad bands (status -1) before anything is rendered.
const CheckedKind kBandPower{"renderBandPower", false, "renderBandPowerSync(handle, request)", "renderBandPower(handle, request, callback)",
                             "spectroplot_hip.renderBandPower", "could not queue the band-power request"};

struct BandPowerJob : PowerJob {
    std::vector<int32_t> rows;   // y0, y1 per band
    std::vector<double> out;
    bool parse_own(napi_env env, napi_value r) override;
    void run() override;
    napi_value result(napi_env env) override;
};

bool BandPowerJob::parse_own(napi_env env, napi_value r)
{
    if (!PowerJob::parse_own(env, r)) return false;
    napi_value v, ab;
    napi_typedarray_type tt;
    size_t len = 0, off = 0;
    void *data = nullptr;
    if (napi_get_named_property(env, r, "bands", &v) != napi_ok || napi_get_typedarray_info(env, v, &tt, &len, &data, &ab, &off) != napi_ok
        || tt != napi_int32_array || len % 2 != 0) {
        napi_throw_type_error(env, nullptr, "bands must be an Int32Array of y0, y1 pairs");
        return false;
    }
    if (len) rows.assign((const int32_t *)data, (const int32_t *)data + len);
    return true;
}

void BandPowerJob::run()
{
    const size_t count = rows.size() / 2;
    if (count <= SP_MAX_BANDS) {   // (more bands than the library takes get no array: it refuses them)
        try {
            out.assign(count * (size_t)width, 0.0);
        } catch (const std::bad_alloc &) {
            status = SP_ERR_NOMEM;
            error = "out of host memory";
            return;
        }
    }
    double none = 0;
    const int32_t c = count > (size_t)SP_MAX_BANDS ? SP_MAX_BANDS + 1 : (int32_t)count;
    status = sp_render_bandpower(ctx, &req, bytes, nbytes, width, rows.data(), c, db, out.empty() ? &none : out.data());
    if (status != SP_OK) error = sp_last_error(ctx);
}

napi_value BandPowerJob::result(napi_env env)
{
    napi_value obj, ab, ta, v;
    void *data = nullptr;
    if (napi_create_object(env, &obj) != napi_ok || napi_create_arraybuffer(env, out.size() * 8, &data, &ab) != napi_ok) return nullptr;
    if (!out.empty()) memcpy(data, out.data(), out.size() * 8);
    if (napi_create_typedarray(env, napi_float64_array, out.size(), ab, 0, &ta) != napi_ok || napi_set_named_property(env, obj, "bands", ta) != napi_ok)
        return nullptr;
    if (napi_create_int32(env, (int32_t)(rows.size() / 2), &v) != napi_ok || napi_set_named_property(env, obj, "count", v) != napi_ok) return nullptr;
    if (napi_create_int32(env, width, &v) != napi_ok || napi_set_named_property(env, obj, "width", v) != napi_ok) return nullptr;
    if (napi_create_int32(env, req.n, &v) != napi_ok || napi_set_named_property(env, obj, "n", v) != napi_ok) return nullptr;
    return obj;
}

napi_value RenderBandPowerSync(napi_env env, napi_callback_info info) { return checked_sync<BandPowerJob>(env, info, kBandPower); }
napi_value RenderBandPower(napi_env env, napi_callback_info info) { return checked_async<BandPowerJob>(env, info, kBandPower); }

// ---- peak track: renderTrack(handle, req, cb) / renderTrackSync(handle, req) -------------------------------------------------------------
// req as for renderBandPower -> {rows, peaks, count, width, n}: rows an Int32Array(count * width) and peaks a Float64Array(count * width),
// band-major - per band and frame the strongest image row that is not a NaN (the smallest among equal ones, -1 where there is none) and
// its |X|^2 (NaN where there is none), or the dB of it with db (sp_render_track).  The library refuses bad bands (status -1) before
// anything is rendered.
const CheckedKind kTrack{"renderTrack", false, "renderTrackSync(handle, request)", "renderTrack(handle, request, callback)",
                         "spectroplot_hip.renderTrack", "could not queue the track request"};

struct TrackJob : BandPowerJob {   // (`rows` are the bands, `out` the peaks)
    std::vector<int32_t> best;     // the strongest row per band and frame
    void run() override;
    napi_value result(napi_env env) override;
};

void TrackJob::run()
{
    const size_t count = rows.size() / 2;
    if (count <= SP_MAX_BANDS) {   // (more bands than the library takes get no arrays: it refuses them)
        try {
            out.assign(count * (size_t)width, 0.0);
            best.assign(count * (size_t)width, 0);
        } catch (const std::bad_alloc &) {
            status = SP_ERR_NOMEM;
            error = "out of host memory";
            return;
        }
    }
    double none = 0;
    int32_t no_row = 0;
    const int32_t c = count > (size_t)SP_MAX_BANDS ? SP_MAX_BANDS + 1 : (int32_t)count;
    status = sp_render_track(ctx, &req, bytes, nbytes, width, rows.data(), c, db, best.empty() ? &no_row : best.data(), out.empty() ? &none : out.data());
    if (status != SP_OK) error = sp_last_error(ctx);
}

napi_value TrackJob::result(napi_env env)
{
    napi_value obj, ab, ta, v;
    void *data = nullptr;
    if (napi_create_object(env, &obj) != napi_ok || napi_create_arraybuffer(env, best.size() * 4, &data, &ab) != napi_ok) return nullptr;
    if (!best.empty()) memcpy(data, best.data(), best.size() * 4);
    if (napi_create_typedarray(env, napi_int32_array, best.size(), ab, 0, &ta) != napi_ok || napi_set_named_property(env, obj, "rows", ta) != napi_ok)
        return nullptr;
    if (napi_create_arraybuffer(env, out.size() * 8, &data, &ab) != napi_ok) return nullptr;
    if (!out.empty()) memcpy(data, out.data(), out.size() * 8);
    if (napi_create_typedarray(env, napi_float64_array, out.size(), ab, 0, &ta) != napi_ok || napi_set_named_property(env, obj, "peaks", ta) != napi_ok)
        return nullptr;
    if (napi_create_int32(env, (int32_t)(rows.size() / 2), &v) != napi_ok || napi_set_named_property(env, obj, "count", v) != napi_ok) return nullptr;
    if (napi_create_int32(env, width, &v) != napi_ok || napi_set_named_property(env, obj, "width", v) != napi_ok) return nullptr;
    if (napi_create_int32(env, req.n, &v) != napi_ok || napi_set_named_property(env, obj, "n", v) != napi_ok) return nullptr;
    return obj;
}

napi_value RenderTrackSync(napi_env env, napi_callback_info info) { return checked_sync<TrackJob>(env, info, kTrack); }
napi_value RenderTrack(napi_env env, napi_callback_info info) { return checked_async<TrackJob>(env, info, kTrack); }

// ---- occupancy counts: renderOccupancy(handle, req, cb) / renderOccupancySync(handle, req) ------------------------------------------------
// req as for renderBandPower (db is not looked at) plus `threshold`, a Float64Array(n): one power per image row -> {rows, frames, count,
// width, n}: rows a Uint32Array(n) - per image row the frames whose |X|^2 is >= the row's threshold - and frames a
// Uint32Array(count * width), band-major - per band and frame the rows of the band that reach theirs (sp_render_occupancy; a NaN on
// either side is no hit).  The library refuses bad bands, and a threshold of another length is refused here (status -1), before
// anything is rendered.
const CheckedKind kOccupancy{"renderOccupancy", false, "renderOccupancySync(handle, request)", "renderOccupancy(handle, request, callback)",
                             "spectroplot_hip.renderOccupancy", "could not queue the occupancy request"};

struct OccupancyJob : BandPowerJob {   // (`rows` are the bands; `out` is not used)
    std::vector<double> threshold;
    std::vector<uint32_t> row_counts, frame_counts;
    bool parse_own(napi_env env, napi_value r) override;
    void run() override;
    napi_value result(napi_env env) override;
};

bool OccupancyJob::parse_own(napi_env env, napi_value r)
{
    if (!BandPowerJob::parse_own(env, r)) return false;
    napi_value v, ab;
    napi_typedarray_type tt;
    size_t len = 0, off = 0;
    void *data = nullptr;
    if (napi_get_named_property(env, r, "threshold", &v) != napi_ok || napi_get_typedarray_info(env, v, &tt, &len, &data, &ab, &off) != napi_ok
        || tt != napi_float64_array) {
        napi_throw_type_error(env, nullptr, "threshold must be a Float64Array of n powers");
        return false;
    }
    if (len) threshold.assign((const double *)data, (const double *)data + len);
    return true;
}

void OccupancyJob::run()
{
    const size_t count = rows.size() / 2;
    if (req.n < 1 || threshold.size() != (size_t)req.n) {
        status = SP_ERR_INVALID_ARG;
        error = "threshold must hold n values, one per image row";
        return;
    }
    try {
        row_counts.assign((size_t)req.n, 0);
        if (count <= SP_MAX_BANDS && width > 0) frame_counts.assign(count * (size_t)width, 0);   // (more bands than the library takes: it refuses)
    } catch (const std::bad_alloc &) {
        status = SP_ERR_NOMEM;
        error = "out of host memory";
        return;
    }
    uint32_t none = 0;
    const int32_t c = count > (size_t)SP_MAX_BANDS ? SP_MAX_BANDS + 1 : (int32_t)count;
    status = sp_render_occupancy(ctx, &req, bytes, nbytes, width, threshold.data(), rows.data(), c, row_counts.data(),
                                 frame_counts.empty() ? &none : frame_counts.data());
    if (status != SP_OK) error = sp_last_error(ctx);
}

napi_value OccupancyJob::result(napi_env env)
{
    napi_value obj, ab, ta, v;
    void *data = nullptr;
    if (napi_create_object(env, &obj) != napi_ok || napi_create_arraybuffer(env, row_counts.size() * 4, &data, &ab) != napi_ok) return nullptr;
    if (!row_counts.empty()) memcpy(data, row_counts.data(), row_counts.size() * 4);
    if (napi_create_typedarray(env, napi_uint32_array, row_counts.size(), ab, 0, &ta) != napi_ok
        || napi_set_named_property(env, obj, "rows", ta) != napi_ok)
        return nullptr;
    if (napi_create_arraybuffer(env, frame_counts.size() * 4, &data, &ab) != napi_ok) return nullptr;
    if (!frame_counts.empty()) memcpy(data, frame_counts.data(), frame_counts.size() * 4);
    if (napi_create_typedarray(env, napi_uint32_array, frame_counts.size(), ab, 0, &ta) != napi_ok
        || napi_set_named_property(env, obj, "frames", ta) != napi_ok)
        return nullptr;
    if (napi_create_int32(env, (int32_t)(rows.size() / 2), &v) != napi_ok || napi_set_named_property(env, obj, "count", v) != napi_ok) return nullptr;
    if (napi_create_int32(env, width, &v) != napi_ok || napi_set_named_property(env, obj, "width", v) != napi_ok) return nullptr;
    if (napi_create_int32(env, req.n, &v) != napi_ok || napi_set_named_property(env, obj, "n", v) != napi_ok) return nullptr;
    return obj;
}

napi_value RenderOccupancySync(napi_env env, napi_callback_info info) { return checked_sync<OccupancyJob>(env, info, kOccupancy); }
napi_value RenderOccupancy(napi_env env, napi_callback_info info) { return checked_async<OccupancyJob>(env, info, kOccupancy); }

napi_value DeviceCount(napi_env env, napi_callback_info)
{
    int32_t c = 0;
    sp_device_count(&c);
    napi_value v;
    napi_create_int32(env, c, &v);
    return v;
}

napi_value ParseFormat(napi_env env, napi_callback_info info)
{
    size_t argc = 1;
    napi_value argv[1], s;
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    NAPI_OK(env, napi_coerce_to_string(env, argv[0], &s));
    char buf[64];
    size_t len = 0;
    napi_get_value_string_utf8(env, s, buf, sizeof buf, &len);
    int32_t id = 0, sw = 0;
    sp_format_parse(buf, &id, &sw);
    napi_value out, v;
    napi_create_object(env, &out);
    napi_create_int32(env, id, &v); napi_set_named_property(env, out, "id", v);
    napi_create_int32(env, sw, &v); napi_set_named_property(env, out, "sampleWidth", v);
    napi_create_int32(env, sp_format_element_size(id), &v); napi_set_named_property(env, out, "elementSize", v);
    return out;
}

napi_value Window(napi_env env, napi_callback_info info)
{
    size_t argc = 2;
    napi_value argv[2];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    char name[64];
    size_t len = 0;
    int32_t n = 0;
    napi_get_value_string_utf8(env, argv[0], name, sizeof name, &len);
    napi_get_value_int32(env, argv[1], &n);
    if (n < 1) return throw_status(env, SP_ERR_INVALID_ARG, "n must be positive");
    napi_value ab, ta, out, w;
    void *data;
    NAPI_OK(env, napi_create_arraybuffer(env, (size_t)n * 8, &data, &ab));
    double weight = 0;
    const int rc = sp_window(name, n, (double *)data, &weight);
    if (rc) return throw_status(env, rc, "unknown window name");
    napi_create_typedarray(env, napi_float64_array, (size_t)n, ab, 0, &ta);
    napi_create_object(env, &out);
    napi_set_named_property(env, out, "window", ta);
    napi_create_double(env, weight, &w);
    napi_set_named_property(env, out, "weight", w);
    return out;
}

napi_value SliceBounds(napi_env env, napi_callback_info info)
{
    size_t argc = 4;
    napi_value argv[4];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    double nbytes = 0;
    int32_t sw = 0, index = 0, count = 0;
    napi_get_value_double(env, argv[0], &nbytes);
    napi_get_value_int32(env, argv[1], &sw);
    napi_get_value_int32(env, argv[2], &index);
    napi_get_value_int32(env, argv[3], &count);
    size_t b = 0, e = 0;
    const int rc = sp_slice_bounds((size_t)nbytes, sw, index, count, &b, &e);
    if (rc) return throw_status(env, rc, nullptr);
    napi_value out, v;
    napi_create_array_with_length(env, 2, &out);
    napi_create_double(env, (double)b, &v); napi_set_element(env, out, 0, v);
    napi_create_double(env, (double)e, &v); napi_set_element(env, out, 1, v);
    return out;
}

// bandRows(n, fLo, fHi) -> [y0, y1]: sp_band_rows, the image rows whose centre frequency lies in [fLo, fHi] cycles per sample
napi_value BandRows(napi_env env, napi_callback_info info)
{
    size_t argc = 3;
    napi_value argv[3];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    int32_t n = 0, y0 = 0, y1 = 0;
    double lo = 0, hi = 0;
    if (argc < 3 || napi_get_value_int32(env, argv[0], &n) != napi_ok || napi_get_value_double(env, argv[1], &lo) != napi_ok
        || napi_get_value_double(env, argv[2], &hi) != napi_ok) {
        napi_throw_type_error(env, nullptr, "bandRows(n, fLo, fHi): three numbers expected");
        return nullptr;
    }
    const int rc = sp_band_rows(n, lo, hi, &y0, &y1);
    if (rc) return throw_status(env, rc, "bandRows: n must be a power of two >= 2 and fLo <= fHi");
    napi_value out, v;
    NAPI_OK(env, napi_create_array_with_length(env, 2, &out));
    NAPI_OK(env, napi_create_int32(env, y0, &v));
    NAPI_OK(env, napi_set_element(env, out, 0, v));
    NAPI_OK(env, napi_create_int32(env, y1, &v));
    NAPI_OK(env, napi_set_element(env, out, 1, v));
    return out;
}

void ctx_finalize(napi_env, void *data, void *)
{
    Ctx *x = (Ctx *)data;
    x->closed = true;
    x->collected = true;
    ctx_release(x);
}

napi_value DestroyContext(napi_env env, napi_callback_info info)
{
    size_t argc = 1;
    napi_value argv[1];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    void *p = nullptr;
    if (napi_get_value_external(env, argv[0], &p) != napi_ok || !p) {
        napi_throw_type_error(env, nullptr, "context handle expected");
        return nullptr;
    }
    Ctx *x = (Ctx *)p;
    x->closed = true;
    ctx_release(x);
    napi_value v;
    napi_get_boolean(env, x->c == nullptr && x->g == nullptr, &v);    // true: released now; false: a render is still in flight, released when it ends
    return v;
}

napi_value CreateGroup(napi_env env, napi_callback_info info)
{
    size_t argc = 1;
    napi_value argv[1];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    uint32_t len = 0;
    bool is_array = false;
    if (argc < 1 || napi_is_array(env, argv[0], &is_array) != napi_ok || !is_array || napi_get_array_length(env, argv[0], &len) != napi_ok || len < 1) {
        napi_throw_type_error(env, nullptr, "createGroup: a non-empty array of device indices expected");
        return nullptr;
    }
    std::vector<int32_t> devices(len);
    for (uint32_t i = 0; i < len; i++) {
        napi_value e;
        napi_get_element(env, argv[0], i, &e);
        napi_get_value_int32(env, e, &devices[i]);
    }
    sp_group *g = nullptr;
    const int rc = sp_group_create(devices.data(), (int32_t)len, &g);
    if (rc) return throw_status(env, rc, rc == SP_ERR_NO_DEVICE ? "no HIP device: spectroplot-hip has no CPU fallback" : nullptr);
    Ctx *x = new Ctx;
    x->g = g;
    napi_value ext;
    if (napi_create_external(env, x, ctx_finalize, nullptr, &ext) != napi_ok) {
        sp_group_destroy(g);
        delete x;
        napi_throw_error(env, nullptr, "napi_create_external failed");
        return nullptr;
    }
    return ext;
}

void pinned_free_cb(napi_env env, void *data, void *hint)
{
    int64_t total = 0;
    napi_adjust_external_memory(env, -(int64_t)(size_t)hint, &total);
    sp_host_free(data);
}

napi_value AllocBuffer(napi_env env, napi_callback_info info)
{
    size_t argc = 1;
    napi_value argv[1];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    double nbytes = 0;
    napi_get_value_double(env, argv[0], &nbytes);
    if (!(nbytes >= 0) || nbytes > 4e12) return throw_status(env, SP_ERR_INVALID_ARG, "allocBuffer: bad size");
    void *p = nullptr;
    const int rc = sp_host_alloc((size_t)nbytes, &p);
    if (rc) return throw_status(env, rc, rc == SP_ERR_NO_DEVICE ? "no HIP device: spectroplot-hip has no CPU fallback" : "page-locked allocation failed");
    napi_value ab;
    if (napi_create_external_arraybuffer(env, p, (size_t)nbytes, pinned_free_cb, (void *)(size_t)nbytes, &ab) != napi_ok) {
        sp_host_free(p);
        napi_throw_error(env, nullptr, "napi_create_external_arraybuffer failed");
        return nullptr;
    }
    int64_t total = 0;
    napi_adjust_external_memory(env, (int64_t)nbytes, &total);
    return ab;
}

napi_value PoolStats(napi_env env, napi_callback_info)
{
    napi_value out, v;
    napi_create_object(env, &out);
    std::lock_guard<std::mutex> g(g_pool.m);
    napi_create_double(env, (double)g_pool.n_fresh, &v); napi_set_named_property(env, out, "fresh", v);
    napi_create_double(env, (double)g_pool.n_recycled, &v); napi_set_named_property(env, out, "recycled", v);
    napi_create_double(env, (double)g_pool.n_recycled_pinned, &v); napi_set_named_property(env, out, "recycledPinned", v);
    napi_create_double(env, (double)g_pool.free_bytes, &v); napi_set_named_property(env, out, "freeBytes", v);
    napi_create_double(env, (double)g_pool.pinned_bytes, &v); napi_set_named_property(env, out, "pinnedBytes", v);
    napi_create_double(env, (double)g_pool.n_pin_refused, &v); napi_set_named_property(env, out, "pinRefused", v);
    napi_create_double(env, (double)g_pool.keep_bytes, &v); napi_set_named_property(env, out, "keepLimit", v);
    napi_create_double(env, (double)g_pool.pinned_limit, &v); napi_set_named_property(env, out, "pinnedLimit", v);
    napi_create_double(env, (double)g_reply_weight_cap, &v); napi_set_named_property(env, out, "replyWeightCap", v);
    return out;
}

napi_value Cmap(napi_env env, napi_callback_info info)
{
    size_t argc = 1;
    napi_value argv[1], sname;
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    NAPI_OK(env, napi_coerce_to_string(env, argv[0], &sname));
    char name[96];
    size_t len = 0;
    napi_get_value_string_utf8(env, sname, name, sizeof name, &len);
    int32_t entries = 0;
    napi_value out;
    if (sp_cmap(name, nullptr, 0, &entries) == SP_ERR_UNSUPPORTED) {
        napi_get_null(env, &out);
        return out;
    }
    napi_value ab;
    void *data;
    NAPI_OK(env, napi_create_arraybuffer(env, 3 * (size_t)entries, &data, &ab));
    sp_cmap(name, (uint8_t *)data, entries, &entries);
    NAPI_OK(env, napi_create_typedarray(env, napi_uint8_array, 3 * (size_t)entries, ab, 0, &out));
    return out;
}

napi_value CmapKeys(napi_env env, napi_callback_info)
{
    napi_value out, v;
    const int n = sp_cmap_count();
    napi_create_array_with_length(env, (size_t)n, &out);
    for (int i = 0; i < n; i++) {
        napi_create_string_utf8(env, sp_cmap_key(i), NAPI_AUTO_LENGTH, &v);
        napi_set_element(env, out, (uint32_t)i, v);
    }
    return out;
}

napi_value NamedResolve(napi_env env, napi_callback_info info)
{
    size_t argc = 2;
    napi_value argv[2], out, v, sv;
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    std::string names[2];
    for (int k = 0; k < 2; k++) {
        size_t len = 0;
        NAPI_OK(env, napi_coerce_to_string(env, argv[k], &sv));
        napi_get_value_string_utf8(env, sv, nullptr, 0, &len);
        names[k].assign(len, '\0');
        napi_get_value_string_utf8(env, sv, &names[k][0], len + 1, &len);
    }
    const char *wname = "", *ckey = "";
    int32_t lut_len = 0;
    sp_named_resolve(names[0].c_str(), names[1].c_str(), &wname, &ckey, &lut_len);
    NAPI_OK(env, napi_create_object(env, &out));
    napi_create_string_utf8(env, wname, NAPI_AUTO_LENGTH, &v); napi_set_named_property(env, out, "window", v);
    napi_create_string_utf8(env, ckey, NAPI_AUTO_LENGTH, &v); napi_set_named_property(env, out, "cmap", v);
    napi_create_int32(env, lut_len, &v); napi_set_named_property(env, out, "lutLength", v);
    return out;
}

// peakSubframes(formatId, n, nbytes, width) -> {subframes, lastColumnCount}: sp_peak_subframes, every argument checked
napi_value PeakSubframes(napi_env env, napi_callback_info info)
{
    size_t argc = 4;
    napi_value argv[4], out, v;
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    double a[4] = {0, 0, 0, 0};
    for (int k = 0; k < 4; k++) {
        napi_valuetype t;
        if (argc < 4 || napi_typeof(env, argv[k], &t) != napi_ok || t != napi_number || napi_get_value_double(env, argv[k], &a[k]) != napi_ok
            || !(a[k] >= 0 && a[k] <= 9007199254740992.0) || a[k] != std::floor(a[k])) {
            napi_throw_type_error(env, nullptr, "peakSubframes(formatId, n, nbytes, width): non-negative integers expected");
            return nullptr;
        }
    }
    if (a[0] > 2147483647.0 || a[1] > 2147483647.0 || a[3] > 2147483647.0) return throw_status(env, SP_ERR_INVALID_ARG, nullptr);
    int32_t m = 1, last = 0;
    const int rc = sp_peak_subframes((int32_t)a[0], (int32_t)a[1], (size_t)a[2], (int32_t)a[3], &m, &last);
    if (rc) return throw_status(env, rc, nullptr);
    NAPI_OK(env, napi_create_object(env, &out));
    napi_create_int32(env, m, &v); napi_set_named_property(env, out, "subframes", v);
    napi_create_int32(env, last, &v); napi_set_named_property(env, out, "lastColumnCount", v);
    return out;
}

napi_value PlanCreations(napi_env env, napi_callback_info info)
{
    size_t argc = 1;
    napi_value argv[1], v;
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    void *p = nullptr;
    if (napi_get_value_external(env, argv[0], &p) != napi_ok || !p || !((Ctx *)p)->c) {
        napi_throw_type_error(env, nullptr, "context handle expected");
        return nullptr;
    }
    int64_t n = 0;
    sp_context_plan_creations(((Ctx *)p)->c, &n);
    NAPI_OK(env, napi_create_int64(env, n, &v));
    return v;
}

napi_value CreateContext(napi_env env, napi_callback_info info)
{
    size_t argc = 1;
    napi_value argv[1];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    int32_t dev = 0;
    if (argc >= 1) napi_get_value_int32(env, argv[0], &dev);
    sp_context *ctx = nullptr;
    const int rc = sp_context_create(dev, &ctx);
    if (rc) return throw_status(env, rc, rc == SP_ERR_NO_DEVICE ? "no HIP device: spectroplot-hip has no CPU fallback" : nullptr);
    Ctx *x = new Ctx;
    x->c = ctx;
    napi_value ext;
    if (napi_create_external(env, x, ctx_finalize, nullptr, &ext) != napi_ok) {
        sp_context_destroy(ctx);
        delete x;
        napi_throw_error(env, nullptr, "napi_create_external failed");
        return nullptr;
    }
    return ext;
}

napi_value Init(napi_env env, napi_value exports)
{
    const napi_property_descriptor props[] = {
        {"deviceCount", nullptr, DeviceCount, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"parseFormat", nullptr, ParseFormat, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"window", nullptr, Window, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"sliceBounds", nullptr, SliceBounds, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"createContext", nullptr, CreateContext, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"destroyContext", nullptr, DestroyContext, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"allocBuffer", nullptr, AllocBuffer, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"poolStats", nullptr, PoolStats, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"cmap", nullptr, Cmap, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"cmapKeys", nullptr, CmapKeys, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"render", nullptr, Render, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"renderSync", nullptr, RenderSync, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"renderNamed", nullptr, RenderNamed, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"renderNamedSync", nullptr, RenderNamedSync, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"renderBatch", nullptr, RenderBatch, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"renderBatchSync", nullptr, RenderBatchSync, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"renderTraces", nullptr, RenderTraces, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"renderTracesSync", nullptr, RenderTracesSync, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"renderPower", nullptr, RenderPower, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"renderPowerSync", nullptr, RenderPowerSync, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"renderMean", nullptr, RenderMean, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"renderMeanSync", nullptr, RenderMeanSync, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"bandRows", nullptr, BandRows, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"renderBandPower", nullptr, RenderBandPower, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"renderBandPowerSync", nullptr, RenderBandPowerSync, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"renderTrack", nullptr, RenderTrack, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"renderTrackSync", nullptr, RenderTrackSync, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"renderOccupancy", nullptr, RenderOccupancy, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"renderOccupancySync", nullptr, RenderOccupancySync, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"renderIndex", nullptr, RenderIndex, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"renderIndexSync", nullptr, RenderIndexSync, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"renderDensity", nullptr, RenderDensity, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"renderDensitySync", nullptr, RenderDensitySync, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"namedResolve", nullptr, NamedResolve, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"peakSubframes", nullptr, PeakSubframes, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"planCreations", nullptr, PlanCreations, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"createGroup", nullptr, CreateGroup, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"destroyGroup", nullptr, DestroyContext, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"groupRender", nullptr, Render, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"groupRenderSync", nullptr, RenderSync, nullptr, nullptr, nullptr, napi_default, nullptr},
    };
    napi_define_properties(env, exports, sizeof props / sizeof props[0], props);
    napi_value v;
    napi_create_int32(env, sp_version(), &v);
    napi_set_named_property(env, exports, "version", v);
    return exports;
}

}  // namespace

NAPI_MODULE(NODE_GYP_MODULE_NAME, Init)
