// addon.cc — N-API binding of the C ABI (include/spectroplot_hip.h) for Node.js.
//
// The JavaScript class HipWorker (js/hip_worker.js) is what the reference library receives through its
// `workerOrUrl` option (lib/spectroplot.js:100-116); this file only moves typed-array pointers across the
// language boundary.  No compute happens here and there is no fallback: every entry point that needs a device
// throws when the HIP library reports an error.
//
// Exports: every name of Init's table, once (the sections below have the detail)
//   deviceCount()                                  -> number
//   parseFormat(name)                              -> {id, sampleWidth, elementSize}
//   window(name, n)                                -> {window: Float64Array, weight}
//   sliceBounds(nbytes, sampleWidth, index, count) -> [begin, end]
//   bandRows(n, fLo, fHi)                          -> [y0, y1]: the image rows whose centre frequency lies in the band (sp_band_rows)
//   peakSubframes(formatId, n, nbytes, width)      -> {subframes, lastColumnCount} (sp_peak_subframes)
//   cmap(name)                                     -> Uint8Array of r,g,b triples (the reference's map under its lookup rules) or null
//   cmapKeys()                                     -> the reference's colour-map keys in its table order
//   namedResolve(window, cmap)                     -> {window, cmap, lutLength}: what the two option names resolve to (sp_named_resolve)
//   poolStats()                                    -> {fresh, recycled, recycledPinned, freeBytes, pinnedBytes, pinRefused, keepLimit,
//                                                      pinnedLimit, replyWeightCap} of the reply-image pool
//   allocBuffer(nbytes)                            -> ArrayBuffer in page-locked host memory (sp_host_alloc): a request whose `buffer`
//                                                     is one of these goes to the device at the full rate of the host link
//   createContext(device)                          -> external handle
//   destroyContext(handle)                         -> releases the device context as soon as no render is in flight on it
//   planCreations(handle)                          -> how many plans this context has built (sp_context_plan_creations)
//   createGroup(devices: number[])                 -> external handle of an sp_group: one member context per listed device
//   destroyGroup(handle)                           -> like destroyContext
// The render entry points come in pairs: name(handle, req, cb) runs the library call on a libuv worker thread and calls cb(err, reply) on
// the main thread; nameSync(handle, req) returns the same reply or throws.  An error of the library carries its `status`.
//   render / renderSync              req = {format: int, buffer: ArrayBuffer, n, windowc: Float64Array, block_norm, gain, range,
//                                    lut: Uint8Array, width, channelMode, waterfall, detector} -> {rgba, gauge_mins, gauge_maxs,
//                                    gauge_amps: ArrayBuffer, c_hist, cB_hist: Float64Array, stages, dBfs_min, dBfs_max} (sp_render)
//   renderNamed / renderNamedSync    req = {format, window, cmap: strings, buffer, n, gain, range, width, channelMode, waterfall,
//                                    detector} -> render's reply (sp_render_named: the library resolves the names as the reference's
//                                    caller does, lib/spectroplot.js:238-264, 1113-1146, and keeps the plan while they repeat)
//   groupRender / groupRenderSync    a group handle; req as for render, `width` = frames of the WHOLE image, plus gather: 'device'
//                                    (default) | 'host' -> render's reply for the merged image plus {members, sliceWidth, transport:
//                                    'none' | 'rccl' | 'peer', transportNote, timings} (sp_group_render_ex: the caller's sliced render,
//                                    lib/spectroplot.js:1206-1244, with the strips gathered device to device and merged on the root)
//   renderBatch / renderBatchSync    (handle, req, items[, cb]): req as for render without buffer and width, items = [{buffer, width}]
//                                    -> one reply per item shaped as render's (sp_render_batch)
//   renderTraces / ...Sync           req without a picture -> {trace_min, trace_max}: per-bin min / max traces
//   renderIndex / ...Sync            req as for render -> render's reply with `index`, a Uint8Array(width * n), in place of `rgba`
//   renderDensity / ...Sync          req as for render -> {density: Uint32Array(n * lutLen), n, lutLen, width}: the persistence spectrum
//   renderPower / ...Sync            req without a picture plus db -> {power: Float64Array(width * n), width, n}: |X|^2 or its dB
//   renderMean / ...Sync             req as for renderPower -> {mean: Float64Array(n), width, n}: the exact mean of |X|^2 per row
//   renderBandPower / ...Sync        req as for renderPower plus bands -> {bands: Float64Array(count * width), count, width, n}
//   renderTrack / ...Sync            req as for renderBandPower -> {rows: Int32Array, peaks: Float64Array, count, width, n}
//   renderOccupancy / ...Sync        req as for renderBandPower plus threshold -> {rows, frames: Uint32Array, count, width, n}
// and `version`, the library's (sp_version), a number.
// One render at a time per handle: a second render on a handle whose first is still in flight throws (HipWorker serialises its own).
#include <node_api.h>

#include <chrono>
#include <cmath>

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <initializer_list>
#include <mutex>
#include <new>
#include <sys/mman.h>
#include <string>
#include <utility>
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
// the buffers that did not go to JavaScript.  The ways a run() ends are here: refused before the library was asked, out of host memory,
// and the library call's status with the context's error text.
struct JobBase {
    Ctx *owner = nullptr;
    int status = SP_OK;
    std::string error;
    napi_async_work work = nullptr;
    std::vector<napi_ref> refs;
    virtual ~JobBase() = default;
    virtual void run() = 0;
    virtual napi_value result(napi_env env) = 0;

    void refuse(int code, const char *why) { status = code; error = why; }
    void no_memory() { refuse(SP_ERR_NOMEM, "out of host memory"); }
    // the job's reply arrays: false, and the job out of memory, if they cannot be had
    template <typename F> bool allocated(F &&assign)
    {
        try {
            assign();
            return true;
        } catch (const std::bad_alloc &) {
            no_memory();
            return false;
        }
    }
    // (a job's context stays the owner's while the job is counted in `inflight`)
    void finish(int rc)
    {
        status = rc;
        if (status != SP_OK) error = sp_last_error(owner->c);
    }
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


inline double now_us()
{
    return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
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

// ---- readers: what the request parsers below share; each returns false (or null) once it has thrown --------------------------------
// The Ctx behind a handle.  `who`: the entry point that takes contexts only, named in its refusal of a group; null: a group will do.
Ctx *read_handle(napi_env env, napi_value handle, const char *who)
{
    void *p = nullptr;
    if (napi_get_value_external(env, handle, &p) != napi_ok || !p) {
        napi_throw_type_error(env, nullptr, "context handle expected");
        return nullptr;
    }
    Ctx *x = (Ctx *)p;
    if (!x->closed && (x->c || (x->g && !who))) return x;
    napi_throw_error(env, nullptr, who && x->g ? (std::string(who) + " takes a context handle, not a group").c_str() : "context has been destroyed");
    return nullptr;
}

// The samples of one request and how many frames are wanted of them
struct Capture {
    const uint8_t *bytes = nullptr;
    size_t nbytes = 0;
    int32_t width = 0;
};

bool read_buffer(napi_env env, napi_value obj, Capture *c)
{
    napi_value v;
    void *data = nullptr;
    if (napi_get_named_property(env, obj, "buffer", &v) != napi_ok || napi_get_arraybuffer_info(env, v, &data, &c->nbytes) != napi_ok) {
        napi_throw_type_error(env, nullptr, "buffer must be an ArrayBuffer");
        return false;
    }
    c->bytes = (const uint8_t *)data;
    return true;
}

// A typed-array property copied into `out`: of one of `types`, at least `min_len` elements and a multiple of `multiple`, or `refusal` is
// thrown as a TypeError.
template <typename T>
bool read_array(napi_env env, napi_value obj, const char *name, std::initializer_list<napi_typedarray_type> types, const char *refusal,
                std::vector<T> *out, size_t min_len = 0, size_t multiple = 1)
{
    napi_value v, ab;
    napi_typedarray_type tt;
    size_t len = 0, off = 0;
    void *data = nullptr;
    bool ok = napi_get_named_property(env, obj, name, &v) == napi_ok && napi_get_typedarray_info(env, v, &tt, &len, &data, &ab, &off) == napi_ok;
    bool of_type = false;
    for (napi_typedarray_type t : types) of_type = of_type || (ok && tt == t);
    if (!of_type || len < min_len || len % multiple != 0) {
        napi_throw_type_error(env, nullptr, refusal);
        return false;
    }
    out->assign((const T *)data, (const T *)data + len);
    return true;
}

// What a request asks of the library, with the taper and the colour map it points into
struct Settings {
    sp_request req{};
    std::vector<double> window;
    std::vector<uint8_t> lut;
    void bind()
    {
        req.lut_len = (int32_t)(lut.size() / 3);
        req.windowc = window.data();
        req.lut_rgb = lut.data();
    }
};

bool read_windowc(napi_env env, napi_value req, Settings *s)
{
    return read_array(env, req, "windowc", {napi_float64_array}, "windowc must be a Float64Array", &s->window);
}

bool window_covers_n(napi_env env, const Settings &s)
{
    if (s.req.n <= 0 || s.window.size() >= (size_t)s.req.n) return true;
    napi_throw_range_error(env, nullptr, "windowc is shorter than n");
    return false;
}

bool read_lut(napi_env env, napi_value req, Settings *s, size_t min_len, const char *refusal)
{
    return read_array(env, req, "lut", {napi_uint8_array, napi_uint8_clamped_array}, refusal, &s->lut, min_len);
}

// ... and the three that only some checked kinds have
bool read_db(napi_env env, napi_value req, int32_t *db) { return checked_bool(env, req, "db", db); }

// The bands of a request, y0 and y1 per band (half-open ranges of image rows), and what the library is given for them: a count beyond
// SP_MAX_BANDS is refused there, so the kinds allocate no arrays for it and SP_MAX_BANDS + 1 stands for any such count.
struct Bands {
    std::vector<int32_t> rows;
    size_t count() const { return rows.size() / 2; }
    bool taken() const { return count() <= (size_t)SP_MAX_BANDS; }
    int32_t for_library() const { return taken() ? (int32_t)count() : SP_MAX_BANDS + 1; }
};
// ... and an array that was deliberately not allocated, for a request the library refuses before it writes: one element to point at
template <typename T> T *or_placeholder(std::vector<T> &v, T *none) { return v.empty() ? none : v.data(); }

bool read_bands(napi_env env, napi_value req, Bands *b)
{
    return read_array(env, req, "bands", {napi_int32_array}, "bands must be an Int32Array of y0, y1 pairs", &b->rows, 0, 2);
}

bool read_threshold(napi_env env, napi_value req, std::vector<double> *t)
{
    return read_array(env, req, "threshold", {napi_float64_array}, "threshold must be a Float64Array of n powers", t);
}

// ---- reply buffers ---------------------------------------------------------------------------------------------------------------------
// One block of the reply pool on its way into a reply: taken on the worker thread; handed to JavaScript by Reply::block, or given back
// here if the job ended without a reply.
struct PoolBlock {
    uint8_t *p = nullptr;
    size_t size = 0;
    int pin = kUnpinned;
    PoolBlock() = default;
    PoolBlock(const PoolBlock &) = delete;
    bool take(size_t bytes)
    {
        size = bytes;
        p = (uint8_t *)g_pool.take(size, &pin);
        return p != nullptr;
    }
    ~PoolBlock() { if (p) g_pool.give(p, size, pin); }
};

// What the library writes of an image reply: the image in a pool block, the gauges malloc'd (external ArrayBuffers later), histograms
// and dBfs range.
struct ImageBuffers {
    PoolBlock image;
    uint8_t *gmin = nullptr, *gmax = nullptr, *gamp = nullptr;
    std::vector<uint64_t> c_hist, cb_hist;
    double minmax[2] = {0.0, -200.0};
    ImageBuffers() = default;
    ImageBuffers(const ImageBuffers &) = delete;
    // an image of W x n pixels of `pixel_bytes` each; `r` gets everything but the image.  false: out of host memory
    bool take(size_t pixel_bytes, size_t W, size_t n, size_t lut_len, sp_reply *r)
    {
        image.take(pixel_bytes * W * n + 1);
        gmin = (uint8_t *)calloc(W + 1, 1);
        gmax = (uint8_t *)calloc(W + 1, 1);
        gamp = (uint8_t *)calloc(W + 1, 1);
        c_hist.assign(lut_len, 0);
        cb_hist.assign(SP_CB_HIST_SIZE, 0);
        r->gauge_mins = gmin; r->gauge_maxs = gmax; r->gauge_amps = gamp;
        r->c_hist = c_hist.data(); r->cb_hist = cb_hist.data(); r->dbfs_minmax = minmax;
        return image.p && gmin && gmax && gamp;
    }
    ~ImageBuffers() { free(gmin); free(gmax); free(gamp); }
};

// ---- writers: a reply object under construction ----------------------------------------------------------------------------------------
// Properties appear in the order of the calls.  After a failed N-API call the remaining calls do nothing and done() is null; a buffer
// belongs to JavaScript only once its ArrayBuffer exists, so whatever did not get that far is still freed by the job.
struct Reply {
    napi_env env;
    napi_value obj = nullptr;
    bool ok;
    explicit Reply(napi_env e) : env(e) { ok = napi_create_object(env, &obj) == napi_ok; }
    napi_value done() const { return ok ? obj : nullptr; }

    void set(const char *name, napi_value v) { ok = ok && napi_set_named_property(env, obj, name, v) == napi_ok; }
    static size_t element_size(napi_typedarray_type type) { return type == napi_float64_array ? 8 : type == napi_uint8_array ? 1 : 4; }
    // `count` elements of `ab` from byte `offset` on, as the typed array `name`
    void view(const char *name, napi_typedarray_type type, napi_value ab, size_t offset, size_t count)
    {
        napi_value ta;
        ok = ok && napi_create_typedarray(env, type, count, ab, offset, &ta) == napi_ok;
        set(name, ta);
    }
    // a new ArrayBuffer of `bytes` bytes; `data`: where they are
    napi_value buffer(size_t bytes, void **data)
    {
        napi_value ab = nullptr;
        ok = ok && napi_create_arraybuffer(env, bytes, data, &ab) == napi_ok;
        return ab;
    }
    napi_value copy_of(const void *from, size_t bytes)
    {
        void *data = nullptr;
        napi_value ab = buffer(bytes, &data);
        if (ok && bytes) memcpy(data, from, bytes);
        return ab;
    }
    // these `count` elements, copied into a new typed array `name`
    void array(const char *name, napi_typedarray_type type, const void *from, size_t count)
    {
        view(name, type, copy_of(from, count * element_size(type)), 0, count);
    }
    void ints(std::initializer_list<std::pair<const char *, int32_t>> props)
    {
        for (const auto &p : props) {
            napi_value v = nullptr;
            ok = ok && napi_create_int32(env, p.second, &v) == napi_ok;
            set(p.first, v);
        }
    }
    // ... and doubles, in an object of their own under `under` if that is given
    void doubles(const char *under, std::initializer_list<std::pair<const char *, double>> props)
    {
        Reply to = under ? Reply(env) : *this;
        to.ok = to.ok && ok;
        for (const auto &p : props) {
            napi_value v = nullptr;
            to.ok = to.ok && napi_create_double(env, p.second, &v) == napi_ok;
            to.set(p.first, v);
        }
        ok = to.ok;
        if (under) set(under, to.obj);
    }
    void string(const char *name, const std::string &s)
    {
        napi_value v = nullptr;
        ok = ok && napi_create_string_utf8(env, s.c_str(), NAPI_AUTO_LENGTH, &v) == napi_ok;
        set(name, v);
    }
    // a histogram's counts as a Float64Array
    void hist(const char *name, const std::vector<uint64_t> &h)
    {
        void *data = nullptr;
        napi_value ab = buffer(h.size() * 8, &data);
        for (size_t i = 0; ok && i < h.size(); i++) ((double *)data)[i] = (double)h[i];
        view(name, napi_float64_array, ab, 0, h.size());
    }
    // `len` malloc'd bytes as an external ArrayBuffer that frees them
    void external(const char *name, uint8_t *&p, size_t len)
    {
        napi_value ab = nullptr;
        ok = ok && napi_create_external_arraybuffer(env, p, len, free_cb, nullptr, &ab) == napi_ok;
        if (ok) p = nullptr;   // owned by the ArrayBuffer now
        set(name, ab);
    }
    void gauges(ImageBuffers &b, size_t W)
    {
        external("gauge_mins", b.gmin, W);
        external("gauge_maxs", b.gmax, W);
        external("gauge_amps", b.gamp, W);
    }
    // The pool block's first `bytes` bytes as an external ArrayBuffer under `name` - or, with `view_as`, the typed array of `count`
    // elements over it.  V8 is told the block's weight; the ArrayBuffer's finalizer takes the weight back and returns the block.
    void block(const char *name, PoolBlock &b, size_t bytes, const napi_typedarray_type *view_as = nullptr, size_t count = 0)
    {
        if (!ok) return;
        napi_value ab;
        PoolTag *tag = new PoolTag{b.size, b.pin};
        if (napi_create_external_arraybuffer(env, b.p, bytes, pool_free_cb, tag, &ab) != napi_ok) {
            delete tag;
            ok = false;
            return;
        }
        int64_t total = 0;
        napi_adjust_external_memory(env, reply_weight(b.size), &total);
        b.p = nullptr;   // owned by the ArrayBuffer now
        if (view_as) view(name, *view_as, ab, 0, count);
        else set(name, ab);
    }
};
const napi_typedarray_type kAsU8 = napi_uint8_array, kAsF64 = napi_float64_array;

// render's reply, and renderIndex's: the W x n image under `name` (as `bytes` bytes, or the Uint8Array of them), the gauges, the
// histograms, `stages` (take_us, native_us) if given, and the dBfs range
Reply image_reply(napi_env env, ImageBuffers &b, const char *name, bool as_u8, size_t bytes, size_t W, const double *stages)
{
    Reply r(env);
    r.block(name, b.image, bytes, as_u8 ? &kAsU8 : nullptr, bytes);
    r.gauges(b, W);
    r.hist("c_hist", b.c_hist);
    r.hist("cB_hist", b.cb_hist);
    if (stages) r.doubles("stages", {{"take_us", stages[0]}, {"native_us", stages[1]}});
    r.doubles(nullptr, {{"dBfs_min", b.minmax[0]}, {"dBfs_max", b.minmax[1]}});
    return r;
}

inline size_t at_least_0(int32_t v) { return v > 0 ? (size_t)v : 0; }

// ---- render, renderNamed, groupRender: (handle, req, cb) / ...Sync(handle, req) ------------------------------------------------------------
// req: {format: int, buffer, n, windowc, block_norm, gain, range, lut, width, channelMode, waterfall, detector} - or, named, {format,
// window, cmap: strings, buffer, n, gain, range, width, channelMode, waterfall, detector} - plus `gather` on a group handle.  The
// numbers are read unchecked: one that is no number keeps the value read before it, and the library refuses what it cannot render.
struct RenderJob : JobBase {
    Settings set;
    Capture cap;
    // a request by option names (renderNamed): the library evaluates taper and colour map itself
    bool named = false;
    std::string nformat, nwindow, ncmap;
    sp_group *group = nullptr;                  // a group handle's job
    int32_t gather = SP_GROUP_GATHER_DEVICE;    // ... and where its strips meet (req.gather: 'device' | 'host')
    std::string transport, note;
    double t_render = 0, t_gather = 0, t_download = 0;
    // where the job's time went on the worker thread (microseconds): reply buffers from the pool, everything else
    double stages[2] = {0, 0};
    ImageBuffers out;
    void run() override;
    void call(sp_reply *r);
    napi_value result(napi_env env) override;
};

bool parse_request(napi_env env, napi_value handle, napi_value req, RenderJob *j, bool named)
{
    if (!(j->owner = read_handle(env, handle, nullptr))) return false;
    j->group = j->owner->g;
    sp_request &q = j->set.req;
    napi_value v;
    int32_t i32 = 0;
    j->named = named;
    if (named) {
        j->nformat = get_string(env, req, "format");
        j->nwindow = get_string(env, req, "window");
        j->ncmap = get_string(env, req, "cmap");
    } else {
        get_named(env, req, "format", &v); napi_get_value_int32(env, v, &i32); q.format = i32;
    }
    get_named(env, req, "n", &v); napi_get_value_int32(env, v, &i32); q.n = i32;
    get_named(env, req, "width", &v); napi_get_value_int32(env, v, &i32); j->cap.width = i32;
    if (j->group && get_string(env, req, "gather") == "host") j->gather = SP_GROUP_GATHER_HOST;
    q.channel_mode = get_bool(env, req, "channelMode");
    q.waterfall = get_bool(env, req, "waterfall");
    if (!read_detector(env, req, &q.detector)) return false;
    q.block_norm = get_double(env, req, "block_norm");
    q.gain = get_double(env, req, "gain");
    q.range = get_double(env, req, "range");
    if (!read_buffer(env, req, &j->cap)) return false;
    if (named) {
        int32_t lut_len = 0;
        sp_named_resolve(j->nwindow.c_str(), j->ncmap.c_str(), nullptr, nullptr, &lut_len);   // sizes the reply's c_hist
        q.lut_len = lut_len;
        return true;
    }
    if (!read_windowc(env, req, &j->set) || !read_lut(env, req, &j->set, 0, "lut must be a Uint8Array") || !window_covers_n(env, j->set)) return false;
    j->set.bind();
    return true;
}

void RenderJob::run()
{
    const double t0 = now_us();
    sp_reply r{};
    const bool taken = out.take(4, at_least_0(cap.width), at_least_0(set.req.n), at_least_0(set.req.lut_len), &r);
    r.rgba = out.image.p;
    stages[0] = now_us() - t0;
    if (taken) call(&r);
    else no_memory();
    stages[1] = now_us() - t0 - stages[0];
}

void RenderJob::call(sp_reply *r)
{
    const sp_request &q = set.req;
    if (group) {
        status = sp_group_render_ex(group, &q, cap.bytes, cap.nbytes, cap.width, r, gather);
        if (status != SP_OK) error = sp_group_last_error(group);
        // (read here, on the worker thread that owns the group for the duration of the job)
        transport = sp_group_transport(group);
        note = sp_group_transport_note(group);
        sp_group_last_timings(group, &t_render, &t_gather, &t_download);
        return;
    }
    if (!named) return finish(sp_render(owner->c, &q, cap.bytes, cap.nbytes, cap.width, r));
    sp_named_request nr{};
    nr.format = nformat.c_str();
    nr.window = nwindow.c_str();
    nr.cmap = ncmap.c_str();
    nr.n = q.n;
    nr.channel_mode = q.channel_mode;
    nr.waterfall = q.waterfall;
    nr.gain = q.gain;
    nr.range = q.range;
    finish(sp_render_named_ex(owner->c, &nr, q.detector, cap.bytes, cap.nbytes, cap.width, r));
}

napi_value RenderJob::result(napi_env env)
{
    const size_t W = at_least_0(cap.width);
    Reply r = image_reply(env, out, "rgba", false, 4 * W * (size_t)set.req.n, W, stages);
    if (group) {
        const int members = sp_group_size(group);
        r.ints({{"members", members}, {"sliceWidth", members > 0 ? cap.width / members : 0}});
        r.string("transport", transport);
        r.string("transportNote", note);
        r.doubles("timings", {{"render_ms", t_render}, {"gather_ms", t_gather}, {"download_ms", t_download}});
    }
    return r.done();
}

template <bool Named, bool Async>
napi_value Render(napi_env env, napi_callback_info info)
{
    size_t argc = 3;
    napi_value argv[3];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    RenderJob *j = new RenderJob;
    if (!parse_request(env, argv[0], argv[1], j, Named)) { free_job(env, j); return nullptr; }
    if (!Async) return run_sync(env, j);
    napi_value buf = nullptr;   // (left null, it fails the queueing)
    napi_get_named_property(env, argv[1], "buffer", &buf);
    return queue_async(env, j, {argv[2], argv[0], buf}, "spectroplot_hip.render", "could not queue the render");
}

// ---- batches: renderBatch(handle, req, [{buffer, width}], cb) / renderBatchSync(handle, req, items) -------------------------------
// req is render's request without buffer and width; every item gets its own reply, shaped as render's (sp_render_batch).  Every
// value is read with its status checked: a missing or non-numeric field throws instead of leaving a stale value behind.
struct BatchJob : JobBase {
    Settings set;
    struct Item {
        Capture cap;
        ImageBuffers out;
    };
    std::deque<Item> items;
    void run() override;
    napi_value result(napi_env env) override;
};

bool parse_batch(napi_env env, napi_value handle, napi_value req, napi_value items, BatchJob *b)
{
    if (!(b->owner = read_handle(env, handle, "renderBatch"))) return false;
    sp_request &q = b->set.req;
    if (!checked_int32(env, req, "format", &q.format) || !checked_int32(env, req, "n", &q.n)) return false;
    if (!checked_bool(env, req, "channelMode", &q.channel_mode) || !checked_bool(env, req, "waterfall", &q.waterfall)) return false;
    if (!read_detector(env, req, &q.detector)) return false;   // (a peak batch is refused by the library: SP_ERR_UNSUPPORTED)
    if (!checked_number(env, req, "block_norm", &q.block_norm) || !checked_number(env, req, "gain", &q.gain)) return false;
    if (!checked_number(env, req, "range", &q.range)) return false;
    if (!read_windowc(env, req, &b->set) || !window_covers_n(env, b->set) || !read_lut(env, req, &b->set, 0, "lut must be a Uint8Array")) return false;
    b->set.bind();
    bool is_array = false;
    uint32_t count = 0;
    if (napi_is_array(env, items, &is_array) != napi_ok || !is_array || napi_get_array_length(env, items, &count) != napi_ok) {
        napi_throw_type_error(env, nullptr, "items must be an array of {buffer, width}");
        return false;
    }
    for (uint32_t k = 0; k < count; k++) {
        napi_value it;
        napi_valuetype t;
        if (napi_get_element(env, items, k, &it) != napi_ok || napi_typeof(env, it, &t) != napi_ok || t != napi_object) {
            napi_throw_type_error(env, nullptr, "items must be an array of {buffer, width}");
            return false;
        }
        b->items.emplace_back();
        Capture &c = b->items.back().cap;
        if (!checked_int32(env, it, "width", &c.width)) return false;
        if (c.width < 0) {
            napi_throw_range_error(env, nullptr, "width must not be negative");
            return false;
        }
        if (!read_buffer(env, it, &c)) return false;
    }
    return true;
}

void BatchJob::run()
{
    std::vector<sp_batch_item> its(items.size());
    for (size_t k = 0; k < items.size(); k++) {
        Item &j = items[k];
        sp_batch_item &it = its[k];
        if (!j.out.take(4, (size_t)j.cap.width, (size_t)set.req.n, at_least_0(set.req.lut_len), &it.reply)) return no_memory();
        it.reply.rgba = j.out.image.p;
        it.bytes = j.cap.bytes;
        it.nbytes = j.cap.nbytes;
        it.width = j.cap.width;
    }
    finish(sp_render_batch(owner->c, &set.req, its.data(), (int32_t)its.size()));
}

napi_value BatchJob::result(napi_env env)
{
    napi_value arr;
    if (napi_create_array_with_length(env, items.size(), &arr) != napi_ok) return nullptr;
    const double no_stages[2] = {0, 0};   // (an item's reply has render's properties)
    for (size_t k = 0; k < items.size(); k++) {
        const size_t W = (size_t)items[k].cap.width;
        napi_value r = image_reply(env, items[k].out, "rgba", false, 4 * W * (size_t)set.req.n, W, no_stages).done();
        if (!r || napi_set_element(env, arr, (uint32_t)k, r) != napi_ok) return nullptr;
    }
    return arr;
}

template <bool Async>
napi_value RenderBatch(napi_env env, napi_callback_info info)
{
    size_t argc = 4;
    napi_value argv[4];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    napi_valuetype t = napi_undefined;
    if (argc < (Async ? 4 : 3) || (Async && (napi_typeof(env, argv[3], &t) != napi_ok || t != napi_function))) {
        napi_throw_type_error(env, nullptr, Async ? "renderBatch(handle, request, items, callback)" : "renderBatchSync(handle, request, items)");
        return nullptr;
    }
    BatchJob *b = new BatchJob;
    if (!parse_batch(env, argv[0], argv[1], argv[2], b)) { free_job(env, b); return nullptr; }
    if (!Async) return run_sync(env, b);
    // (the items array keeps their buffers alive)
    return queue_async(env, b, {argv[3], argv[0], argv[2]}, "spectroplot_hip.renderBatch", "could not queue the batch");
}

// ---- checked requests: every kind below -----------------------------------------------------------------------------------------------------
// Every value of such a request is read into a variable of its own with its status checked, as for a batch: a request that cannot be
// read throws and never renders.  The shared fields are {format, n, width, channelMode, block_norm, gain, range, windowc, buffer} and,
// if the kind carries a picture, {waterfall, detector, lut}; a kind without one gets the sample detector and a 2-entry map (the plan
// wants one).  A kind is a struct with
//   kind      its entry point's name (the usage lines, the async resource and the refusal of a group are built from it), the noun of
//             "could not queue the ... request", and whether it carries a picture
//   read()    the readers of its own request fields, behind the shared ones
//   run()     its reply arrays and its library call, on the worker thread
//   result()  the properties of its reply
// and the members these use; its entry points are Checked<Kind, false> (sync) and Checked<Kind, true> in Init's table.
struct CheckedKind {
    const char *name, *noun;
    bool picture;
};

struct CheckedRequest : JobBase {   // what parse_checked fills
    Settings set;
    Capture cap;
};

bool parse_checked(napi_env env, napi_value handle, napi_value req, CheckedRequest *t, const CheckedKind &kind)
{
    if (!(t->owner = read_handle(env, handle, kind.name))) return false;
    sp_request &q = t->set.req;
    if (!checked_int32(env, req, "format", &q.format) || !checked_int32(env, req, "n", &q.n)) return false;
    if (!checked_int32(env, req, "width", &t->cap.width)) return false;
    if (!checked_bool(env, req, "channelMode", &q.channel_mode)) return false;
    q.detector = SP_DETECTOR_SAMPLE;
    if (kind.picture && (!checked_bool(env, req, "waterfall", &q.waterfall) || !read_detector(env, req, &q.detector))) return false;
    if (!checked_number(env, req, "block_norm", &q.block_norm) || !checked_number(env, req, "gain", &q.gain)) return false;
    if (!checked_number(env, req, "range", &q.range)) return false;
    if (q.n < 1 || t->cap.width < 0) {
        napi_throw_range_error(env, nullptr, "n must be positive and width must not be negative");
        return false;
    }
    if (!read_windowc(env, req, &t->set) || !window_covers_n(env, t->set)) return false;
    t->set.lut = {0, 0, 0, 255, 255, 255};   // (a request without a picture has no colours; the plan wants a map)
    if (kind.picture && !read_lut(env, req, &t->set, 3, "lut must be a Uint8Array of r, g, b triples")) return false;
    if (!read_buffer(env, req, &t->cap)) return false;
    t->set.bind();
    return true;
}

template <typename K>
struct CheckedJob : CheckedRequest {
    K k;
    void run() override { k.run(*this); }
    napi_value result(napi_env env) override { return k.result(env, *this); }
};

template <typename K, bool Async>
napi_value Checked(napi_env env, napi_callback_info info)
{
    const std::string name = K::kind.name;
    size_t argc = 3;
    napi_value argv[3];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    napi_valuetype ty = napi_undefined;
    if (argc < (Async ? 3 : 2) || (Async && (napi_typeof(env, argv[2], &ty) != napi_ok || ty != napi_function))) {
        napi_throw_type_error(env, nullptr, (Async ? name + "(handle, request, callback)" : name + "Sync(handle, request)").c_str());
        return nullptr;
    }
    CheckedJob<K> *t = new CheckedJob<K>;
    if (!parse_checked(env, argv[0], argv[1], t, K::kind) || !t->k.read(env, argv[1])) { free_job(env, t); return nullptr; }
    if (!Async) return run_sync(env, t);
    napi_value buf = nullptr;   // (left null, it fails the queueing)
    napi_get_named_property(env, argv[1], "buffer", &buf);
    return queue_async(env, t, {argv[2], argv[0], buf}, ("spectroplot_hip." + name).c_str(),
                       ("could not queue the " + std::string(K::kind.noun) + " request").c_str());
}

// The library call of every checked kind begins with these
#define SP_CALL_HEAD(j) (j).owner->c, &(j).set.req, (j).cap.bytes, (j).cap.nbytes, (j).cap.width

// traces: the shared fields -> {trace_min, trace_max}, two Float64Array(n) in image row order over one ArrayBuffer (sp_render_traces)
struct Traces {
    static constexpr CheckedKind kind{"renderTraces", "traces", false};
    std::vector<double> out;   // trace_min, then trace_max
    bool read(napi_env, napi_value) { return true; }
    void run(CheckedRequest &j)
    {
        const size_t n = (size_t)j.set.req.n;
        out.assign(2 * n, 0.0);
        j.finish(sp_render_traces(SP_CALL_HEAD(j), out.data(), out.data() + n));
    }
    napi_value result(napi_env env, CheckedRequest &j)
    {
        const size_t n = (size_t)j.set.req.n;
        Reply r(env);
        napi_value ab = r.copy_of(out.data(), 2 * n * 8);
        r.view("trace_min", napi_float64_array, ab, 0, n);
        r.view("trace_max", napi_float64_array, ab, n * 8, n);
        return r.done();
    }
};

// indexed images: req as for render -> render's reply with `index` - a Uint8Array(width * n), one colour-index byte per pixel in the
// RGBA image's pixel order, in a page-locked block of the reply pool - in place of `rgba`, and without `stages` (sp_render_index)
struct Index {
    static constexpr CheckedKind kind{"renderIndex", "indexed", true};
    ImageBuffers out;
    bool read(napi_env, napi_value) { return true; }
    void run(CheckedRequest &j)
    {
        sp_reply r{};
        if (!out.take(1, (size_t)j.cap.width, (size_t)j.set.req.n, (size_t)j.set.req.lut_len, &r)) return j.no_memory();
        j.finish(sp_render_index(SP_CALL_HEAD(j), &r, out.image.p));
    }
    napi_value result(napi_env env, CheckedRequest &j)
    {
        const size_t W = (size_t)j.cap.width;
        return image_reply(env, out, "index", true, W * (size_t)j.set.req.n, W, nullptr).done();
    }
};

// persistence spectrum: req as for renderIndex -> {density, n, lutLen, width}: density a Uint32Array(n * lutLen), row y at y * lutLen -
// how many of the request's frames showed colour index g in image row y (sp_render_density)
struct Density {
    static constexpr CheckedKind kind{"renderDensity", "density", true};
    std::vector<uint32_t> counts;
    bool read(napi_env, napi_value) { return true; }
    void run(CheckedRequest &j)
    {
        const sp_request &q = j.set.req;
        // (a map the library refuses gets no array: its n * lut_len could be anything)
        if (q.lut_len >= 1 && q.lut_len <= 256 && !j.allocated([&] { counts.assign((size_t)q.n * (size_t)q.lut_len, 0u); })) return;
        uint32_t none = 0;
        j.finish(sp_render_density(SP_CALL_HEAD(j), or_placeholder(counts, &none)));
    }
    napi_value result(napi_env env, CheckedRequest &j)
    {
        Reply r(env);
        r.array("density", napi_uint32_array, counts.data(), counts.size());
        r.ints({{"n", j.set.req.n}, {"lutLen", j.set.req.lut_len}, {"width", j.cap.width}});
        return r.done();
    }
};

// power plane: the shared fields plus `db` (boolean) -> {power, width, n}: power a Float64Array(width * n), frame-major - |X|^2 of frame
// x at image row y in power[x * n + y], or its dB plane with db - in a page-locked block of the reply pool (sp_render_power)
struct Power {
    static constexpr CheckedKind kind{"renderPower", "power", false};
    int32_t db = 0;
    PoolBlock out;
    bool read(napi_env env, napi_value req) { return read_db(env, req, &db); }
    void run(CheckedRequest &j)
    {
        if (!out.take((size_t)j.cap.width * (size_t)j.set.req.n * sizeof(double) + 8)) return j.no_memory();
        j.finish(sp_render_power(SP_CALL_HEAD(j), db, (double *)out.p));
    }
    napi_value result(napi_env env, CheckedRequest &j)
    {
        const size_t count = (size_t)j.cap.width * (size_t)j.set.req.n;
        Reply r(env);
        r.block("power", out, count * sizeof(double), &kAsF64, count);
        r.ints({{"width", j.cap.width}, {"n", j.set.req.n}});
        return r.done();
    }
};

// exact mean-power trace: req as for renderPower -> {mean, width, n}: mean a Float64Array(n) in image row order - the correctly rounded
// sum of |X|^2 over the request's frames divided by width, or the dB of it with db (sp_render_mean)
struct Mean {
    static constexpr CheckedKind kind{"renderMean", "mean", false};
    int32_t db = 0;
    std::vector<double> out;
    bool read(napi_env env, napi_value req) { return read_db(env, req, &db); }
    void run(CheckedRequest &j)
    {
        out.assign((size_t)j.set.req.n, 0.0);
        j.finish(sp_render_mean(SP_CALL_HEAD(j), db, out.data()));
    }
    napi_value result(napi_env env, CheckedRequest &j)
    {
        Reply r(env);
        r.array("mean", napi_float64_array, out.data(), out.size());
        r.ints({{"width", j.cap.width}, {"n", j.set.req.n}});
        return r.done();
    }
};

// exact band-power series: req as for renderPower plus `bands`, an Int32Array of y0, y1 pairs (half-open ranges of image rows) ->
// {bands, count, width, n}: bands a Float64Array(count * width), band-major - per band and frame the correctly rounded sum of |X|^2 over
// the band's rows, or the dB of it with db (sp_render_bandpower).  The library refuses bad bands (status -1) before anything is rendered.
struct BandPower {
    static constexpr CheckedKind kind{"renderBandPower", "band-power", false};
    int32_t db = 0;
    Bands bands;
    std::vector<double> out;
    bool read(napi_env env, napi_value req) { return read_db(env, req, &db) && read_bands(env, req, &bands); }
    void run(CheckedRequest &j)
    {
        if (bands.taken() && !j.allocated([&] { out.assign(bands.count() * (size_t)j.cap.width, 0.0); })) return;
        double none = 0;
        j.finish(sp_render_bandpower(SP_CALL_HEAD(j), bands.rows.data(), bands.for_library(), db, or_placeholder(out, &none)));
    }
    napi_value result(napi_env env, CheckedRequest &j)
    {
        Reply r(env);
        r.array("bands", napi_float64_array, out.data(), out.size());
        r.ints({{"count", (int32_t)bands.count()}, {"width", j.cap.width}, {"n", j.set.req.n}});
        return r.done();
    }
};

// peak track: req as for renderBandPower -> {rows, peaks, count, width, n}: rows an Int32Array(count * width) and peaks a
// Float64Array(count * width), band-major - per band and frame the strongest image row that is not a NaN (the smallest among equal ones,
// -1 where there is none) and its |X|^2 (NaN where there is none), or the dB of it with db (sp_render_track).  The library refuses bad
// bands (status -1) before anything is rendered.
struct Track {
    static constexpr CheckedKind kind{"renderTrack", "track", false};
    int32_t db = 0;
    Bands bands;
    std::vector<int32_t> best;    // the strongest row per band and frame
    std::vector<double> peaks;    // ... and its power
    bool read(napi_env env, napi_value req) { return read_db(env, req, &db) && read_bands(env, req, &bands); }
    void run(CheckedRequest &j)
    {
        const size_t count = bands.count() * (size_t)j.cap.width;
        if (bands.taken() && !j.allocated([&] { peaks.assign(count, 0.0); best.assign(count, 0); })) return;
        double none = 0;
        int32_t no_row = 0;
        j.finish(sp_render_track(SP_CALL_HEAD(j), bands.rows.data(), bands.for_library(), db, or_placeholder(best, &no_row), or_placeholder(peaks, &none)));
    }
    napi_value result(napi_env env, CheckedRequest &j)
    {
        Reply r(env);
        r.array("rows", napi_int32_array, best.data(), best.size());
        r.array("peaks", napi_float64_array, peaks.data(), peaks.size());
        r.ints({{"count", (int32_t)bands.count()}, {"width", j.cap.width}, {"n", j.set.req.n}});
        return r.done();
    }
};

// occupancy counts: req as for renderBandPower (db is read and not looked at) plus `threshold`, a Float64Array(n): one power per image
// row -> {rows, frames, count, width, n}: rows a Uint32Array(n) - per image row the frames whose |X|^2 is >= the row's threshold - and
// frames a Uint32Array(count * width), band-major - per band and frame the rows of the band that reach theirs (sp_render_occupancy; a NaN
// on either side is no hit).  The library refuses bad bands, and a threshold of another length is refused here (status -1), before
// anything is rendered.
struct Occupancy {
    static constexpr CheckedKind kind{"renderOccupancy", "occupancy", false};
    Bands bands;
    std::vector<double> threshold;
    std::vector<uint32_t> row_counts, frame_counts;
    bool read(napi_env env, napi_value req)
    {
        int32_t db = 0;
        return read_db(env, req, &db) && read_bands(env, req, &bands) && read_threshold(env, req, &threshold);
    }
    void run(CheckedRequest &j)
    {
        const int32_t n = j.set.req.n, width = j.cap.width;
        if (n < 1 || threshold.size() != (size_t)n) return j.refuse(SP_ERR_INVALID_ARG, "threshold must hold n values, one per image row");
        if (!j.allocated([&] {
                row_counts.assign((size_t)n, 0);
                if (bands.taken() && width > 0) frame_counts.assign(bands.count() * (size_t)width, 0);
            }))
            return;
        uint32_t none = 0;
        j.finish(sp_render_occupancy(SP_CALL_HEAD(j), threshold.data(), bands.rows.data(), bands.for_library(), row_counts.data(),
                                     or_placeholder(frame_counts, &none)));
    }
    napi_value result(napi_env env, CheckedRequest &j)
    {
        Reply r(env);
        r.array("rows", napi_uint32_array, row_counts.data(), row_counts.size());
        r.array("frames", napi_uint32_array, frame_counts.data(), frame_counts.size());
        r.ints({{"count", (int32_t)bands.count()}, {"width", j.cap.width}, {"n", j.set.req.n}});
        return r.done();
    }
};
#undef SP_CALL_HEAD

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
    Reply r(env);
    r.ints({{"id", id}, {"sampleWidth", sw}, {"elementSize", sp_format_element_size(id)}});
    return r.done();
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
    Reply r(env);
    std::lock_guard<std::mutex> g(g_pool.m);
    r.doubles(nullptr, {{"fresh", (double)g_pool.n_fresh}, {"recycled", (double)g_pool.n_recycled},
                        {"recycledPinned", (double)g_pool.n_recycled_pinned}, {"freeBytes", (double)g_pool.free_bytes},
                        {"pinnedBytes", (double)g_pool.pinned_bytes}, {"pinRefused", (double)g_pool.n_pin_refused},
                        {"keepLimit", (double)g_pool.keep_bytes}, {"pinnedLimit", (double)g_pool.pinned_limit},
                        {"replyWeightCap", (double)g_reply_weight_cap}});
    return r.done();
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
    napi_value argv[2], sv;
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
    Reply r(env);
    r.string("window", wname);
    r.string("cmap", ckey);
    r.ints({{"lutLength", lut_len}});
    return r.done();
}

// peakSubframes(formatId, n, nbytes, width) -> {subframes, lastColumnCount}: sp_peak_subframes, every argument checked
napi_value PeakSubframes(napi_env env, napi_callback_info info)
{
    size_t argc = 4;
    napi_value argv[4];
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
    Reply r(env);
    r.ints({{"subframes", m}, {"lastColumnCount", last}});
    return r.done();
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
    const struct { const char *name; napi_callback fn; } table[] = {
        {"deviceCount", DeviceCount},
        {"parseFormat", ParseFormat},
        {"window", Window},
        {"sliceBounds", SliceBounds},
        {"createContext", CreateContext},
        {"destroyContext", DestroyContext},
        {"allocBuffer", AllocBuffer},
        {"poolStats", PoolStats},
        {"cmap", Cmap},
        {"cmapKeys", CmapKeys},
        {"render", Render<false, true>},
        {"renderSync", Render<false, false>},
        {"renderNamed", Render<true, true>},
        {"renderNamedSync", Render<true, false>},
        {"renderBatch", RenderBatch<true>},
        {"renderBatchSync", RenderBatch<false>},
        {"renderTraces", Checked<Traces, true>},
        {"renderTracesSync", Checked<Traces, false>},
        {"renderPower", Checked<Power, true>},
        {"renderPowerSync", Checked<Power, false>},
        {"renderMean", Checked<Mean, true>},
        {"renderMeanSync", Checked<Mean, false>},
        {"bandRows", BandRows},
        {"renderBandPower", Checked<BandPower, true>},
        {"renderBandPowerSync", Checked<BandPower, false>},
        {"renderTrack", Checked<Track, true>},
        {"renderTrackSync", Checked<Track, false>},
        {"renderOccupancy", Checked<Occupancy, true>},
        {"renderOccupancySync", Checked<Occupancy, false>},
        {"renderIndex", Checked<Index, true>},
        {"renderIndexSync", Checked<Index, false>},
        {"renderDensity", Checked<Density, true>},
        {"renderDensitySync", Checked<Density, false>},
        {"namedResolve", NamedResolve},
        {"peakSubframes", PeakSubframes},
        {"planCreations", PlanCreations},
        {"createGroup", CreateGroup},
        {"destroyGroup", DestroyContext},
        {"groupRender", Render<false, true>},
        {"groupRenderSync", Render<false, false>},
    };
    std::vector<napi_property_descriptor> props;
    for (const auto &e : table) props.push_back({e.name, nullptr, e.fn, nullptr, nullptr, nullptr, napi_default, nullptr});
    napi_define_properties(env, exports, props.size(), props.data());
    napi_value v;
    napi_create_int32(env, sp_version(), &v);
    napi_set_named_property(env, exports, "version", v);
    return exports;
}

}  // namespace

NAPI_MODULE(NODE_GYP_MODULE_NAME, Init)
