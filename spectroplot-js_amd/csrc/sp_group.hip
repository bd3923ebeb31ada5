// sp_group.hip — the caller's sliced render with the merge on the device, from ONE process (include/spectroplot_hip.h, sp_group_*).
//
// The reference cuts a capture into `workers` contiguous slices (lib/samples.js:253-258), renders each on its own Worker and merges
// histograms, dBfs range and strips on the main thread (lib/spectroplot.js:1206-1244).  A group owns one context per listed device:
// slice r is uploaded to and rendered on member r, all members at once.  Where the strips meet is the caller's choice:
//   * SP_GROUP_GATHER_DEVICE: on the root member's device, without touching host memory - RCCL (grouped ncclSend / ncclRecv over xGMI)
//     when the members sit on distinct devices and librccl can be loaded, peer copies otherwise.  Peer copies and the waterfall layout's
//     receives land in the image itself; only the spectrogram layout under RCCL receives whole strips beside the image and re-tiles
//     them.  sp_merge_replies does the side outputs' merge; the merged image comes back in one copy.
//   * SP_GROUP_GATHER_HOST: in the caller's host image - every member runs the chunked host render (sp_render_strip) on its slice and
//     writes its band over its own host link; the side outputs are merged on the host.
// Built on the library's own C ABI (contexts, plans, device buffers) plus the HIP runtime for the copies; RCCL is loaded at run time
// (dlopen), so the library has no link-time dependency on it.  An RCCL failure of any kind ends in peer copies, never in a failed render.
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "../../include/spectroplot_hip.h"
#include "sp_formats.h"
#include "sp_geometry.h"
#include "sp_host.h"

namespace {

// the RCCL entry points the gather needs (signatures of rccl.h; ncclUint8 = 1)
struct Rccl {
    void *lib = nullptr;
    std::string loaded_from, why;
    int (*CommInitAll)(void **comms, int ndev, const int *devlist) = nullptr;
    int (*CommDestroy)(void *comm) = nullptr;
    int (*CommAbort)(void *comm) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    int (*Send)(const void *buf, size_t count, int dtype, int peer, void *comm, hipStream_t stream) = nullptr;
    int (*Recv)(void *buf, size_t count, int dtype, int peer, void *comm, hipStream_t stream) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
    int (*GetVersion)(int *) = nullptr;
    bool load(const char *override_name)
    {
        if (lib) return true;
        std::vector<std::string> names;
        if (override_name && *override_name) names.push_back(override_name);
        else names = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
        for (const std::string &name : names) {
            lib = dlopen(name.c_str(), RTLD_NOW | RTLD_LOCAL);
            if (lib) {
                loaded_from = name;
                break;
            }
            const char *de = dlerror();
            why = std::string("dlopen(") + name + "): " + (de ? de : "failed");
        }
        if (!lib) return false;
        CommInitAll = (decltype(CommInitAll))dlsym(lib, "ncclCommInitAll");
        CommDestroy = (decltype(CommDestroy))dlsym(lib, "ncclCommDestroy");
        CommAbort = (decltype(CommAbort))dlsym(lib, "ncclCommAbort");
        GroupStart = (decltype(GroupStart))dlsym(lib, "ncclGroupStart");
        GroupEnd = (decltype(GroupEnd))dlsym(lib, "ncclGroupEnd");
        Send = (decltype(Send))dlsym(lib, "ncclSend");
        Recv = (decltype(Recv))dlsym(lib, "ncclRecv");
        GetErrorString = (decltype(GetErrorString))dlsym(lib, "ncclGetErrorString");
        GetVersion = (decltype(GetVersion))dlsym(lib, "ncclGetVersion");
        {
            Dl_info di;   // where the loader found it
            if (CommInitAll && dladdr((void *)CommInitAll, &di) && di.dli_fname) loaded_from = di.dli_fname;
        }
        // (ncclCommAbort is part of the set: without it a half-posted exchange could not be taken back, and giving up on RCCL would
        // have to wait for kernels that may never finish)
        if (CommInitAll && CommDestroy && CommAbort && GroupStart && GroupEnd && Send && Recv) return true;
        why = loaded_from + " lacks an entry point of the gather (ncclCommInitAll / ncclCommAbort / ncclSend / ncclRecv / ncclGroupStart / ncclGroupEnd)";
        dlclose(lib);
        lib = nullptr;
        return false;
    }
    std::string describe(int code) const { return GetErrorString ? GetErrorString(code) : ("ncclResult " + std::to_string(code)); }
};
constexpr int kNcclUint8 = 1;

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    int reserve(size_t bytes)
    {
        if (bytes <= cap) return SP_OK;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        if (hipMalloc(&p, bytes + 256) != hipSuccess) return SP_ERR_NOMEM;
        cap = bytes + 256;
        return SP_OK;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

struct Member {
    int device = 0;
    bool peer_ok = true;            // the root can address this member's memory (same device, or peer access enabled both ways)
    sp_context *ctx = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t started = nullptr, rendered = nullptr, done = nullptr;
    sp_plan *plan = nullptr;
    DevBuf strip, small;
    int status = SP_OK;
    std::string error;
    // host mode: the slice's side outputs and the host clock of its render
    std::vector<uint64_t> h_hist;
    double h_minmax[2] = {0.0, -200.0};
    double host_ms = 0;
};

enum { kRcclUntried = 0, kRcclReady = 1, kRcclFailed = -1 };

}  // namespace

struct sp_group {
    std::vector<Member> m;
    std::string error, note;
    // the request the members' plans were built from
    bool have_plan = false;
    sp_request req{};
    std::vector<double> window;
    std::vector<uint8_t> lut;
    // root-side gather targets
    DevBuf staging, smalls, image, merged;
    hipEvent_t gathered = nullptr, downloaded = nullptr;
    std::vector<uint8_t> host_small;
    // transport of the last render: 0 none (one member), 1 RCCL, 2 peer copies, 3 host
    int transport = 0;
    bool distinct = false;
    bool no_rccl = false, force_rccl = false;
    std::string rccl_lib;
    Rccl rccl;
    int rccl_state = kRcclUntried;
    std::vector<void *> comms;
    double t_render = 0, t_gather = 0, t_download = 0;
};

namespace {

int gfail(sp_group *g, int code, const std::string &msg)
{
    if (g) g->error = msg;
    return code;
}

void add_note(sp_group *g, const std::string &msg)
{
    if (g->note.find(msg) != std::string::npos) return;
    if (!g->note.empty()) g->note += "; ";
    g->note += msg;
}

void drop_plans(sp_group *g)
{
    for (Member &mb : g->m) {
        if (mb.plan) sp_plan_destroy(mb.plan);
        mb.plan = nullptr;
    }
    g->have_plan = false;
}

void drain(sp_group *g)
{
    for (Member &o : g->m) {
        (void)hipSetDevice(o.device);
        if (o.stream) (void)hipStreamSynchronize(o.stream);
    }
    if (!g->m.empty()) (void)hipSetDevice(g->m[0].device);
}

// RCCL is out for this group from now on: whatever its kernels were doing is aborted, the streams are drained, and the reason is kept.
void give_up_rccl(sp_group *g, const std::string &why)
{
    for (void *c : g->comms)
        if (c) {
            (void)g->rccl.CommAbort(c);
        }
    g->comms.clear();
    g->rccl_state = kRcclFailed;
    drain(g);
    (void)hipGetLastError();
    add_note(g, "RCCL not used: " + why + " (peer copies instead)");
}

// members run side by side on their own host threads when they sit on distinct devices (each thread drives its own GPU: uploads and
// downloads over N host links at once); members that share a device take turns on this thread - their kernels still overlap on the
// device's streams.  A thread that cannot be started runs its member here.
template <typename F>
void for_each_member(sp_group *g, F &&run)
{
    const int count = (int)g->m.size();
    if (count == 1 || !g->distinct) {
        for (int r = 0; r < count; r++) run(r);
        return;
    }
    std::vector<std::thread> th;
    th.reserve((size_t)count);
    for (int r = 0; r < count; r++) {
        try {
            th.emplace_back(run, r);
        } catch (...) {
            run(r);
        }
    }
    for (std::thread &t : th) t.join();
}

double now_ms()
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

}  // namespace

extern "C" int sp_group_create(const int32_t *devices, int32_t count, sp_group **out)
{
    if (!out) return SP_ERR_INVALID_ARG;
    *out = nullptr;
    if (!devices || count < 1 || count > 64) return SP_ERR_INVALID_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return SP_ERR_NO_DEVICE;
    for (int i = 0; i < count; i++)
        if (devices[i] < 0 || devices[i] >= ndev) return SP_ERR_INVALID_ARG;
    sp_group *g = new (std::nothrow) sp_group;
    if (!g) return SP_ERR_NOMEM;
    g->m.resize((size_t)count);
    g->distinct = true;
    for (int i = 0; i < count; i++)
        for (int k = 0; k < i; k++) g->distinct = g->distinct && devices[i] != devices[k];
    {
        auto on = [](const char *name) {
            const char *v = getenv(name);
            return v && *v && strcmp(v, "0") != 0;
        };
        g->no_rccl = on("SPECTROPLOT_HIP_NO_RCCL");
        g->force_rccl = on("SPECTROPLOT_HIP_FORCE_RCCL") && !g->no_rccl;
        const char *lib = getenv("SPECTROPLOT_HIP_RCCL_LIB");
        if (lib) g->rccl_lib = lib;
    }
    int rc = SP_OK;
    for (int i = 0; i < count && rc == SP_OK; i++) {
        Member &mb = g->m[(size_t)i];
        mb.device = devices[i];
        rc = sp_context_create(devices[i], &mb.ctx);
        if (rc) break;
        if (hipSetDevice(mb.device) != hipSuccess || hipStreamCreateWithFlags(&mb.stream, hipStreamNonBlocking) != hipSuccess
            || hipEventCreate(&mb.started) != hipSuccess || hipEventCreate(&mb.rendered) != hipSuccess || hipEventCreate(&mb.done) != hipSuccess) {
            rc = SP_ERR_HIP;
            break;
        }
        rc = sp_context_set_stream(mb.ctx, mb.stream);
    }
    if (rc == SP_OK
        && (hipSetDevice(g->m[0].device) != hipSuccess || hipEventCreate(&g->gathered) != hipSuccess || hipEventCreate(&g->downloaded) != hipSuccess))
        rc = SP_ERR_HIP;
    // peers: the root and a member on another device address each other's memory (peer copies; RCCL sets up its own paths).  A pair
    // that cannot is served by hipMemcpyPeerAsync into a staging block, and the note says so.
    if (rc == SP_OK && count > 1) {
        const int root = g->m[0].device;
        for (int i = 1; i < count; i++) {
            Member &mb = g->m[(size_t)i];
            if (mb.device == root) continue;
            auto enable = [&](int from, int to) {
                int can = 0;
                hipError_t e = hipDeviceCanAccessPeer(&can, from, to);
                if (e == hipSuccess && !can) return std::string("device ") + std::to_string(from) + " cannot access device " + std::to_string(to);
                if (e == hipSuccess) e = hipSetDevice(from);
                if (e == hipSuccess) e = hipDeviceEnablePeerAccess(to, 0);
                if (e == hipErrorPeerAccessAlreadyEnabled) {
                    (void)hipGetLastError();
                    e = hipSuccess;
                }
                if (e != hipSuccess) {
                    (void)hipGetLastError();
                    return std::string("peer access ") + std::to_string(from) + " -> " + std::to_string(to) + ": " + hipGetErrorString(e);
                }
                return std::string();
            };
            const std::string a = enable(root, mb.device), b = enable(mb.device, root);
            if (!a.empty() || !b.empty()) {
                mb.peer_ok = false;
                add_note(g, (a.empty() ? b : a) + " (copies to the root go through hipMemcpyPeerAsync and a staging block)");
            }
        }
        (void)hipSetDevice(root);
        // (tests) treat every other member as one the root cannot address: its strip is staged beside the image and re-tiled
        const char *np = getenv("SPECTROPLOT_HIP_ASSUME_NO_PEER");
        if (np && *np && strcmp(np, "0") != 0) {
            for (int i = 1; i < count; i++) g->m[(size_t)i].peer_ok = false;
            add_note(g, "SPECTROPLOT_HIP_ASSUME_NO_PEER: copies to the root go through a staging block");
        }
    }
    if (rc != SP_OK) {
        sp_group_destroy(g);
        return rc;
    }
    *out = g;
    return SP_OK;
}

extern "C" void sp_group_destroy(sp_group *g)
{
    if (!g) return;
    for (Member &mb : g->m) {
        if (mb.ctx) {
            (void)hipSetDevice(mb.device);
            if (mb.stream) (void)hipStreamSynchronize(mb.stream);
        }
    }
    for (void *c : g->comms)
        if (c && g->rccl.CommDestroy) (void)g->rccl.CommDestroy(c);
    drop_plans(g);
    if (!g->m.empty()) {
        (void)hipSetDevice(g->m[0].device);
        g->staging.release();
        g->smalls.release();
        g->image.release();
        g->merged.release();
        if (g->gathered) (void)hipEventDestroy(g->gathered);
        if (g->downloaded) (void)hipEventDestroy(g->downloaded);
    }
    for (Member &mb : g->m) {
        (void)hipSetDevice(mb.device);
        mb.strip.release();
        mb.small.release();
        if (mb.ctx) {
            (void)sp_context_set_stream(mb.ctx, nullptr);
            sp_context_destroy(mb.ctx);
        }
        if (mb.started) (void)hipEventDestroy(mb.started);
        if (mb.rendered) (void)hipEventDestroy(mb.rendered);
        if (mb.done) (void)hipEventDestroy(mb.done);
        if (mb.stream) (void)hipStreamDestroy(mb.stream);
    }
    delete g;
}

extern "C" int sp_group_size(const sp_group *g) { return g ? (int)g->m.size() : 0; }

extern "C" const char *sp_group_last_error(const sp_group *g) { return g ? g->error.c_str() : ""; }

extern "C" const char *sp_group_transport(const sp_group *g)
{
    if (!g) return "";
    return g->transport == 1 ? "rccl" : g->transport == 2 ? "peer" : g->transport == 3 ? "host" : "none";
}

extern "C" const char *sp_group_transport_note(const sp_group *g) { return g ? g->note.c_str() : ""; }

extern "C" int sp_group_rccl_info(const sp_group *g, char *text, size_t capacity)
{
    if (!g || !text || !capacity) return SP_ERR_INVALID_ARG;
    std::string t;
    if (g->rccl.lib) {
        int v = 0;
        if (g->rccl.GetVersion) (void)g->rccl.GetVersion(&v);
        t = g->rccl.loaded_from + ", ncclGetVersion " + std::to_string(v) + ", " + std::to_string(g->comms.size()) + " communicator(s)";
    }
    snprintf(text, capacity, "%s", t.c_str());
    return SP_OK;
}

extern "C" int sp_group_last_timings(const sp_group *g, double *render_ms, double *gather_ms, double *download_ms)
{
    if (!g) return SP_ERR_INVALID_ARG;
    if (render_ms) *render_ms = g->t_render;
    if (gather_ms) *gather_ms = g->t_gather;
    if (download_ms) *download_ms = g->t_download;
    return SP_OK;
}

extern "C" int sp_group_root_bytes(const sp_group *g, size_t *image_bytes, size_t *staging_bytes)
{
    if (!g) return SP_ERR_INVALID_ARG;
    if (image_bytes) *image_bytes = g->image.cap;
    if (staging_bytes) *staging_bytes = g->staging.cap;
    return SP_OK;
}

namespace {

// One sliced render of a group: what the request, the reply and the group fix before a member runs, and the phases of the render.  A
// phase returns its status and leaves the text of a failure in `why`; sp_group_render_ex is the one place that drains and reports.
struct GroupRender {
    sp_group *g;
    const sp_request *req;
    const uint8_t *bytes;
    size_t nbytes;
    int32_t width;
    const sp_reply &reply;   // the caller's
    const int count;
    Member &root;
    const spgeo::SliceLayout lay;
    const sphost::ReplyRecord rec, side;   // a member's record; its histograms and range (what is merged)
    const size_t small_pitch;              // the members' records lie this far apart on the root
    const bool want_image;
    // choose_transport's: RCCL or peer copies; the first member that sends; whether strips land beside the image, and how many
    bool use_rccl = false, rccl_done = false, stage = false;
    int first_sender = 1;
    size_t staged = 0;
    std::string why;

    GroupRender(sp_group *g_, const sp_request *q, const uint8_t *b, size_t nb, int32_t w, const sp_reply &to)
        : g(g_), req(q), bytes(b), nbytes(nb), width(w), reply(to), count((int)g_->m.size()), root(g_->m[0]),
          lay(q->n, w, count, q->waterfall != 0), rec{(size_t)q->lut_len, lay.slice_width}, side{(size_t)q->lut_len, 0},
          small_pitch((rec.bytes() + 15) & ~(size_t)15), want_image(to.rgba && lay.strip_bytes())
    {
    }

    // the one convention for a failure: its status is returned, its text left in `why` (a member's HIP error: in the member's `error`)
    int fail(int code, const std::string &msg)
    {
        why = msg;
        return code;
    }
    static int hip(std::string &to, hipError_t e, const char *what)
    {
        if (e != hipSuccess) to = std::string(what) + hipGetErrorString(e);
        return e == hipSuccess ? SP_OK : SP_ERR_HIP;
    }
    int gather_hip(hipError_t e) { return hip(why, e, "group gather: "); }

    // What sp_group_render_ex refuses before it touches the group: the group's own refusals around the request as every entry point
    // checks it (sphost::validate_request).
    int check_request(int32_t gather)
    {
        if (gather != SP_GROUP_GATHER_DEVICE && gather != SP_GROUP_GATHER_HOST) return fail(SP_ERR_INVALID_ARG, "unknown gather mode");
        if (width < 0) return fail(SP_ERR_INVALID_ARG, "width < 0");
        if (nbytes && !bytes) return fail(SP_ERR_INVALID_ARG, "bytes is null");
        if (const int rc = sphost::validate_request(req, why)) return rc;
        // (a slice is its own request with its own stride, hence its own sub-frame count: not built here)
        if (req->detector != SP_DETECTOR_SAMPLE) return fail(SP_ERR_UNSUPPORTED, "the peak detector is not supported in group renders");
        // the reference constructs its typed view over the whole buffer before it slices (lib/spectroplot.js:1096-1100)
        if (nbytes % (size_t)spfmt::describe(req->format).elem) return fail(SP_ERR_BYTE_LENGTH, "byte length is not a multiple of the element size");
        return SP_OK;
    }

    // Every member's slice (lib/samples.js:253-258) through `render(member, r, slice, slice bytes)`, all members at once; a member keeps
    // its status, its error text (its context's unless `render` left one) and the host clock of its render.
    template <typename R>
    int run_members(R &&render)
    {
        for_each_member(g, [&](int r) {
            Member &mb = g->m[(size_t)r];
            mb.error.clear();
            size_t b0 = 0, b1 = 0;
            sp_slice_bounds(nbytes, spfmt::describe(req->format).width, r, count, &b0, &b1);
            const double t0 = now_ms();
            mb.status = render(mb, r, bytes + b0, b1 - b0);
            mb.host_ms = now_ms() - t0;
            if (mb.status && mb.error.empty()) mb.error = sp_last_error(mb.ctx);
        });
        for (Member &mb : g->m)
            if (mb.status) return fail(mb.status, mb.error);
        return SP_OK;
    }

    // ---- SP_GROUP_GATHER_HOST: N host links side by side, nothing gathered on a device ------------------------------------------------
    int render_to_host()
    {
        const size_t L = side.lut_len;
        const int rc = run_members([&](Member &mb, int r, const uint8_t *slice, size_t slice_bytes) {
            mb.h_hist.assign(L + SP_CB_HIST_SIZE, 0);
            sp_reply hr{};
            hr.rgba = reply.rgba ? reply.rgba + lay.band_offset((size_t)r) : nullptr;
            hr.c_hist = mb.h_hist.data();
            hr.cb_hist = mb.h_hist.data() + L;
            hr.dbfs_minmax = mb.h_minmax;
            hr.gauge_mins = reply.gauge_mins ? reply.gauge_mins + lay.gauge_offset((size_t)r) : nullptr;
            hr.gauge_maxs = reply.gauge_maxs ? reply.gauge_maxs + lay.gauge_offset((size_t)r) : nullptr;
            hr.gauge_amps = reply.gauge_amps ? reply.gauge_amps + lay.gauge_offset((size_t)r) : nullptr;
            return sp_render_strip(mb.ctx, req, slice, slice_bytes, (int32_t)lay.slice_width, &hr, width);
        });
        if (rc) return rc;
        g->transport = 3;
        g->t_render = 0;
        for (Member &mb : g->m) g->t_render = mb.host_ms > g->t_render ? mb.host_ms : g->t_render;
        g->t_gather = g->t_download = 0;

        // the caller's merge (lib/spectroplot.js:1125-1126, 1229-1238)
        double mn = 0.0, mx = -200.0;
        for (Member &mb : g->m) {
            if (mb.h_minmax[0] < mn) mn = mb.h_minmax[0];
            if (mb.h_minmax[1] > mx) mx = mb.h_minmax[1];
        }
        if (reply.dbfs_minmax) {
            reply.dbfs_minmax[0] = mn;
            reply.dbfs_minmax[1] = mx;
        }
        const auto sum = [&](uint64_t *to, size_t from, size_t bins) {
            for (size_t i = 0; to && i < bins; i++) {
                to[i] = 0;
                for (Member &mb : g->m) to[i] += mb.h_hist[from + i];
            }
        };
        sum(reply.c_hist, 0, L);
        sum(reply.cb_hist, L, SP_CB_HIST_SIZE);
        // what no slice draws stays clear, as on the caller's fresh canvas (:1208: columns workers * sliceWidth ... width - 1)
        if (lay.rest) {
            if (reply.rgba)
                for (size_t y = 0; y < lay.rest_rows(); y++) memset(reply.rgba + lay.rest_offset() + lay.rest_pitch() * y, 0, lay.rest_row_bytes());
            for (uint8_t *gp : {reply.gauge_mins, reply.gauge_maxs, reply.gauge_amps})
                if (gp) memset(gp + lay.gauge_offset((size_t)count), 0, lay.rest);
        }
        return SP_OK;
    }

    // ---- SP_GROUP_GATHER_DEVICE ------------------------------------------------------------------------------------------------------
    // plans: one per member (its tables live on its device), kept while the request's constants repeat
    int ensure_plans()
    {
        if (g->have_plan && sphost::same_request(g->req, g->window, g->lut, req)) return SP_OK;
        drop_plans(g);
        for (Member &mb : g->m) {
            const int rc = sp_plan_create(mb.ctx, req, &mb.plan);
            if (rc) {
                why = sp_last_error(mb.ctx);
                drop_plans(g);
                return rc;
            }
        }
        g->req = *req;
        g->window.assign(req->windowc, req->windowc + req->n);
        g->lut.assign(req->lut_rgb, req->lut_rgb + 3 * (size_t)req->lut_len);
        g->req.windowc = nullptr;
        g->req.lut_rgb = nullptr;
        g->have_plan = true;
        return SP_OK;
    }

    // (buffers first, on this thread: growing one frees the old block, and hipFree waits for the whole device - not something to do
    // next to another member's copy in flight; the capture's own staging buffer belongs to the member's context)
    int reserve_member_buffers()
    {
        for (Member &mb : g->m) {
            if (hipSetDevice(mb.device) != hipSuccess) return fail(SP_ERR_HIP, "hipSetDevice");
            int rc = mb.strip.reserve(lay.strip_bytes() + 16);
            if (!rc) rc = mb.small.reserve(small_pitch);
            if (rc) return fail(rc, "group member: out of device memory");
        }
        return SP_OK;
    }

    // ... and the root's gather targets, once the transport has said whether strips arrive beside the image
    int reserve_root_buffers()
    {
        (void)hipSetDevice(root.device);
        int rc = g->smalls.reserve(small_pitch * (size_t)count);
        if (!rc && staged) rc = g->staging.reserve(lay.strip_bytes() * staged + 16);
        if (!rc && reply.rgba) rc = g->image.reserve(lay.image_bytes() + 16);
        if (!rc) rc = g->merged.reserve(side.bytes() * ((size_t)count + 1));   // the records end to end, then the merged record
        return rc ? fail(rc, "group root: out of device memory") : SP_OK;
    }

    // which transport: RCCL between distinct devices (or when forced), peer copies otherwise.  RCCL is brought up once per group; a
    // failure of it leaves a note and peer copies.
    int choose_transport()
    {
        use_rccl = !g->no_rccl && g->rccl_state != kRcclFailed && (g->force_rccl || (count > 1 && g->distinct));
        if (use_rccl && g->rccl_state == kRcclUntried) {
            if (!g->rccl.load(g->rccl_lib.c_str())) {
                give_up_rccl(g, g->rccl.why);
            } else {
                std::vector<int> devs;
                for (Member &mb : g->m) devs.push_back(mb.device);
                g->comms.assign((size_t)count, nullptr);
                const int nrc = g->rccl.CommInitAll(g->comms.data(), count, devs.data());
                if (nrc != 0) {
                    for (void *&c : g->comms) c = nullptr;   // (a failed init hands out no communicators)
                    give_up_rccl(g, "ncclCommInitAll: " + g->rccl.describe(nrc));
                } else {
                    g->rccl_state = kRcclReady;
                }
            }
            use_rccl = g->rccl_state == kRcclReady;
        }
        // under RCCL the root is a sender like every other member only in a forced one-member group (which has nothing else to send);
        // otherwise its strip is already where the merge happens
        first_sender = use_rccl && g->force_rccl && count == 1 ? 0 : 1;
        // spectrogram strips are column bands: an RCCL receive is contiguous, so those strips land beside the image and are re-tiled;
        // peers that cannot address the root's memory directly need the same block
        stage = use_rccl && !lay.waterfall;
        for (int r = 1; r < count; r++) stage = stage || !g->m[(size_t)r].peer_ok;
        staged = want_image && stage ? (size_t)(count - (use_rccl ? first_sender : 1)) : 0;
        return SP_OK;
    }

    // every member: its slice to its device, rendered there.  The slice travels in chunks of frames while earlier chunks are rendered
    // (a sparse slice: only the samples its frames read)
    int render_members()
    {
        return run_members([&](Member &mb, int, const uint8_t *slice, size_t slice_bytes) {
            int rc = hip(mb.error, hipSetDevice(mb.device), "hipSetDevice: ");
            if (!rc) rc = hip(mb.error, hipEventRecord(mb.started, mb.stream), "hipEventRecord: ");
            if (rc) return rc;
            sp_reply d = rec.view(mb.small.p);
            d.rgba = reply.rgba ? (uint8_t *)mb.strip.p : nullptr;
            rc = sp_plan_execute_from_host(mb.plan, slice, slice_bytes, (int32_t)lay.slice_width, &d);
            return rc ? rc : hip(mb.error, hipEventRecord(mb.rendered, mb.stream), "hipEventRecord: ");
        });
    }

    // where on the root strip r goes in the image, where it waits beside the image, and where member r's record block lands
    char *band(int r) const { return (char *)g->image.p + lay.band_offset((size_t)r); }
    char *stage_slot(int r) const { return (char *)g->staging.p + lay.strip_bytes() * (size_t)(r - (use_rccl ? first_sender : 1)); }
    char *small_slot(int r) const { return (char *)g->smalls.p + small_pitch * (size_t)r; }

    // strip r from `src` into its band, on member `on`'s stream.  Row bands (waterfall) are one contiguous copy.  Column bands on the
    // image's own device go through the placement kernel (sp_place_strips; a pitched device-to-device copy of 1024 rows of 1 MiB runs at
    // ~120 GB/s here, the kernel at HBM rate: 8 GiB of config-4 strips 129 -> ~10 ms), `cnt` strips laid end to end in one launch;
    // from another device a pitched peer copy.
    int place(Member &on, int r, const void *src, int cnt = 1)
    {
        if (lay.waterfall) return gather_hip(hipMemcpyAsync(band(r), src, lay.strip_bytes(), hipMemcpyDeviceToDevice, on.stream));
        if (on.device != root.device)
            return gather_hip(hipMemcpy2DAsync(band(r), lay.band_pitch(), src, lay.band_row_bytes(), lay.band_row_bytes(), lay.band_rows(),
                                               hipMemcpyDeviceToDevice, on.stream));
        const int prc = sp_place_strips(on.ctx, (uint8_t *)band(r), (const uint8_t *)src, cnt, req->n, width, (int32_t)lay.slice_width, 0);
        return prc == SP_OK ? SP_OK : fail(SP_ERR_HIP, std::string("group gather: sp_place_strips: ") + sp_last_error(on.ctx));
    }

    // what no slice draws stays clear (:1208) - only that part is cleared: the members' copies into their bands are not ordered
    // behind the root's stream
    int clear_rest()
    {
        hipError_t e = hipSetDevice(root.device);
        g->transport = 0;
        if (e == hipSuccess && reply.rgba && lay.rest) {
            char *at = (char *)g->image.p + lay.rest_offset();
            if (lay.waterfall) e = hipMemsetAsync(at, 0, lay.rest_row_bytes(), root.stream);
            else e = hipMemset2DAsync(at, lay.rest_pitch(), 0, lay.rest_row_bytes(), lay.rest_rows(), root.stream);
        }
        return gather_hip(e);
    }

    // one grouped exchange: every sender ships its strip and its record block, the root posts the matching receives (the waterfall
    // layout's straight into the image's row bands).  A failure of RCCL is no failure of the render: rccl_done stays false.
    int gather_rccl()
    {
        int nrc = g->rccl.GroupStart();
        std::string where = "ncclGroupStart";
        for (int r = first_sender; r < count && nrc == 0; r++) {
            Member &mb = g->m[(size_t)r];
            if (want_image) {
                where = "ncclSend / ncclRecv of a strip";
                nrc = g->rccl.Send(mb.strip.p, lay.strip_bytes(), kNcclUint8, 0, g->comms[(size_t)r], mb.stream);
                if (!nrc) nrc = g->rccl.Recv(lay.waterfall ? band(r) : stage_slot(r), lay.strip_bytes(), kNcclUint8, r, g->comms[0], root.stream);
            }
            if (!nrc) {
                where = "ncclSend / ncclRecv of a record block";
                nrc = g->rccl.Send(mb.small.p, small_pitch, kNcclUint8, 0, g->comms[(size_t)r], mb.stream);
            }
            if (!nrc) nrc = g->rccl.Recv(small_slot(r), small_pitch, kNcclUint8, r, g->comms[0], root.stream);
        }
        const int erc = g->rccl.GroupEnd();
        if (nrc == 0 && erc != 0) {
            nrc = erc;
            where = "ncclGroupEnd";
        }
        if (nrc != 0) {
            give_up_rccl(g, where + ": " + g->rccl.describe(nrc));   // drains every stream; the renders are complete, the copies redo the gather
            return SP_OK;
        }
        rccl_done = true;
        g->transport = 1;
        // the strips that arrived beside the image go to their column bands (the root's stream: behind its receives), one launch
        if (want_image && !lay.waterfall && count > first_sender) return place(root, first_sender, stage_slot(first_sender), count - first_sender);
        return SP_OK;
    }

    // peer copies on the sender's stream (behind its render), the root's stream waits for each
    int gather_peer()
    {
        g->transport = 2;
        int rc = SP_OK;
        for (int r = 1; r < count && !rc; r++) {
            Member &mb = g->m[(size_t)r];
            const auto peer = [&](void *dst, const void *src, size_t nb) {
                return gather_hip(mb.device == root.device ? hipMemcpyAsync(dst, src, nb, hipMemcpyDeviceToDevice, mb.stream)
                                                           : hipMemcpyPeerAsync(dst, root.device, src, mb.device, nb, mb.stream));
            };
            rc = gather_hip(hipSetDevice(mb.device));
            bool restage = false;
            if (!rc && want_image) {
                if (lay.waterfall) rc = peer(band(r), mb.strip.p, lay.strip_bytes());   // a contiguous band of rows
                else if (mb.peer_ok) rc = place(mb, r, mb.strip.p);                      // a column band, written where it belongs
                else {
                    rc = peer(stage_slot(r), mb.strip.p, lay.strip_bytes());
                    restage = true;
                }
            }
            if (!rc) rc = peer(small_slot(r), mb.small.p, small_pitch);
            if (!rc) rc = gather_hip(hipEventRecord(mb.done, mb.stream));
            if (!rc) rc = gather_hip(hipSetDevice(root.device));
            if (!rc) rc = gather_hip(hipStreamWaitEvent(root.stream, mb.done, 0));
            if (!rc && restage) rc = place(root, r, stage_slot(r));
        }
        return rc ? rc : gather_hip(hipSetDevice(root.device));
    }

    // the root's own strip and record block (its stream: behind its render)
    int place_root()
    {
        const int rc = want_image ? place(root, 0, root.strip.p) : SP_OK;
        return rc ? rc : gather_hip(hipMemcpyAsync(small_slot(0), root.small.p, small_pitch, hipMemcpyDeviceToDevice, root.stream));
    }

    // the caller's merge on the root (lib/spectroplot.js:1229-1238), then image, records and merged record to the host.  Records sit
    // small_pitch apart: sp_merge_replies takes them end to end, so they are packed first (count small copies)
    int merge_and_download()
    {
        char *packed = (char *)g->merged.p;   // [count records] then [merged record]
        hipError_t e = hipSuccess;
        for (int r = 0; r < count && e == hipSuccess; r++)
            e = hipMemcpyAsync(packed + side.bytes() * (size_t)r, small_slot(r), side.bytes(), hipMemcpyDeviceToDevice, root.stream);
        const sp_reply dm = side.view(packed + side.bytes() * (size_t)count);
        if (e == hipSuccess) {
            const int rc = sp_merge_replies(root.ctx, packed, count, (int32_t)side.lut_len, dm.c_hist, dm.cb_hist, dm.dbfs_minmax);
            if (rc) return fail(rc, sp_last_error(root.ctx));
        }
        const size_t records = small_pitch * (size_t)count;
        if (e == hipSuccess) e = hipEventRecord(g->gathered, root.stream);
        if (e == hipSuccess && reply.rgba && lay.image_bytes())
            e = hipMemcpyAsync(reply.rgba, g->image.p, lay.image_bytes(), hipMemcpyDeviceToHost, root.stream);
        g->host_small.resize(records + side.bytes());
        if (e == hipSuccess) e = hipMemcpyAsync(g->host_small.data(), g->smalls.p, records, hipMemcpyDeviceToHost, root.stream);
        if (e == hipSuccess) e = hipMemcpyAsync(g->host_small.data() + records, dm.c_hist, side.bytes(), hipMemcpyDeviceToHost, root.stream);
        if (e == hipSuccess) e = hipEventRecord(g->downloaded, root.stream);
        if (e == hipSuccess) e = hipStreamSynchronize(root.stream);
        for (int r = 1; r < count; r++) {   // (the senders' streams: their part of the exchange has long finished)
            (void)hipSetDevice(g->m[(size_t)r].device);
            const hipError_t e2 = hipStreamSynchronize(g->m[(size_t)r].stream);
            if (e == hipSuccess) e = e2;
        }
        return hip(why, e, "group download: ");
    }

    // phase clocks (device events; a member's pair lives on its own device)
    void read_clocks()
    {
        g->t_render = g->t_gather = g->t_download = 0;
        float ms = 0;
        for (Member &mb : g->m) {
            (void)hipSetDevice(mb.device);
            if (hipEventElapsedTime(&ms, mb.started, mb.rendered) == hipSuccess && ms > g->t_render) g->t_render = ms;
        }
        (void)hipSetDevice(root.device);
        if (hipEventElapsedTime(&ms, root.rendered, g->gathered) == hipSuccess) g->t_gather = ms;
        // members that share the root's device render one after the other: the gather starts when the LAST of them has rendered
        // (events of one device can be compared; on distinct devices the members render side by side and the root's event stands for all)
        for (Member &mb : g->m)
            if (mb.device == root.device && hipEventElapsedTime(&ms, mb.rendered, g->gathered) == hipSuccess && ms < g->t_gather) g->t_gather = ms;
        if (hipEventElapsedTime(&ms, g->gathered, g->downloaded) == hipSuccess) g->t_download = ms;
        (void)hipGetLastError();
    }

    // the merged side outputs, and the gauges: slice r's at columns [r * sliceWidth, (r + 1) * sliceWidth), the rest clear
    void unpack()
    {
        side.unpack_side(g->host_small.data() + small_pitch * (size_t)count, reply);
        for (uint8_t *gp : {reply.gauge_mins, reply.gauge_maxs, reply.gauge_amps})
            if (gp) memset(gp, 0, lay.width);
        for (int r = 0; r < count; r++) rec.unpack_gauges(g->host_small.data() + small_pitch * (size_t)r, reply, lay.gauge_offset((size_t)r));
    }
};

}  // namespace

extern "C" int sp_group_render_ex(sp_group *g, const sp_request *req, const uint8_t *bytes, size_t nbytes, int32_t width, const sp_reply *reply,
                                  int32_t gather)
{
    if (!g || !req || !reply) return SP_ERR_INVALID_ARG;
    GroupRender gr(g, req, bytes, nbytes, width, *reply);
    int rc = gr.check_request(gather);
    if (rc) return gfail(g, rc, gr.why);
    if (gather == SP_GROUP_GATHER_HOST) {
        rc = gr.render_to_host();
        return rc ? gfail(g, rc, gr.why) : SP_OK;
    }
    rc = gr.ensure_plans();
    if (!rc) rc = gr.reserve_member_buffers();
    if (!rc) rc = gr.choose_transport();
    if (!rc) rc = gr.reserve_root_buffers();
    if (rc) return gfail(g, rc, gr.why);   // (no stream has been touched yet)

    rc = gr.render_members();
    if (!rc) rc = gr.clear_rest();
    if (!rc && gr.use_rccl) rc = gr.gather_rccl();
    if (!rc && !gr.rccl_done && gr.count > 1) rc = gr.gather_peer();
    if (!rc && !(gr.rccl_done && gr.first_sender == 0)) rc = gr.place_root();   // (unless they went through the forced exchange)
    if (!rc) rc = gr.merge_and_download();
    if (rc) {
        drain(g);
        return gfail(g, rc, gr.why);
    }
    gr.read_clocks();
    gr.unpack();
    return SP_OK;
}

extern "C" int sp_group_render(sp_group *g, const sp_request *req, const uint8_t *bytes, size_t nbytes, int32_t width, const sp_reply *reply)
{
    return sp_group_render_ex(g, req, bytes, nbytes, width, reply, SP_GROUP_GATHER_DEVICE);
}
