// sp_kernel_frames_batch.h — k_frames_batch: the frame loop of k_frames over the groups of MANY items in one launch (sp_plan_execute_batch).
//
// The items of a batch share one plan (format, n, taper, LUT, gain, range, layout); each has its own capture, width, stride and reply.
// The host deals every item's frames into groups of one size, chosen from the batch's total frame count with launch_frames' rule, so
// small captures get full 32-frame groups and a full grid; a group never spans two items.  A table of item records and a group -> item
// map travel to the device in one copy.  The loop is k_frames' (sp_kernel_frames.h) with these differences:
//   * the workgroup reads its group's item record with scalar loads at group start;
//   * when its next group belongs to another item, the current item's last group is written out, its gauges evaluated, and the
//     workgroup's share of the item's histograms and dBfs range added to the item's reply (batch_flush); the LDS cells and range restart;
//   * the next frame's samples are requested one frame ahead as in k_frames - from the next item's capture when that frame is the
//     first of a group of another item;
//   * no reply clearing and no request number: sp_plan_execute_batch queues a small clearing kernel ahead of the launch on the same
//     stream, so no workgroup waits for another (dispatch order is undefined) and the context's single-request state is not touched.
// The body is a copy of k_frames' rather than a shared template: routed through a common always-inline body, k_frames' own instruction
// stream changed (every variant at n = 1024), and k_frames is the kernel the benchmark configurations run.
// Every measured figure in the comments of the copied loop (microseconds, per cent, profiles/ files) was measured on k_frames, not on
// this kernel.  A fix to the frame loop in sp_kernel_frames.h must be made here too.
#pragma once

#include "sp_kernel_frames.h"

namespace spk2 {

// k_frames_batch is built for n <= 512 only.  There its prefetching variants keep k_frames' register budget (no scratch, no spilled
// VGPR); at n >= 1024 the item bookkeeping on top of the frame loop's peak cost them scratch and spills.  Larger plans render the items
// of a batch one by one through k_frames: a capture of n >= 1024 fills the chip with far fewer frames, which is what batching buys.
constexpr int kBatchMaxLog2N = 9;

// k_frames_batch (sp_plan_execute_batch): one record per item of a batch, which shares the plan (the fields of FrameArgs that describe
// a capture, an image and a reply are taken from here instead).  A group of frames never spans two items; an item's groups are
// [first_group, first_group + ceil(width / group_frames)) of its launch.
struct BatchItem {
    const uint8_t *bytes;
    int64_t nbytes, nelem;
    double stride;
    uint8_t *rgba, *gauge_mins, *gauge_maxs, *gauge_amps;
    unsigned long long *out_c, *out_cb;
    double *out_minmax;
    int32_t width, in_bounds, rgba_fast, first_group;
};
typedef const __attribute__((address_space(4))) BatchItem *BatchItemK;   // scalar loads: the table is read-only for the launch

// The item of group g, and an item's record behind an opaque copy of its address: the fields are fetched (s_load) where they are used
// instead of being held in SGPRs through the frame loop (two records' worth of pointers, lengths and strides live across the loop
// cost the prefetching variants scratch and spilled VGPRs).
__device__ inline int group_item_of(const int32_t *group_item, int g)
{
    return ((const __attribute__((address_space(4))) int32_t *)group_item)[g];
}
// (every index is wave-uniform: an item is a group's, and a slot's next frame leaves its group in the same round for every slot,
// because group_frames is a multiple of the frames per round - readfirstlane tells the compiler so)
__device__ inline BatchItemK item_rec(const BatchItem *items, int i)
{
    BatchItemK p = (BatchItemK)items + __builtin_amdgcn_readfirstlane(i);
    asm volatile("" : "+s"(p));
    return p;
}

// The generic loaders of k_frames_batch: the format switch of the frame loop over the current item's capture.
template <int LOG2N>
__device__ inline void load_frame_item(int format, const BatchItemK c, int64_t start, int tl, const double (&win)[16], double (&re)[16],
                                       double (&im)[16], double2 *centre)
{
    constexpr int T = (1 << LOG2N) / 16;
    FrameArgs fa{};
    fa.bytes = c->bytes;
    fa.in_bounds = c->in_bounds;
    const spfmt::View view{c->bytes, c->nbytes, c->nelem};
    switch (format) {
#define SP_CASE(F) case F: load_frame<F>(fa, view, start, tl, T, LOG2N, win, re, im, centre); break;
        SP_CASE(SP_FMT_CU4) SP_CASE(SP_FMT_CS4) SP_CASE(SP_FMT_CU8) SP_CASE(SP_FMT_CS8) SP_CASE(SP_FMT_CU12)
        SP_CASE(SP_FMT_CS12) SP_CASE(SP_FMT_CU16) SP_CASE(SP_FMT_CS16) SP_CASE(SP_FMT_CU32) SP_CASE(SP_FMT_CS32)
        SP_CASE(SP_FMT_CU64) SP_CASE(SP_FMT_CS64) SP_CASE(SP_FMT_CF32)
#undef SP_CASE
    default: load_frame<SP_FMT_CF64>(fa, view, start, tl, T, LOG2N, win, re, im, centre); break;
    }
}

// k_frames_batch: the workgroup's share of one item's histograms and dBfs range goes to the item's reply (as at the end of k_frames,
// without the request-number check: the reply was cleared by a kernel queued ahead), then the merged cells and the range restart for
// the next item.  Every thread calls it, behind the item's last side outputs (their LDS minimum / maximum land before the first barrier).
template <int kThreads>
__device__ inline void batch_flush(const FrameArgs &a, unsigned char *smem, double *s_red, const BatchItemK it, const int tid)
{
    constexpr int kPer = 3;
    unsigned int *const s_cells = (unsigned int *)(smem + kOffCells);
    unsigned int *const s_pre = (unsigned int *)(smem + kOffXch);
    unsigned int *const s_part = s_pre + kThreads * kPer + 4;
    const int lane = tid & 63;
    const LateArgs la = late_args();   // (lut_len, cells too: nothing of this is held through the frame loop)
    const uint16_t *const cell_g = la->cell_g, *const cell_l = la->cell_l;
    const int gi_c = tid < la->lut_len ? tid : 0;
    const int cg_lo = cell_g[gi_c], cg_hi = cell_g[gi_c + 1];
    int l_lo[2], l_hi[2];
#pragma unroll
    for (int u = 0; u < 2; u++) {
        const int gi = tid + u * kThreads;
        const int l_cb = gi < SP_CB_HIST_SIZE ? SP_CB_HIST_SIZE - 1 - gi : 0;
        l_lo[u] = cell_l[l_cb];
        l_hi[u] = cell_l[l_cb + 1];
    }
    unsigned int v[kPer], run = 0;
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        const int c = tid * kPer + k;
        v[k] = c < la->cells ? s_cells[c] : 0u;
        run += v[k];
    }
    const unsigned int incl = wave_scan_u32(run);
    if (lane == 63) s_part[tid >> 6] = incl;
    lds_barrier();
    for (int i = tid; i < la->cells; i += kThreads) s_cells[i] = 0;   // (read above: the next item counts from zero)
    unsigned int base = incl - run;
    {
        const uint4 p0 = *(const uint4 *)s_part, p1 = *(const uint4 *)(s_part + 4);
        const unsigned int part[8] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w};
        const int wave = tid >> 6;
#pragma unroll
        for (int w = 0; w < 7; w++) base += w < wave ? part[w] : 0u;
    }
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        s_pre[tid * kPer + k] = base;
        base += v[k];
    }
    if (tid == kThreads - 1) s_pre[kThreads * kPer] = base;
    lds_barrier();
    const int sp0 = la->cells - 2, sp1 = la->cells - 1;
    const unsigned int n0 = s_pre[sp0 + 1] - s_pre[sp0], n1 = s_pre[sp1 + 1] - s_pre[sp1];
    unsigned long long *const out_c = it->out_c, *const out_cb = it->out_cb;
    if (tid < la->lut_len && out_c) {
        const unsigned int cnt = s_pre[cg_hi] - s_pre[cg_lo] + (tid == 0 ? n0 : 0u) + (tid == la->lut_len - 1 ? n1 : 0u);
        if (cnt) atomicAdd(&out_c[tid], (unsigned long long)cnt);
    }
#pragma unroll
    for (int u = 0; u < 2; u++) {
        const int gi = tid + u * kThreads;
        if (gi < SP_CB_HIST_SIZE && out_cb) {
            const unsigned int cnt = s_pre[l_hi[u]] - s_pre[l_lo[u]] + (gi == 0 ? n0 + n1 : 0u);
            if (cnt) atomicAdd(&out_cb[gi], (unsigned long long)cnt);
        }
    }
    double *const out_mm = it->out_minmax;
    if (tid < 2) {
        typedef __attribute__((address_space(1))) double *GlobalF64;
        if (out_mm) {
            if (tid == 0) __builtin_amdgcn_global_atomic_fmin_f64((GlobalF64)&out_mm[0], s_red[0]);
            else __builtin_amdgcn_global_atomic_fmax_f64((GlobalF64)&out_mm[1], s_red[1]);
        }
        s_red[tid] = tid ? -200.0 : 0.0;                                      // worker.js:35-36
    }
    lds_barrier();   // (the prefix's reads are done before the next frame's re-distribution writes over it)
}

template <int LOG2N, bool CH, int PFB>
__global__ __launch_bounds__(kFrameThreads, 1) void k_frames_batch(const FrameArgs a, const int format, const double2 *__restrict__ stage_tw,
                                                             const int group_frames, const int groups, const BatchItem *__restrict__ bitems,
                                                             const int32_t *__restrict__ bgroup)
{
    constexpr int kThreads = kFrameThreads;   // eight waves, two per SIMD, one workgroup per CU
    constexpr int N = 1 << LOG2N;
    constexpr int T = N / 16;                       // threads per frame
    constexpr int FPB = kThreads / T;               // frames per round
    constexpr bool BLOCK_SYNC = T > 64;
    constexpr int TWMAX = frames_tw_max_stage(N);
    constexpr int NPASS = (LOG2N + 3) / 4;
    constexpr bool PERMLANE_MID = LOG2N == 13;
    constexpr bool STAGED = PFB == 0;   // the generic loaders leave no registers for a whole pass's twiddles: read stage by stage
    // 8-byte samples at n >= 2048: a frame's samples are requested when it starts, not one frame ahead (the prefetch registers of
    // the next frame were what spilled there: cf32, n = 2048: 411 -> 358 us per 32 768 frames); its partner wave covers the latency
    // The L/R split at n >= 2048 likewise (its 16 partner values on top of a frame's 32 spill ~32 registers with the prefetch kept): a
    // spill reload waits for every vector-memory operation issued before it - in-order completion - i.e. for the prefetch itself.
    // Requested at frame start, 12 spilled registers are left and configs 3 / 5 in channel mode take 12 % less time (1.39 -> 1.22 ms,
    // 3.41 -> 2.96 ms).  (The taper from L2 per frame instead of registers: no spills at all, and slower than either.)
    // (8-byte samples with the split at n = 1024: 22 spilled registers -> 0, 90.1 -> 88.0 us at config 2's shape; n = 512: 14 -> 0,
    // 81.6 -> 77.8 us per 2^24 samples; n = 256, 6 spilled registers, is 2 % faster with the prefetch and keeps it)
    constexpr bool LATE_PF = ((PFB == 8 || (CH && PFB != 0)) && LOG2N >= 11) || (CH && PFB == 8 && LOG2N >= 9);

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const Layout lay = layout(N, a.lut_len, group_frames);
    double *s_xch = (double *)(smem + kOffXch);
    double2 *s_tw = (double2 *)(smem + lay.off_tw);
    const double *edge_g = (const double *)(smem + lay.off_gedge);
    const double *edge_cb = (const double *)(smem + lay.off_cbedge);
    unsigned long long *s_mm = (unsigned long long *)(smem + lay.off_mm);
    unsigned char *s_tile = smem + lay.off_tile;
    unsigned int *const s_lut = (unsigned int *)(smem + kOffLut);
    unsigned int *const s_cells = (unsigned int *)(smem + kOffCells);
    [[maybe_unused]] unsigned int *s_done = (unsigned int *)(smem + lay.off_done);
    double *s_red = (double *)(smem + lay.off_amp);                           // the workgroup's share of dBfs_min / dBfs_max so far
    double2 *s_amp = (double2 *)(smem + lay.off_amp + 16);                    // [2][group_frames] (I, Q) of sample n/2, by group parity

    // (lds_read_u32 / lds_count address the dynamic LDS block from 0)
    if ((unsigned)(size_t)(__attribute__((address_space(3))) unsigned char *)smem != 0u) __builtin_trap();
    const int tid = threadIdx.x;
    [[maybe_unused]] const int lane = tid & 63;
    const int fs = tid / T;                         // frame slot within a round
    const int tl = tid % T;                         // thread within the frame
    double *xbuf = s_xch + fs * (N + N / 16);
    constexpr bool COUNTER_SYNC = BLOCK_SYNC && T < kThreads;   // a frame's waves are not the whole workgroup (n = 2048, 4096)
    FrameMeet<COUNTER_SYNC, BLOCK_SYNC> meet{
        (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(size_t)(const __attribute__((address_space(3))) unsigned int *)(s_done + 2 + fs)),
        0u, (unsigned)(T / 64)};
    const int tile_pitch = N + kTilePad;
    const int cmax = a.lut_len - 1;

    // groups are dealt so that workgroups sharing an XCD (blockIdx % 8) own neighbouring groups
    const int xcd = blockIdx.x & 7, lane_in_xcd = blockIdx.x >> 3, per_xcd = gridDim.x >> 3;
    const int chunk = (groups + 7) >> 3;
    const int g_end = min(groups, (xcd + 1) * chunk);
    // the item of the workgroup's current group, the item of the frame requested next
    int cur = group_item_of(bgroup, min(xcd * chunk + lane_in_xcd, groups - 1)), rq = cur;

    constexpr bool PF = PFB != 0;
    const int sidx_pf = (int)(__brev((unsigned)tl) >> (32 - (LOG2N - 4)));
    const int rounds = (group_frames + FPB - 1) / FPB;
    uint32_t raw_lo[PF ? 16 : 1], raw_hi[PFB == 8 ? 16 : 1];
    int raw_back = 0;
    auto request = [&](int xq) {
        if constexpr (PF) {
            // (the prefetching variants only run when every frame lies inside the buffer: launch_frames)
            const BatchItemK rr = item_rec(bitems, rq);
            const int xe = rr->width;
            const int xc = xq < xe ? xq : xe - 1;
            constexpr bool UNI = T >= 64;   // a frame per wave or more: its start is wave-uniform
            const int sv = frame_start_in_bounds(rr->stride, xc);
            const int64_t st = UNI ? __builtin_amdgcn_readfirstlane(sv) : sv;
            if constexpr (PFB == 3) raw_back = (st + N) * 3 + 1 > rr->nbytes ? 1 : 0;
            issue_raw<PFB, UNI>(rr->bytes, st, T, sidx_pf, raw_lo, raw_hi, raw_back);
        }
    };
    // n = 1024, 32-frame groups: the first / second waves of the SIMDs each take one half of a group's frames
    const bool HALVES = T == 64 && group_frames == 32;
    const int fs0 = HALVES ? (fs / (FPB / 2)) * (group_frames / 2) + fs % (FPB / 2) : fs;     // the slot's frame in a group's first round
    // n <= 1024 requests the first frame's samples behind the table loads, below (config 2: -1.6 us per launch); above, where the tables
    // are a quarter of the size and the taper goes to registers after them, the old order measures the same (n = 2048) or 1.3 % better
    // (n = 8192: the other order shifts the loop's register allocation)
    constexpr bool REQ_AFTER_TABLES = PF && !LATE_PF && LOG2N <= 10;
    if (PF && !LATE_PF && !REQ_AFTER_TABLES && xcd * chunk + lane_in_xcd < g_end) request((xcd * chunk + lane_in_xcd - item_rec(bitems, rq)->first_group) * group_frames + fs0);

    constexpr bool WIN_LDS = lds_win_in_lds(N);   // taper in LDS for n <= 1024, in registers for the whole launch above
    double *s_win = (double *)(smem + lay.off_win);
    constexpr int MMS = mm_slots(N);
    constexpr bool LATE_SIDE = late_side_outputs(N);
    {
        // tables -> LDS: every global load is issued before the first LDS store (one memory latency for the prologue)
        constexpr int WINK = WIN_LDS ? (N + kThreads - 1) / kThreads : 1;
        double win_r[WINK];
        if constexpr (WIN_LDS) {
#pragma unroll
            for (int k = 0; k < WINK; k++) {
                const int i = tid + k * kThreads, e = i / T, t = i % T;
                win_r[k] = i < N ? a.window[rev4(e) * T + (int)(__brev((unsigned)t) >> (32 - (LOG2N - 4)))] : 0.0;
            }
        }
        constexpr int NTW = frames_tw_entries(N);
        constexpr int TWK = (NTW + kThreads - 1) / kThreads;
        double2 tw_r[TWK > 0 ? TWK : 1];
#pragma unroll
        for (int k = 0; k < TWK; k++) {
            const int i = tid + k * kThreads;
            tw_r[k] = i < NTW ? stage_tw[i] : make_double2(0.0, 0.0);
        }
        const unsigned int lut_r = tid < a.lut_len ? a.lut_rgba[tid] : 0u;       // lut_len <= 256 < kThreads
        double cb_r[(SP_CB_HIST_SIZE + kThreads) / kThreads];
        const double ge_r = tid < a.lut_len ? a.gray_edge[tid] : 0.0;
#pragma unroll
        for (int k = 0; k < (SP_CB_HIST_SIZE + kThreads) / kThreads; k++) {
            const int i = tid + k * kThreads;
            cb_r[k] = i <= SP_CB_HIST_SIZE ? a.cb_edge[i] : 0.0;
        }
        // The first frame's samples are requested BEHIND the table loads (vector-memory operations complete in order: requested ahead of
        // them, the wait for the tables - L2 hits - was a wait for the samples from HBM), and unconditionally (a frame past the end is
        // clamped), so that the compiler can count the 16 younger loads in that wait: s_waitcnt vmcnt(16).
        if constexpr (REQ_AFTER_TABLES) request((xcd * chunk + lane_in_xcd - item_rec(bitems, rq)->first_group) * group_frames + fs0);
        // what needs no table is set up while the loads are in flight (a table load takes ~2.3 us at the start of a launch)
        for (int i = tid; i < a.cells; i += kThreads) s_cells[i] = 0;
        if (tid < 8) s_done[tid] = 0;
        if (tid < 2) s_red[tid] = tid ? -200.0 : 0.0;                             // worker.js:35-36
        for (int i = tid; i < (LATE_SIDE ? 2 : 1) * group_frames * MMS; i += kThreads) {
            s_mm[2 * i] = 0x7ff0000000000000ull;
            s_mm[2 * i + 1] = 0ull;
        }
#pragma unroll
        for (int k = 0; k < TWK; k++) {
            const int i = tid + k * kThreads;
            if (i < NTW) s_tw[i] = tw_r[k];
        }
        if (tid < a.lut_len) s_lut[tid] = lut_r;
        if (tid < a.lut_len) ((double *)(smem + lay.off_gedge))[tid] = ge_r;
#pragma unroll
        for (int k = 0; k < (SP_CB_HIST_SIZE + kThreads) / kThreads; k++) {
            const int i = tid + k * kThreads;
            if (i <= SP_CB_HIST_SIZE) ((double *)(smem + lay.off_cbedge))[i] = cb_r[k];
        }
        if constexpr (WIN_LDS) {
#pragma unroll
            for (int k = 0; k < WINK; k++) {
                const int i = tid + k * kThreads;
                if (i < N) s_win[i] = win_r[k];
            }
        }
    }

    const double *const wbase = s_win + tl;   // stored as the threads read it: entry e*T + tl = taper[rev4(e)*T + rev(tl)]
    double win_reg[WIN_LDS ? 1 : 16];
    if constexpr (!WIN_LDS) {
        const int sidx = (int)(__brev((unsigned)tl) >> (32 - (LOG2N - 4)));
#pragma unroll
        for (int e = 0; e < 16; e++) win_reg[e] = a.window[rev4(e) * T + sidx];
    }
    lds_barrier();

    uint32_t pf_word = 0;
    // epilogue constants (sp_host.cpp build_thresholds): t = a + b*log2(|X|^2), already lowered by the margin
    const float g_a = a.g2_a, g_b = a.g2_b, g_m = a.g2_m;
    const float c_a = a.c2_a, c_b = a.c2_b, c_m = a.c2_m, c_lo = a.c2_lo, c_hi = a.c2_hi;
    const float thr = fminf(a.g2_thr, a.c2_thr);
    // A VALU instruction reads ONE scalar register: with both coefficients of a scale in SGPRs the compiler copies one of them into a
    // VGPR again for every batch of bins (24 v_mov per frame).  The addends and the upper clamp bound live in VGPRs instead.
    // (n <= 1024, where registers are left: above, the loop sits at the 256-VGPR limit and three more spill)
    float g_a_v = g_a, c_a_v = c_a, c_hi_v = c_hi;
    constexpr bool COEF_VGPR = LOG2N <= 10 && !CH && !(PFB == 8 && LOG2N < 9);
    if constexpr (COEF_VGPR) asm volatile("" : "+v"(g_a_v), "+v"(c_a_v), "+v"(c_hi_v));
    // ... and, at n = 1024, both scales of a batch's two bins as packed pairs (below that size the loop measures the same with and
    // without, and the launch-bound config 1 pays 1 % for the longer set-up: profiles/r05_experiments.txt)
    constexpr bool PK_SCALES = COEF_VGPR && LOG2N == 10;
    [[maybe_unused]] f32x2 g_b2 = {g_b, g_b}, g_a2 = {g_a, g_a}, c_b2 = {c_b, c_b}, c_a2 = {c_a, c_a};
    if constexpr (PK_SCALES) asm volatile("" : "+v"(g_b2), "+v"(g_a2), "+v"(c_b2), "+v"(c_a2));
    // clamp bounds of the colour value: clipped pixels sit in the middle of the first / last step, far from the risky zone
    const float g_lo = 0.5f, g_hi = (float)cmax + 0.5f;
    const int cell_sp0 = a.cells - 2;   // -inf / NaN dB (colour 0, bin 0), +inf dB is the next one (last colour, bin 0)

    // Side outputs of a finished group of frames (worker.js:124-136), by the workgroup's first 3 * group_frames threads: gauge_mins and
    // gauge_maxs from the frame's extreme |X|^2 (d is monotone in |X|^2, so the frame's extreme d belong to them), gauge_amps from its
    // raw centre sample: one software log10 per output.  The frame's clamped extremes are also its share of the request's dBfs range
    // (worker.js:124-125): they are folded into the workgroup's; the frame's slots are reset.
    auto side_outputs = [&](const int x0, const int par) {
        if (__builtin_amdgcn_readfirstlane(tid) >= 3 * group_frames) return;   // (wave-uniform: the waves that hold none of those threads)
        const LateArgs la = late_args();
        // three scalar loads, selected per lane below (the compiler turns a select between fields into ONE indexed vector load, whose
        // wait covers every outstanding vector-memory operation of the wave: the sample prefetch, ~2 us)
        const BatchItemK ir = item_rec(bitems, cur);
        uint8_t *out_min = ir->gauge_mins, *out_max = ir->gauge_maxs, *out_amp = ir->gauge_amps;
        int x_end = ir->width;
        asm volatile("" : "+s"(out_min), "+s"(out_max), "+s"(out_amp), "+s"(x_end));
        const double gain = la->gain, range = la->range, bn_db = la->block_norm_db;
        if (tid >= 3 * group_frames) return;
        const int role = (tid >= group_frames ? 1 : 0) + (tid >= 2 * group_frames ? 1 : 0), f = tid - role * group_frames;
        double arg;
        if (role < 2) {
            unsigned long long ext = role ? 0ull : 0x7ff0000000000000ull;
#pragma unroll
            for (int k = 0; k < MMS; k++) {
                unsigned long long *slot = s_mm + 2 * (((LATE_SIDE ? par : 0) * group_frames + f) * MMS + k) + role;
                const unsigned long long v = *slot;
                ext = role ? (v > ext ? v : ext) : (v < ext ? v : ext);
                *slot = role ? 0ull : 0x7ff0000000000000ull;
            }
            arg = __longlong_as_double((long long)ext);
        } else {
            const double2 c = s_amp[par * group_frames + f];
            arg = c.x * c.x + c.y * c.y;                                                       // worker.js:130-131
        }
        const double l5 = 5 * spjs::log10(arg);
        double v;
        if (role == 2) {
            v = l5 + gain;
        } else {
            const double d = (l5 + bn_db + gain) - gain;                                       // dBfs - gain, worker.js:100
            v = role ? (d > -200.0 ? d : -200.0) : (d < 0.0 ? d : 0.0);                        // worker.js:82-83, 102-103
            if (role) lds_max_f64(&s_red[1], v);
            else lds_min_f64(&s_red[0], v);
        }
        uint8_t *const out = role == 0 ? out_min : role == 1 ? out_max : out_amp;
        if (out && x0 + f < x_end) out[x0 + f] = clamp_u8(0.5 + (range + v) * 256 / range);   // worker.js:128-136
    };
    // write-out of tile rows [f0, f0 + fcount) by the threads [t0, t0 + dthreads), slice `part` of `nparts`
    auto drain_rows = [&](const int x0, const int part, const int nparts, const int f0, const int fcount, const int t0, const int dthreads,
                          const bool nt_rows) {
        const int dt = tid - t0;
        if (dt < 0) return;
        // (the image's address, width and layout are read from the argument segment here, once per write-out, instead of sitting in
        // SGPRs through every frame)
        const LateArgs la = late_args();
        const BatchItemK ir = item_rec(bitems, cur);
        uint8_t *const img = ir->rgba;
        const int img_width = ir->width, img_waterfall = la->waterfall;
        const int img_fast = ir->rgba_fast;
        const int x_end = img_width;
        if (img) {
            if (!img_waterfall) {
                // spectrogram: image is n rows x width columns; row y holds bin (n/2 - y) mod n            worker.js:90,117
                // The tile keeps a frame as the epilogue leaves it: 16 bytes per thread, byte e = bin tl + e*T.  A write-out item is
                // one of a thread's four dwords (bins tl + (4*e4 + j)*T, j = 0..3) of 4 consecutive frames: four 16-byte stores in four
                // rows; the items of a row segment (8 frame quads) sit in lanes 4 apart, and a wave's dword reads are conflict-free
                // (tile pitch = 1 dword mod 8).
                const int quads = fcount / 4;                     // a power of two (launch_frames)
                const int lq = 31 - __builtin_clz((unsigned)quads);
                const int items = (N / 4) * quads;
                for (int it0 = dt + part * 2 * dthreads; it0 < items; it0 += nparts * 2 * dthreads) {
                    uint32_t gb[2][4];
                    int i0v[2], xav[2];
#pragma unroll
                    for (int u = 0; u < 2; u++) {
                        const int it = it0 + u * dthreads;
                        const int itc = it < items ? it : it0;
                        const int e4 = itc & 3, fq = (itc >> 2) & (quads - 1), tq = (itc >> 2) >> lq;   // tq: thread of the frame
                        i0v[u] = tq + 4 * e4 * T;
                        xav[u] = it < items ? x0 + f0 + fq * 4 : x_end;
#pragma unroll
                        for (int k = 0; k < 4; k++)
                            gb[u][k] = *(const uint32_t *)(s_tile + __umul24((unsigned)(f0 + fq * 4), (unsigned)tile_pitch) + k * tile_pitch + tq * 16 + e4 * 4);
                    }
                    uint32_t px[2][4][4];
                    const auto lut_at = [&](unsigned off4) { return lds_read_u32(kOffLut, off4); };
#pragma unroll
                    for (int u = 0; u < 2; u++)
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                            px[u][0][k] = lut_at(byte_times4<0>(gb[u][k]));
                            px[u][1][k] = lut_at(byte_times4<1>(gb[u][k]));
                            px[u][2][k] = lut_at(byte_times4<2>(gb[u][k]));
                            px[u][3][k] = lut_at(byte_times4<3>(gb[u][k]));
                        }
                    if (img_fast) {
                        // rows are 16-byte aligned, the width is a multiple of 4 and the image is below 4 GiB: 32-bit offsets from the
                        // uniform base (24-bit multiplies), no per-store checks
#pragma unroll
                        for (int u = 0; u < 2; u++) {
                            const int xa = xav[u];
                            if (xa >= x_end) continue;
                            const unsigned y0 = (unsigned)(N / 2 - i0v[u]) & (N - 1);
#pragma unroll
                            for (int j = 0; j < 4; j++) {
                                const unsigned y = (y0 - (unsigned)(j * T)) & (N - 1);
                                const unsigned off = (__umul24(y, (unsigned)img_width) + (unsigned)xa) * 4u;
                                // written once, never read by this kernel: non-temporal where a group's row segments are whole
                                // 128-byte lines, so that the image does not displace the capture's lines in L2 (measured: 2.5 % of the
                                // kernel at n = 1024); shorter segments (large n) are pieces of lines that L2 has to merge with the
                                // neighbouring groups' pieces (non-temporal there doubled the HBM traffic)
                                store16_at(img, off, px[u][j][0], px[u][j][1], px[u][j][2], px[u][j][3], nt_rows);
                            }
                        }
                        continue;
                    }
#pragma unroll
                    for (int u = 0; u < 2; u++) {
                        const int xa = xav[u];
                        if (xa >= x_end) continue;
#pragma unroll
                        for (int j = 0; j < 4; j++) {
                            const int i = i0v[u] + j * T;
                            const int y = (N / 2 - i) & (N - 1);
                            uint8_t *dst = img + ((size_t)y * (size_t)img_width + (size_t)xa) * 4;
                            if (xa + 3 < x_end && (((size_t)dst & 15) == 0)) {
                                *(uint4 *)dst = make_uint4(px[u][j][0], px[u][j][1], px[u][j][2], px[u][j][3]);
                            } else {
#pragma unroll
                                for (int k = 0; k < 4; k++)
                                    if (xa + k < x_end) ((uint32_t *)dst)[k] = px[u][j][k];
                            }
                        }
                    }
                }
            } else {
                // waterfall: image is width rows x n columns; frame x is row width-1-x, bin i is column (i + n/2 - 1) mod n
                // An item is one dword of the tile - the colour bytes of bins t + (4*e4 + j)*T, j = 0..3, of one frame - read once and
                // stored as four pixels T columns apart; consecutive lanes take consecutive t, so each of a wave's four store
                // instructions covers 64 consecutive pixels of an image row.  (Four consecutive COLUMNS per item - one 16-byte store,
                // but four byte reads from four tile columns - took 6 ... 14 % more of the kernel than the spectrogram layout.)
                const int items = fcount * (N / 4);
                for (int it = dt + part * dthreads; it < items; it += nparts * dthreads) {
                    const int tq = it % T, e4 = (it / T) & 3, f = f0 + it / (4 * T);
                    const int xa = x0 + f;
                    if (xa >= x_end) continue;
                    const uint32_t gb = *(const uint32_t *)(s_tile + f * tile_pitch + tq * 16 + e4 * 4);
                    // columns (i + n/2 - 1) mod n of bins i = tq + (4*e4 + j)*T: c0 + j*T without a wrap inside an item - except for
                    // the one item per frame whose first pixel is the row's last (bin n/2): its other three start the row
                    const int c0 = (tq + 4 * e4 * T + N / 2 - 1) & (N - 1);
                    uint32_t *const row = (uint32_t *)(img + (size_t)(img_width - 1 - xa) * N * 4);
                    uint32_t *const p = row + (c0 == N - 1 ? -1 : c0);
                    const auto lut_at = [&](unsigned off4) { return lds_read_u32(kOffLut, off4); };
                    __builtin_nontemporal_store(lut_at(byte_times4<0>(gb)), row + c0);
                    __builtin_nontemporal_store(lut_at(byte_times4<1>(gb)), p + 1 * T);
                    __builtin_nontemporal_store(lut_at(byte_times4<2>(gb)), p + 2 * T);
                    __builtin_nontemporal_store(lut_at(byte_times4<3>(gb)), p + 3 * T);
                }
            }
        }
    };
    // non-temporal stores where a group's row pieces are whole 128-byte lines (below)
    auto drain = [&](const int x0, const int part, const int nparts) { drain_rows(x0, part, nparts, 0, group_frames, 0, kThreads, group_frames >= SP_NT_MIN_GROUP); };
    int drain_x0 = -1;
    int gpar = 0;   // parity of the workgroup's current group (s_amp)
    meet.arrive();   // the first re-distribution only waits (exchange<.., SECOND = false>)
    for (int g = xcd * chunk + lane_in_xcd; g < g_end; g += per_xcd) {
        {
            // a group of another item: the current item's last group is written out and its shares go to its reply first (the
            // samples of this group's first frame are already on their way, from the new item's capture: `rq` below)
            const int gi = group_item_of(bgroup, g);
            if (gi != cur) {
                if (drain_x0 >= 0) {
                    lds_barrier();
                    drain(drain_x0, 0, 1);
                    side_outputs(drain_x0, gpar ^ 1);
                    batch_flush<kThreads>(a, smem, s_red, item_rec(bitems, cur), tid);
                    drain_x0 = -1;
                }
                cur = gi;
            }
        }
        const int x0 = (g - item_rec(bitems, cur)->first_group) * group_frames;
        for (int r = 0; r < rounds; r++) {
            // HALVES: the first waves of the SIMDs (slots 0 .. FPB/2-1) own the group's first half of the frames, the second waves the
            // other half, so that each set can write its half out by itself after the workgroup's last group
            const int fr = HALVES ? (fs / (FPB / 2)) * (group_frames / 2) + r * (FPB / 2) + fs % (FPB / 2) : r * FPB + fs;
            const int xr = x0 + fr;
            if (fr >= group_frames) continue;   // a slot without a frame in the group's last round (its next frame is already requested)
            const BatchItemK cr = item_rec(bitems, cur);
            const int x_end = cr->width;
            const bool live = xr < x_end;
            const int x = live ? xr : x_end - 1;
            const int64_t start = frame_start(cr->stride, x);

            double re[16], im[16];
            double win[16];
            double2 *const centre = tl == 0 ? &s_amp[gpar * group_frames + fr] : nullptr;   // thread 0 of the frame: where its raw centre sample goes
            bool nonfinite = true;   // wave-uniform
#pragma unroll
            for (int e = 0; e < 16; e++) win[e] = WIN_LDS ? wbase[e * T] : win_reg[WIN_LDS ? 0 : e];
            // the frame this slot processes next: the same slot one round on, or its frame in the workgroup's next group - whose item's
            // record is read here, in the group's last round
            const bool same_group = r + 1 < rounds && (HALVES || fr + FPB < group_frames);
            rq = same_group || g + per_xcd >= g_end ? cur : group_item_of(bgroup, g + per_xcd);
            const int xn = same_group ? xr + (HALVES ? FPB / 2 : FPB)
                                      : (g + per_xcd < g_end ? (g + per_xcd - item_rec(bitems, rq)->first_group) * group_frames + fs0 : -1);
            if constexpr (PF && LATE_PF) {
                rq = cur;
                request(xr);
            }
            if constexpr (PF) {
                if constexpr (PFB == 1) {
                    if (format == SP_FMT_CU4) nonfinite = decode_frame<SP_FMT_CU4, 1>(raw_lo, raw_hi, win, re, im, centre);
                    else nonfinite = decode_frame<SP_FMT_CS4, 1>(raw_lo, raw_hi, win, re, im, centre);
                } else if constexpr (PFB == 3) {
                    if (format == SP_FMT_CU12) nonfinite = decode_frame<SP_FMT_CU12, 1>(raw_lo, raw_hi, win, re, im, centre, 8 * raw_back);
                    else nonfinite = decode_frame<SP_FMT_CS12, 1>(raw_lo, raw_hi, win, re, im, centre, 8 * raw_back);
                } else if constexpr (PFB == 2) {
                    if (format == SP_FMT_CU8) nonfinite = decode_frame<SP_FMT_CU8, 1>(raw_lo, raw_hi, win, re, im, centre);
                    else nonfinite = decode_frame<SP_FMT_CS8, 1>(raw_lo, raw_hi, win, re, im, centre);
                } else if constexpr (PFB == 4) {
                    if (format == SP_FMT_CU16) nonfinite = decode_frame<SP_FMT_CU16, 1>(raw_lo, raw_hi, win, re, im, centre);
                    else nonfinite = decode_frame<SP_FMT_CS16, 1>(raw_lo, raw_hi, win, re, im, centre);
                } else {
                    if (format == SP_FMT_CU32) nonfinite = decode_frame<SP_FMT_CU32, 16>(raw_lo, raw_hi, win, re, im, centre);
                    else if (format == SP_FMT_CS32) nonfinite = decode_frame<SP_FMT_CS32, 16>(raw_lo, raw_hi, win, re, im, centre);
                    else {
                        decode_frame<SP_FMT_CF32, 16>(raw_lo, raw_hi, win, re, im, centre);
                        nonfinite = raw_f32_nonfinite<16>(raw_lo, raw_hi);
                    }
                }
                if (!LATE_PF && xn >= 0) request(xn);           // in flight during this frame's butterflies
            } else {
                asm volatile("" ::"v"(pf_word));
                const BatchItemK nr = item_rec(bitems, rq);
                if (nr->in_bounds && xn >= 0 && xn < nr->width) {
                    const int lines = (N * a.sample_width + 127) >> 7;
                    const int64_t nb = (int64_t)frame_start(nr->stride, xn) * a.sample_width;
                    for (int l = tl; l < lines; l += T) pf_word = *(const uint32_t *)(nr->bytes + ((nb + (int64_t)l * 128) & ~(int64_t)3));
                }
                load_frame_item<LOG2N>(format, cr, start, tl, win, re, im, centre);
            }

            unsigned tw_off = 0;
            asm volatile("" : "+s"(tw_off));
            const double2 *tw = stage_tw + tw_off;
            // the previous group's write-out goes in two slices around this frame's passes, so that its stores drain while the SIMDs compute
            if (drain_x0 >= 0) {
                lds_barrier();
                if constexpr (!LATE_SIDE) side_outputs(drain_x0, gpar ^ 1);
                drain(drain_x0, 0, 2);
            }
            // ---- first pass: literal twiddles ------------------------------------------------------------------------------
            if constexpr (PFB == 0) {
                fft_pass1<false>(re, im);            // frames may leave the buffer (NaN samples), 16-byte formats
            } else if constexpr (PFB == 8) {
                if (nonfinite) fft_pass1<false>(re, im);
                else fft_pass1<true>(re, im);
            } else {
                fft_pass1<true>(re, im);             // integer samples times a finite taper (sp_api.hip: plan_frames_capable)
            }
            if constexpr (NPASS >= 2) {
                constexpr int WS1 = LOG2N >= 8 ? 4 : LOG2N - 4;
                constexpr int E1 = LOG2N >= 8 ? 8 : LOG2N;
                double *const b0 = xbuf + pad_idx(win_pos(tl, 0, 0)), *const b1 = xbuf + pad_idx(win_pos(tl, 0, WS1));
                PassTw<WS1, 5, STAGED ? 4 : E1, TWMAX> tw1;
                if constexpr (!STAGED) load_pass_tw(tw1, tl, s_tw, tw);
                // The first re-distribution never leaves a wave, whatever n: under window 0 as under window [4,8) the 64 threads of a
                // wave hold exactly the positions [1024 w, 1024 w + 1023] of their frame.  So the waves of a frame (n >= 2048) only
                // wait, before its first writes, for the partners' last reads of the frame before; between its writes and reads the
                // LDS's in-order execution of a wave's operations is all that is needed, as at n <= 1024.
                meet.wait();
                exchange<0, WS1, false, false>(re, b0, b1);
                exchange<0, WS1, false, true>(im, b0, b1);
                exchange_wait(re, im);
                if constexpr (STAGED) fft_pass_staged<WS1, 5, E1, TWMAX>(re, im, tl, s_tw, tw);
                else fft_pass<WS1, 5, E1>(re, im, tw1);
                if constexpr (PERMLANE_MID) {
                    // n = 8192: the second re-distribution stays inside the wave too - the register transpose of the 1024-point
                    // layout (window [4,8) -> [6,10) of the wave's block), two stages there, and only then the one re-distribution
                    // that crosses waves, to window [9,13) for the last three stages.  Four workgroup barriers per frame instead of
                    // eight; the swaps cost the VALU, which has the time at this size.
                    PassTw<6, 9, STAGED ? 8 : 10, TWMAX> tw2;
                    if constexpr (!STAGED) load_pass_tw(tw2, tl, s_tw, tw);
                    exchange_permlane<10>(re);
                    exchange_permlane<10>(im);
                    if constexpr (STAGED) fft_pass_staged<6, 9, 10, TWMAX>(re, im, tl, s_tw, tw);
                    else fft_pass<6, 9, 10>(re, im, tw2);
                    constexpr int WS3 = LOG2N - 4;
                    double *const b2 = xbuf + pad_idx(win_pos(tl, 0, 6)), *const b3 = xbuf + pad_idx(win_pos(tl, 0, WS3));
                    PassTw<WS3, 11, STAGED ? 10 : LOG2N, TWMAX> tw3;
                    if constexpr (!STAGED) load_pass_tw(tw3, tl, s_tw, tw);
                    exchange<6, WS3, BLOCK_SYNC, false, decltype(meet) &, false>(re, b2, b3, meet);
                    exchange<6, WS3, BLOCK_SYNC, true>(im, b2, b3, meet);
                    exchange_wait(re, im);
                    if constexpr (STAGED) fft_pass_staged<WS3, 11, LOG2N, TWMAX>(re, im, tl, s_tw, tw);
                    else fft_pass<WS3, 11, LOG2N>(re, im, tw3);
                } else if constexpr (NPASS >= 3) {
                    constexpr int WS2 = LOG2N >= 12 ? 8 : LOG2N - 4;
                    constexpr int E2 = LOG2N >= 12 ? 12 : LOG2N;
                    double *const b2 = xbuf + pad_idx(win_pos(tl, 0, WS2));
                    PassTw<WS2, 9, STAGED ? 8 : E2, TWMAX> tw2;
                    if constexpr (!STAGED) load_pass_tw(tw2, tl, s_tw, tw);
                    if constexpr (LOG2N == 9 || LOG2N == 10) {
                        // two register bits against lane bits 4 / 5: v_permlane16_swap / v_permlane32_swap.  The swaps cost the VALU
                        // about what the LDS round trip costs the LDS pipe (measured: 1.2 % of the kernel in favour of the swaps)
                        exchange_permlane<LOG2N>(re);
                        exchange_permlane<LOG2N>(im);
                    } else {
                        // (writes the positions the wave itself read last: no wait before them)
                        exchange<WS1, WS2, BLOCK_SYNC, false, decltype(meet) &, false>(re, b1, b2, meet);
                        exchange<WS1, WS2, BLOCK_SYNC, true>(im, b1, b2, meet);
                        exchange_wait(re, im);
                    }
                    if constexpr (STAGED) fft_pass_staged<WS2, 9, E2, TWMAX>(re, im, tl, s_tw, tw);
                    else fft_pass<WS2, 9, E2>(re, im, tw2);
                    static_assert(NPASS <= 3, "four passes (n = 8192) take the register-transpose branch above");
                }
            }
            // now register e of thread tl holds bin i = tl + e*T

            if constexpr (CH) {   // fft_nayuki.js:103-119, partner bin n-i fetched through LDS
                // (the partner values eight at a time where registers are short, n >= 2048: two LDS waits per component instead of one,
                // and 16 registers fewer at the frame's register peak)
                constexpr int PH = LOG2N >= 11 ? 8 : 16;
                double pp[PH];
                meet.wait();   // (announced after the last re-distribution's reads)
#pragma unroll
                for (int e = 0; e < 16; e++) xbuf[pad_idx(tl + e * T)] = re[e];
                meet();
#pragma unroll
                for (int h = 0; h < 16; h += PH) {
#pragma unroll
                    for (int k = 0; k < PH; k++) pp[k] = xbuf[pad_idx((N - (tl + (h + k) * T)) & (N - 1))];
#pragma unroll
                    for (int k = 0; k < PH; k++) {
                        const int e = h + k, i = tl + e * T;
                        const double orr = re[e];
                        if (i == 0) {
                        } else if (i == N / 2) {
                            re[e] = 0.0;
                        } else if (i < N / 2) {
                            re[e] = 0.5 * (orr + pp[k]);
                        } else {
                            re[e] = 0.5 * (-pp[k] + orr);
                        }
                    }
                    if (PH < 16) asm volatile("" ::: "memory");   // the second half's reads stay behind the first half's arithmetic
                }
                meet();
#pragma unroll
                for (int e = 0; e < 16; e++) xbuf[pad_idx(tl + e * T)] = im[e];
                meet();
#pragma unroll
                for (int h = 0; h < 16; h += PH) {
#pragma unroll
                    for (int k = 0; k < PH; k++) pp[k] = xbuf[pad_idx((N - (tl + (h + k) * T)) & (N - 1))];
#pragma unroll
                    for (int k = 0; k < PH; k++) {
                        const int e = h + k, i = tl + e * T;
                        const double oi = im[e];
                        if (i == 0 || i == N / 2) {
                            im[e] = 0.0;
                        } else if (i < N / 2) {
                            im[e] = 0.5 * (oi - pp[k]);
                        } else {
                            im[e] = 0.5 * (pp[k] + oi);
                        }
                    }
                    if (PH < 16) asm volatile("" ::: "memory");
                }
                meet.arrive();   // for the next frame's first re-distribution
            }

            if (drain_x0 >= 0) {
                drain(drain_x0, 1, 2);
                lds_barrier();
                // The previous group's side outputs, here: the two waves that evaluate them (a software log10, ~1 us) next meet the
                // others at the start of the following group, where the first waves of the SIMDs arrive early anyway; in front of this
                // barrier they held everybody up.  (The frames' extremes and centre samples are kept per group parity for it.)
                if constexpr (LATE_SIDE) side_outputs(drain_x0, gpar ^ 1);
                drain_x0 = -1;
            }
            // ---- |X|^2 -> colour index, centi-bel level ---------------------------------------------------------------------
            // t = a + b*log2((float)|X|^2) in f32 is within the margin m of the real-valued position of |X|^2 on the index
            // scale (sp_host.cpp); a and the clamp bounds are lowered by m, so floor(t) is exact unless fract(t) >= 1 - 2m.
            // Lanes past that threshold (and centi-bel values at or beyond the ends of the scale, +-inf and NaN among them, whose
            // clamp bounds lie past it by construction) take the exact edge compare.
            // four independent min / max chains: a dependent f64 operation waits several issue slots
            double mn4[4] = {spjs::inf(), spjs::inf(), spjs::inf(), spjs::inf()}, mx4[4] = {0.0, 0.0, 0.0, 0.0};
            uint32_t *trow = (uint32_t *)(s_tile + fr * tile_pitch + tl * 16);
            if (live) {
                constexpr int EB = 2;   // bins per batch
                [[maybe_unused]] uint32_t tile_word = 0;          // four colour bytes per tile dword
                constexpr bool TILE_BYTES = LOG2N >= 10;         // (n <= 512: no gain measured; n = 2048: neutral; n = 8192: -0.6 %)
                [[maybe_unused]] const unsigned trow_addr = (unsigned)(size_t)(__attribute__((address_space(3))) uint32_t *)trow;
                // a batch of bins at a time: independent chains for the VALU, one branch per batch, four colour bytes per tile dword
#pragma unroll
                for (int q = 0; q < 16 / EB; q++) {
                    double abs2[EB];
                    float tg[EB], tc[EB];
                    int gi[EB], cell[EB];
                    unsigned cell4[EB];              // 4 * (colour index + level): the byte offset of the pixel's merged cell
                    float worst = 0.0f;   // largest fractional part of the batch, either scale
                    // written stage by stage: the four chains are independent, and every step of a chain waits on the one before
                    float l2[EB];
#pragma unroll
                    for (int k = 0; k < EB; k++) abs2[k] = re[EB * q + k] * re[EB * q + k] + im[EB * q + k] * im[EB * q + k];   // worker.js:92
#pragma unroll
                    for (int k = 0; k < EB; k++) l2[k] = (float)abs2[k];
#pragma unroll
                    for (int k = 0; k < EB; k++) l2[k] = __log2f(l2[k]);
#pragma unroll
                    for (int k = 0; k < EB; k++) {
                        mn4[k & 3] = min_raw(mn4[k & 3], abs2[k]);
                        mx4[k & 3] = max_raw(mx4[k & 3], abs2[k]);
                    }
                    if constexpr (PK_SCALES) {
                        // one v_pk_fma_f32 per scale for the batch's two bins (4.7 issue cycles instead of 2 x 3.5, one instruction
                        // fewer per bin); each half rounds like v_fma_f32
                        static_assert(EB == 2, "a packed fma takes the batch's two bins");
                        const f32x2 lp = {l2[0], l2[1]};
                        const f32x2 tgp = __builtin_elementwise_fma(g_b2, lp, g_a2), tcp = __builtin_elementwise_fma(c_b2, lp, c_a2);
                        tg[0] = tgp.x; tg[1] = tgp.y;
                        tc[0] = tcp.x; tc[1] = tcp.y;
                    } else {
#pragma unroll
                        for (int k = 0; k < EB; k++) {
                            tg[k] = fmaf(g_b, l2[k], g_a_v);
                            tc[k] = fmaf(c_b, l2[k], c_a_v);
                        }
                    }
#pragma unroll
                    for (int k = 0; k < EB; k++) {
                        tg[k] = __builtin_amdgcn_fmed3f(tg[k], g_lo, g_hi);
                        tc[k] = __builtin_amdgcn_fmed3f(tc[k], c_lo, c_hi_v);
                    }
#pragma unroll
                    for (int k = 0; k < EB; k++) {
                        gi[k] = floor_to_int(tg[k]);                                   // colour index
                        cell[k] = floor_to_int(tc[k]);                                 // level (= 999 - centi-bel bin)
                    }
#pragma unroll
                    for (int k = 0; k < EB; k++) {
                        // (the clamps have turned a NaN into a bound, so the fractional parts are numbers; one threshold, the
                        // smaller of the two, serves both scales)
                        worst = fmaxf(fmaxf(worst, __builtin_amdgcn_fractf(tg[k])), __builtin_amdgcn_fractf(tc[k]));   // one v_max3_f32
                    }
                    if (__builtin_expect(__ballot(!(worst < thr)) != 0ull, 0)) {
                        // Rare (one batch in eleven), and nearly always for ONE lane on ONE bin and ONE scale: each (bin, scale) is
                        // decided on its own - the nearest edge of that scale for every lane (one LDS read, one exact comparison),
                        // only the risky lanes keep the result (edges: sp_host.h Thresholds) - so a typical visit costs a quarter
                        // of deciding everything for the whole batch.
#pragma unroll
                        for (int k = 0; k < EB; k++) {
                            const bool rgk = !(__builtin_amdgcn_fractf(tg[k]) < thr), rck = !(__builtin_amdgcn_fractf(tc[k]) < thr);
                            int lev = cell[k];
                            if (__ballot(rgk) != 0ull) {
                                const int r = min(max((int)rintf(tg[k] + g_m), 1), cmax);
                                const int g = abs2[k] >= edge_g[r] ? r : r - 1;
                                gi[k] = rgk ? g : gi[k];
                            }
                            if (__ballot(rck) != 0ull) {
                                const int r = min(max((int)rintf(tc[k] + c_m), 1), SP_CB_HIST_SIZE);
                                const int l = abs2[k] >= edge_cb[r] ? r : r - 1;
                                // -inf / NaN dB: colour 0; +inf dB: last colour; all three: ToInt32 gives key 0 = bin 0      worker.js:105,111
                                // (the clamp bounds of the level scale are risky by construction, so these lanes always come here)
                                // (their cells lie behind the regular ones: the level is set so that colour index + level names them)
                                const bool dark = !(abs2[k] > 0.0), bright = abs2[k] == spjs::inf();
                                gi[k] = rck && dark ? 0 : gi[k];
                                lev = rck ? (dark ? cell_sp0 : bright ? cell_sp0 + 1 - gi[k] : l) : lev;
                            }
                            cell[k] = lev;
                        }
                    }
                    // the merged cell's byte offset, 4 * (colour index + level), as ONE instruction (left to the compiler it becomes an
                    // add on one side of the branch above and a shift on the other)
#pragma unroll
                    for (int k = 0; k < EB; k++) asm("v_add_lshl_u32 %0, %1, %2, 2" : "=v"(cell4[k]) : "v"(gi[k]), "v"(cell[k]));
#pragma unroll
                    for (int k = 0; k < EB; k++) {
                        const int e = EB * q + k;                 // compile-time after unrolling
                        if constexpr (TILE_BYTES) {
                            // one ds_write_b8 per bin (base + immediate): packing four indices into a dword first costs three
                            // v_lshl_or_b32 per dword, and every VALU instruction costs what an f64 operation costs; the LDS pipe has room
                            asm volatile("ds_write_b8 %0, %1 offset:%2" ::"v"(trow_addr), "v"(gi[k]), "n"(e) : "memory");
                        } else {
                            tile_word = (e & 3) == 0 ? (uint32_t)gi[k] : tile_word | ((uint32_t)gi[k] << (8 * (e & 3)));
                            if ((e & 3) == 3) trow[e >> 2] = tile_word;
                        }
                    }
#pragma unroll
                    for (int k = 0; k < EB; k++) {
                        lds_count(kOffCells, cell4[k]);
                    }
                }
                const double mn = min_raw(min_raw(mn4[0], mn4[1]), min_raw(mn4[2], mn4[3]));
                const double mx = max_raw(max_raw(mx4[0], mx4[1]), max_raw(mx4[2], mx4[3]));
                unsigned long long *slot = s_mm + 2 * (((LATE_SIDE ? gpar : 0) * group_frames + fr) * MMS + (tl & (MMS - 1)));
                atomicMin(slot, (unsigned long long)__double_as_longlong(mn));
                atomicMax(slot + 1, (unsigned long long)__double_as_longlong(mx));
            }
        }
        drain_x0 = x0;
        gpar ^= 1;
    }
    // the last item's last group and shares; no request number to wait for (sp_plan_execute_batch clears the replies first)
    if (drain_x0 >= 0) {
        lds_barrier();
        drain(drain_x0, 0, 1);
        side_outputs(drain_x0, gpar ^ 1);
        batch_flush<kThreads>(a, smem, s_red, item_rec(bitems, cur), tid);
    }
}

template <int L>
int launch_frames_batch_n(const FrameArgs &a, int format, const double2 *stage_tw, int grid, int lds_bytes, int gf, int groups, int prefetch,
                          const BatchItem *items, const int32_t *group_item, int device, hipStream_t stream);
#define SP_DECL(L)                                                                                                              \
    template <>                                                                                                                 \
    int launch_frames_batch_n<L>(const FrameArgs &, int, const double2 *, int, int, int, int, int, const BatchItem *, const int32_t *, int, \
                                 hipStream_t);
SP_DECL(6) SP_DECL(7) SP_DECL(8) SP_DECL(9) SP_DECL(10) SP_DECL(11) SP_DECL(12) SP_DECL(13)
#undef SP_DECL

#ifdef SP_INST_FRAMES_LOG2N
template <int L, bool C, int P>
inline int launch_batch_variant(const FrameArgs &a, int format, const double2 *stage_tw, int grid, int lds_bytes, int gf, int groups,
                                const BatchItem *items, const int32_t *group_item, int device, hipStream_t stream)
{
    static std::atomic<bool> attr_set[kMaxDevices];
    if (device < 0 || device >= kMaxDevices || !attr_set[device].load(std::memory_order_acquire)) {
        if (hipFuncSetAttribute((const void *)k_frames_batch<L, C, P>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
            return SP_ERR_HIP;
        if (device >= 0 && device < kMaxDevices) attr_set[device].store(true, std::memory_order_release);
    }
    hipLaunchKernelGGL((k_frames_batch<L, C, P>), dim3((unsigned)grid), dim3(kFrameThreads), (size_t)lds_bytes, stream, a, format, stage_tw, gf,
                       groups, items, group_item);
    return SP_OK;
}

template <>
int launch_frames_batch_n<SP_INST_FRAMES_LOG2N>(const FrameArgs &a, int format, const double2 *stage_tw, int grid, int lds_bytes, int gf,
                                                int groups, int prefetch, const BatchItem *items, const int32_t *group_item, int device,
                                                hipStream_t stream)
{
    constexpr int L = SP_INST_FRAMES_LOG2N;
    if constexpr (L > kBatchMaxLog2N) {
        return SP_ERR_UNSUPPORTED;   // (not instantiated: plan_batch renders these items one by one)
    } else {
#define SP_V(C, P) return launch_batch_variant<L, C, P>(a, format, stage_tw, grid, lds_bytes, gf, groups, items, group_item, device, stream);
#define SP_CH(C)                                                                                              \
    switch (prefetch) {                                                                                       \
    case 8: SP_V(C, 8) case 4: SP_V(C, 4) case 3: SP_V(C, 3) case 2: SP_V(C, 2) case 1: SP_V(C, 1) default: SP_V(C, 0) \
    }
    if (a.channel_mode) { SP_CH(true) } else { SP_CH(false) }
#undef SP_V
#undef SP_CH
    }
}
#endif

// The batch's group size: launch_frames' rule applied to the frames of every item the batch kernel renders (both of its launches).
inline int batch_group_frames(int n, int64_t total_frames, int cu_count)
{
    int want = 32;
    while (want > 4 && (total_frames + want - 1) / want < 2 * (int64_t)cu_count) want >>= 1;
    return group_frames_for(n, want);
}

// One launch of k_frames_batch over `groups` groups (the caller's work list: items[], group_item[] on the device).
inline int launch_frames_batch(const FrameArgs &a, int format, const double2 *stage_tw, int gf, int groups, int prefetch, const BatchItem *items,
                               const int32_t *group_item, int cu_count, int device, hipStream_t stream)
{
    if (!frames_kernel_supports(a.n) || a.lut_len > kLdsMaxLut || a.lut_len < 2 || groups < 1) return SP_ERR_UNSUPPORTED;
    if (gf & (gf - 1)) return SP_ERR_UNSUPPORTED;
    const Layout lay = layout(a.n, a.lut_len, gf);
    if (lay.total > 160 * 1024) return SP_ERR_UNSUPPORTED;
    int grid = groups < cu_count ? groups : cu_count;
    grid = (grid + 7) & ~7;
    switch (a.levels) {
#define SP_L(L) case L: return launch_frames_batch_n<L>(a, format, stage_tw, grid, lay.total, gf, groups, prefetch, items, group_item, device, stream);
        SP_L(6) SP_L(7) SP_L(8) SP_L(9) SP_L(10) SP_L(11) SP_L(12) SP_L(13)
#undef SP_L
    default: return SP_ERR_UNSUPPORTED;
    }
}

}  // namespace spk2
