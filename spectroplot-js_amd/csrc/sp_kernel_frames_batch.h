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
// The stages of the loop are k_frames' own, the fragments sp_frames_*.inc.h (sp_kernel_frames.h says why they are textual and lists
// them); this file keeps what is the batch's: the item records, the group loop with its item switches, the request and the next
// frame over two items' records, batch_flush and the launchers.  The measured figures in the fragments' comments were measured on k_frames.
#pragma once

#include "sp_kernel_frames.h"

namespace spk2 {

// k_frames_batch is built for n <= 512 only (frames_batch_variant_built).  There its prefetching variants keep k_frames' register budget (no scratch, no spilled
// VGPR); at n >= 1024 the item bookkeeping on top of the frame loop's peak cost them scratch and spills.  Larger plans render the items
// of a batch one by one through k_frames: a capture of n >= 1024 fills the chip with far fewer frames, which is what batching buys.
constexpr int kBatchMaxLog2N = 9;
__host__ __device__ constexpr bool frames_batch_variant_built(int n, bool, int) { return n <= (1 << kBatchMaxLog2N); }

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
        SP_FORMATS_BUT_CF64(SP_CASE)
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
#define SP_LUT_LEN la->lut_len
#define SP_CELLS la->cells
#define SP_REPLY it
#define SP_AFTER_CELLS_READ for (int i = tid; i < la->cells; i += kThreads) s_cells[i] = 0;   // (the next item counts from zero)
#include "sp_frames_hist_ranges.inc.h"
#include "sp_frames_hist_scan.inc.h"
#include "sp_frames_hist_adds.inc.h"
#undef SP_LUT_LEN
#undef SP_CELLS
#undef SP_REPLY
#undef SP_AFTER_CELLS_READ
    double *const out_mm = it->out_minmax;
    if (tid < 2) {
        if (out_mm) {
#include "sp_frames_range_atomics.inc.h"
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
#include "sp_frames_setup.inc.h"
    // the item of the workgroup's current group, the item of the frame requested next
    int cur = group_item_of(bgroup, min(xcd * chunk + lane_in_xcd, groups - 1)), rq = cur;

#include "sp_frames_raw_regs.inc.h"
    // (sp_frames_request.inc.h with the capture, its length, stride and end taken from the record of item `rq`: its own copy, see there)
    auto request = [&](int xq) {
        if constexpr (PF) {
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
    // (the first request's place: as in sp_frames_request_body.inc.h)
    constexpr bool REQ_AFTER_TABLES = PF && !LATE_PF && LOG2N <= 10;
    if (PF && !LATE_PF && !REQ_AFTER_TABLES && xcd * chunk + lane_in_xcd < g_end) request((xcd * chunk + lane_in_xcd - item_rec(bitems, rq)->first_group) * group_frames + fs0);

#include "sp_frames_prologue_consts.inc.h"
    {
#include "sp_frames_table_loads.inc.h"
        if constexpr (REQ_AFTER_TABLES) request((xcd * chunk + lane_in_xcd - item_rec(bitems, rq)->first_group) * group_frames + fs0);
#include "sp_frames_table_stores.inc.h"
    }

#include "sp_frames_taper.inc.h"

    uint32_t pf_word = 0;
#include "sp_frames_epilogue_consts.inc.h"

    // side outputs and write-out as in k_frames, into the current item's gauges and image
#define SP_X_END x_end
    auto side_outputs = [&](const int x0, const int par) {
        if (__builtin_amdgcn_readfirstlane(tid) >= 3 * group_frames) return;
        const LateArgs la = late_args();
        const BatchItemK ir = item_rec(bitems, cur);
        uint8_t *out_min = ir->gauge_mins, *out_max = ir->gauge_maxs, *out_amp = ir->gauge_amps;
        int x_end = ir->width;
        asm volatile("" : "+s"(out_min), "+s"(out_max), "+s"(out_amp), "+s"(x_end));
#include "sp_frames_side_outputs.inc.h"
    };
    auto drain_rows = [&](const int x0, const int part, const int nparts, const int f0, const int fcount, const int t0, const int dthreads,
                          const bool nt_rows) {
        const int dt = tid - t0;
        if (dt < 0) return;
        const LateArgs la = late_args();
        const BatchItemK ir = item_rec(bitems, cur);
        uint8_t *const img = ir->rgba;
        const int img_width = ir->width, img_waterfall = la->waterfall;
        const int img_fast = ir->rgba_fast;
        const int x_end = img_width;
#include "sp_frames_drain_rows.inc.h"
    };
#undef SP_X_END
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
#define SP_SLOT_RECORD const BatchItemK cr = item_rec(bitems, cur); const int x_end = cr->width;
#define SP_X_END x_end
#include "sp_frames_slot_deal.inc.h"
#undef SP_X_END
#undef SP_SLOT_RECORD
            const int64_t start = frame_start(cr->stride, x);

            double2 *const centre = tl == 0 ? &s_amp[gpar * group_frames + fr] : nullptr;   // thread 0 of the frame: where its raw centre sample goes
#include "sp_frames_frame_regs.inc.h"
            // sp_frames_next_frame.inc.h with the next frame's item (`rq`, whose record is read here, in the group's last round) in every
            // expression and load_frame_item as the generic loader: its own copy
            const bool same_group = r + 1 < rounds && (HALVES || fr + FPB < group_frames);
            rq = same_group || g + per_xcd >= g_end ? cur : group_item_of(bgroup, g + per_xcd);
            const int xn = same_group ? xr + (HALVES ? FPB / 2 : FPB)
                                      : (g + per_xcd < g_end ? (g + per_xcd - item_rec(bitems, rq)->first_group) * group_frames + fs0 : -1);
            if constexpr (PF && LATE_PF) {
                rq = cur;
                request(xr);
            }
            if constexpr (PF) {
#include "sp_frames_decode_pf.inc.h"
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

#include "sp_frames_passes.inc.h"
#include "sp_frames_pixels.inc.h"
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

SP_DECLARE_LAUNCH_N(launch_frames_batch_n, SP_SIZES_6_13, const BatchItem *, const int32_t *)

#ifdef SP_INST_FRAMES_LOG2N
template <>
int launch_frames_batch_n<SP_INST_FRAMES_LOG2N>(SP_LAUNCH_N_PARAMS, const BatchItem *items, const int32_t *group_item)
{
    constexpr int L = SP_INST_FRAMES_LOG2N;
    SP_LAUNCH_VARIANT_IF(frames_batch_variant_built, k_frames_batch, items, group_item)   // (n >= 1024: plan_batch renders the items one by one)
}
#endif

// One launch of k_frames_batch over `groups` groups of gf frames (the caller's work list: items[], group_item[] on the device).
inline int launch_frames_batch(const FrameArgs &a, int format, const double2 *stage_tw, int gf, int groups, int prefetch, const BatchItem *items,
                               const int32_t *group_item, int cu_count, int device, hipStream_t stream)
{
    FramesLaunch fl;
    if (groups < 1 || frames_launch_rule(a.n, a.lut_len, groups, cu_count, gf, fl)) return SP_ERR_UNSUPPORTED;
    SP_LAUNCH_LEVELS(SP_SIZES_6_13, launch_frames_batch_n, items, group_item)
}

}  // namespace spk2
