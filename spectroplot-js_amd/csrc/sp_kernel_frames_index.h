// sp_kernel_frames_index.h — k_frames_index: the frame loop of k_frames with an INDEXED image, 64 <= n <= 8192.
//
// An indexed request (include/spectroplot_hip.h, sp_plan_execute_index) asks for the picture as one colour-index byte per pixel - the
// value `gray` of lib/worker.js that c_hist counts - instead of the RGBA the LUT makes of it.  The frame loop already leaves that byte per
// bin in its LDS tile (sp_frames_pixels.inc.h); this kernel is k_frames line for line - the same launch rule, deal of groups to
// workgroups, loaders and LATE_PF order, stages, request-number handshake, side outputs and finale (the split last write-out at n = 1024
// included), all from the fragments sp_frames_*.inc.h (sp_kernel_frames.h says why they are textual and lists them; the comments on the
// loop's order are there) - and differs in ONE fragment: the body of drain_rows is sp_frames_drain_rows_index.inc.h, which stores the
// tile's bytes themselves: no LUT read per pixel, a quarter of the store bytes.
// FrameArgs keeps its layout: the index image's address travels in `rgba`, its fast-path flag (index_fast in sp_api.hip: base, width,
// first frame and end of the launch multiples of 16, image below 4 GiB) in `rgba_fast`.  The LUT is still copied to LDS by the shared
// prologue and never read.
#pragma once

#include "sp_kernel_frames.h"

#ifndef SP_INDEX_NT
#define SP_INDEX_NT 0
#endif

namespace spk2 {

// The variants of k_frames_index that exist: every (n, L/R, loader) of k_frames except those that would spill more VGPRs than their
// k_frames twin (the in-order vector-memory rule of sp_kernel_frames.h; DESIGN.md section 13 has the table) - the L/R split with the
// generic loaders (prefetch 0) at n <= 256, one register over.  Their requests take render_extract.  This predicate is the one place
// that says so: the launcher below compiles by it, sp_api.hip dispatches by it.
__host__ __device__ constexpr bool frames_index_variant_built(int n, bool channel_mode, int prefetch)
{
    return n >= 64 && n <= 8192 && !(channel_mode && prefetch == 0 && n <= 256);
}

// store16_at (sp_kernel_frames.h) for the index write-out: the same `global_store_dwordx4 voff, data, s[base]`, followed by the two
// wait states a VALU write to the data registers of a store of more than 64 bits needs behind it on gfx950 (the store reads them late; the
// compiler cannot see a store issued as inline asm and schedules the next item's address arithmetic into these registers).  Observed, not
// assumed: with store16_at the check of tests/test_isa_checks.py (no VALU write on a wide store's data within two wait states) found 58
// such pairs in the index objects - `global_store_dwordx4 v13, v[4:7], s[2:3]` followed at once by `v_sub_u32 v4, ...`.  The same check
// passes on k_frames, k_frames_batch and k_frames_peak as they are compiled: their drain keeps 32 pixel registers alive across the
// stores, so nothing is written into a store's data that early.
__device__ inline void store16_at_index(uint8_t *base, unsigned off, uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    const u32x4 v = {a, b, c, d};
#if SP_INDEX_NT   // (kernel experiments, tools/build_variant.sh: the non-temporal row pieces DESIGN.md section 13 measures against these)
    asm volatile("global_store_dwordx4 %0, %1, %2 nt\n\ts_nop 1" ::"v"(off), "v"(v), "s"(base) : "memory");
#else
    asm volatile("global_store_dwordx4 %0, %1, %2\n\ts_nop 1" ::"v"(off), "v"(v), "s"(base) : "memory");
#endif
}

template <int LOG2N, bool CH, int PFB>
__global__ __launch_bounds__(kFrameThreads, 1) void k_frames_index(const FrameArgs a, const int format, const double2 *__restrict__ stage_tw,
                                                       const int group_frames, const int groups)
{
#include "sp_frames_setup.inc.h"

#include "sp_frames_raw_regs.inc.h"
    auto request = [&](int xq) {
        if constexpr (PF) {
            const int xc = xq < a.x_end ? xq : a.x_end - 1;
            constexpr bool UNI = T >= 64;   // a frame per wave or more: its start is wave-uniform
            const int sv = frame_start_in_bounds(a.stride, xc);
            const int64_t st = UNI ? __builtin_amdgcn_readfirstlane(sv) : sv;
            if constexpr (PFB == 3) raw_back = (st + N) * 3 + 1 > a.nbytes ? 1 : 0;
            issue_raw<PFB, UNI>(a.bytes, st, T, sidx_pf, raw_lo, raw_hi, raw_back);
        }
    };
    const bool HALVES = T == 64 && group_frames == 32;
    const int fs0 = HALVES ? (fs / (FPB / 2)) * (group_frames / 2) + fs % (FPB / 2) : fs;     // the slot's frame in a group's first round
    constexpr bool REQ_AFTER_TABLES = PF && !LATE_PF && LOG2N <= 10;
    if (PF && !LATE_PF && !REQ_AFTER_TABLES && xcd * chunk + lane_in_xcd < g_end) request(a.frame0 + (xcd * chunk + lane_in_xcd) * group_frames + fs0);

    const bool owner = blockIdx.x == 0 && __builtin_amdgcn_readfirstlane(tid >> 6) == 0 && a.first;   // (wave-uniform)
    constexpr bool WIN_LDS = lds_win_in_lds(N);   // taper in LDS for n <= 1024, in registers for the whole launch above
    double *s_win = (double *)(smem + lay.off_win);
    constexpr int MMS = mm_slots(N);
    constexpr bool LATE_SIDE = late_side_outputs(N);
    {
#include "sp_frames_table_loads.inc.h"
#include "sp_frames_reply_clear.inc.h"
        if constexpr (REQ_AFTER_TABLES) request(a.frame0 + (xcd * chunk + lane_in_xcd) * group_frames + fs0);
#include "sp_frames_table_stores.inc.h"
    }

    const double *const wbase = s_win + tl;   // stored as the threads read it: entry e*T + tl = taper[rev4(e)*T + rev(tl)]
    double win_reg[WIN_LDS ? 1 : 16];
    if constexpr (!WIN_LDS) {
        const int sidx = (int)(__brev((unsigned)tl) >> (32 - (LOG2N - 4)));
#pragma unroll
        for (int e = 0; e < 16; e++) win_reg[e] = a.window[rev4(e) * T + sidx];
    }
    lds_barrier();

    const spfmt::View view{a.bytes, a.nbytes, a.nelem};
    uint32_t pf_word = 0;
#include "sp_frames_epilogue_consts.inc.h"

#define SP_DRAIN_ROWS_BODY "sp_frames_drain_rows_index.inc.h"
#include "sp_frames_writeout.inc.h"
#undef SP_DRAIN_ROWS_BODY
    int drain_x0 = -1;
    int gpar = 0;   // parity of the workgroup's current group (s_amp)
    meet.arrive();   // the first re-distribution only waits (exchange<.., SECOND = false>)
    for (int g = xcd * chunk + lane_in_xcd; g < g_end; g += per_xcd) {
        const int x0 = a.frame0 + g * group_frames;
        for (int r = 0; r < rounds; r++) {
            const int fr = HALVES ? (fs / (FPB / 2)) * (group_frames / 2) + r * (FPB / 2) + fs % (FPB / 2) : r * FPB + fs;
            const int xr = x0 + fr;
            if (fr >= group_frames) continue;   // a slot without a frame in the group's last round (its next frame is already requested)
            const bool live = xr < a.x_end;
            const int x = live ? xr : a.x_end - 1;
            const int64_t start = frame_start(a.stride, x);

            double re[16], im[16];
            double win[16];
            double2 *const centre = tl == 0 ? &s_amp[gpar * group_frames + fr] : nullptr;   // thread 0 of the frame: where its raw centre sample goes
            bool nonfinite = true;   // wave-uniform
#pragma unroll
            for (int e = 0; e < 16; e++) win[e] = WIN_LDS ? wbase[e * T] : win_reg[WIN_LDS ? 0 : e];
            const int xn = (r + 1 < rounds && (HALVES || fr + FPB < group_frames)) ? xr + (HALVES ? FPB / 2 : FPB)
                                                                         : (g + per_xcd < g_end ? a.frame0 + (g + per_xcd) * group_frames + fs0 : -1);
            if constexpr (PF && LATE_PF) request(xr);
            if constexpr (PF) {
#include "sp_frames_decode_pf.inc.h"
                if (!LATE_PF && xn >= 0) request(xn);           // in flight during this frame's butterflies
            } else {
                asm volatile("" ::"v"(pf_word));
                if (a.in_bounds && xn >= 0 && xn < a.x_end) {
                    const int lines = (N * a.sample_width + 127) >> 7;
                    const int64_t nb = (int64_t)frame_start(a.stride, xn) * a.sample_width;
                    for (int l = tl; l < lines; l += T) pf_word = *(const uint32_t *)(a.bytes + ((nb + (int64_t)l * 128) & ~(int64_t)3));
                }
                switch (format) {
#define SP_CASE(F) case F: load_frame<F>(a, view, start, tl, T, LOG2N, win, re, im, centre); break;
                    SP_FORMATS_BUT_CF64(SP_CASE)
#undef SP_CASE
                default: load_frame<SP_FMT_CF64>(a, view, start, tl, T, LOG2N, win, re, im, centre); break;
                }
            }

            unsigned tw_off = 0;
            asm volatile("" : "+s"(tw_off));
            const double2 *tw = stage_tw + tw_off;
            if (drain_x0 >= 0) {
                lds_barrier();
                if constexpr (!LATE_SIDE) side_outputs(drain_x0, gpar ^ 1);
                drain(drain_x0, 0, 2);
            }
#include "sp_frames_fft.inc.h"

#include "sp_frames_lr_split.inc.h"

            if (drain_x0 >= 0) {
                drain(drain_x0, 1, 2);
                lds_barrier();
                if constexpr (LATE_SIDE) side_outputs(drain_x0, gpar ^ 1);
                drain_x0 = -1;
            }
#include "sp_frames_pixels.inc.h"
#include "sp_frames_publish.inc.h"
        }
        drain_x0 = x0;
        gpar ^= 1;
    }

#include "sp_frames_finale.inc.h"
}

SP_DECLARE_LAUNCH_N(launch_frames_index_n, SP_SIZES_6_13)

#ifdef SP_INST_INDEX_LOG2N
// One variant's launch, or SP_ERR_UNSUPPORTED for a variant the register rule drops: inside a template the discarded branch is not
// instantiated, so such a variant is not compiled either.
template <int L, bool C, int P>
inline int launch_frames_index_variant(SP_LAUNCH_N_PARAMS)
{
    (void)prefetch;
    if constexpr (frames_index_variant_built(1 << L, C, P)) {
        SP_LAUNCH_VARIANT_CP(k_frames_index, C, P)
    } else {
        return SP_ERR_UNSUPPORTED;
    }
}

template <>
int launch_frames_index_n<SP_INST_INDEX_LOG2N>(SP_LAUNCH_N_PARAMS)
{
    constexpr int L = SP_INST_INDEX_LOG2N;
#define SP_INDEX_C(C)                                                                                                  \
    switch (prefetch) {                                                                                                \
    case 8: return launch_frames_index_variant<L, C, 8>(a, format, stage_tw, fl, prefetch, device, stream);            \
    case 4: return launch_frames_index_variant<L, C, 4>(a, format, stage_tw, fl, prefetch, device, stream);            \
    case 3: return launch_frames_index_variant<L, C, 3>(a, format, stage_tw, fl, prefetch, device, stream);            \
    case 2: return launch_frames_index_variant<L, C, 2>(a, format, stage_tw, fl, prefetch, device, stream);            \
    case 1: return launch_frames_index_variant<L, C, 1>(a, format, stage_tw, fl, prefetch, device, stream);            \
    default: return launch_frames_index_variant<L, C, 0>(a, format, stage_tw, fl, prefetch, device, stream);           \
    }
    if (a.channel_mode) { SP_INDEX_C(true) } else { SP_INDEX_C(false) }
#undef SP_INDEX_C
}
#endif

// Host-side launch over frames [a.frame0, a.x_end) into the index image at a.rgba; groups and grid by the launch rule, as launch_frames.
// Returns SP_OK or SP_ERR_UNSUPPORTED.
inline int launch_frames_index(const FrameArgs &a, int format, const double2 *stage_tw, int cu_count, int device, hipStream_t stream)
{
    const int prefetch = frames_prefetch_width(a.sample_width, a.in_bounds, a.stride, a.width);
    FramesLaunch fl;
    if (frames_launch_rule(a.n, a.lut_len, a.x_end - a.frame0, cu_count, 0, fl)) return SP_ERR_UNSUPPORTED;
    switch (a.levels) {
#define SP_L(L) case L: return launch_frames_index_n<L>(a, format, stage_tw, fl, prefetch, device, stream);
        SP_L(6) SP_L(7) SP_L(8) SP_L(9) SP_L(10) SP_L(11) SP_L(12) SP_L(13)
#undef SP_L
    default: return SP_ERR_UNSUPPORTED;
    }
}

}  // namespace spk2
