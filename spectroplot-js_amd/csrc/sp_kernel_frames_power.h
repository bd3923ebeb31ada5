// sp_kernel_frames_power.h — k_frames_power: the frame loop of k_frames with the numeric spectrogram as its reply, 64 <= n <= 1024.
//
// A power request (include/spectroplot_hip.h, sp_plan_execute_power) asks for |X|^2 of every frame and bin as f64, frame-major:
// power[x * n + y], y the image row of bin i (worker.js:90).  One launch and nothing else: k_frames' frame loop - the same launch rule,
// deal of groups to workgroups, loaders, LATE_PF order and HALVES slot mapping, the stages from the fragments sp_frames_*.inc.h - up to
// the L/R split, and behind it two multiplies and an add per bin and 16 eight-byte global stores per thread, straight from registers
// (sp_frames_power_store.inc.h).  There is no reply clear, write-out, publication, finale or pixel epilogue, no LDS array beyond the
// tables and the exchange buffers, no atomic, no workspace and no request number: every value is written once by the one thread that
// computed it, so the plane does not depend on the deal of frames to workgroups and the launch may be captured into a graph.
// Unlike the traces' fold a store cannot be repeated harmlessly: a slot past the launch's end (the ragged last group) or without a frame
// in a group's last round stores nothing.
#pragma once

#include "sp_kernel_frames.h"

namespace spk2 {

constexpr int kPowerMaxLog2N = 10;   // a frame is at most one wave (as for the traces)

__host__ __device__ inline bool frames_power_supports(int n) { return frames_kernel_supports(n) && n <= (1 << kPowerMaxLog2N); }

template <int LOG2N, bool CH, int PFB>
__global__ __launch_bounds__(kFrameThreads, 1) void k_frames_power(const FrameArgs a, const int format, const double2 *__restrict__ stage_tw,
                                                             const int group_frames, const int groups, double *const power)
{
#include "sp_frames_setup.inc.h"
    static_assert(!BLOCK_SYNC, "a frame stays inside one wave");
    (void)edge_g, (void)edge_cb, (void)s_amp, (void)tile_pitch, (void)cmax, (void)s_tile;   // (the picture's: not used here)

#include "sp_frames_raw_regs.inc.h"
    auto request = [&](int xq) {
        if constexpr (PF) {
            // (the prefetching variants only run when every frame lies inside the buffer: launch_frames_power)
            const int xc = xq < a.x_end ? xq : a.x_end - 1;
            constexpr bool UNI = T >= 64;   // a frame per wave: its start is wave-uniform
            const int sv = frame_start_in_bounds(a.stride, xc);
            const int64_t st = UNI ? __builtin_amdgcn_readfirstlane(sv) : sv;
            if constexpr (PFB == 3) raw_back = (st + N) * 3 + 1 > a.nbytes ? 1 : 0;
            issue_raw<PFB, UNI>(a.bytes, st, T, sidx_pf, raw_lo, raw_hi, raw_back);
        }
    };
    const bool HALVES = T == 64 && group_frames == 32;   // (as in k_frames)
    const int fs0 = HALVES ? (fs / (FPB / 2)) * (group_frames / 2) + fs % (FPB / 2) : fs;

    constexpr bool WIN_LDS = lds_win_in_lds(N);
    static_assert(WIN_LDS, "n <= 1024 keeps the taper in LDS");
    double *s_win = (double *)(smem + lay.off_win);
    constexpr int MMS = mm_slots(N);
    constexpr bool LATE_SIDE = late_side_outputs(N);
    {
#include "sp_frames_table_loads.inc.h"
        // the first frame's samples behind the table loads, unconditionally, as in k_frames
        if constexpr (PF && !LATE_PF) request(a.frame0 + (xcd * chunk + lane_in_xcd) * group_frames + fs0);
#include "sp_frames_table_stores.inc.h"
    }

    const double *const wbase = s_win + tl;   // stored as the threads read it: entry e*T + tl = taper[rev4(e)*T + rev(tl)]
    lds_barrier();

    const spfmt::View view{a.bytes, a.nbytes, a.nelem};
    meet.arrive();
    for (int g = xcd * chunk + lane_in_xcd; g < g_end; g += per_xcd) {
        const int x0 = a.frame0 + g * group_frames;
        for (int r = 0; r < rounds; r++) {
            const int fr = HALVES ? (fs / (FPB / 2)) * (group_frames / 2) + r * (FPB / 2) + fs % (FPB / 2) : r * FPB + fs;
            const int xr = x0 + fr;
            if (fr >= group_frames) continue;   // a slot without a frame in the group's last round (its next frame is already requested)
            const int x = xr < a.x_end ? xr : a.x_end - 1;   // past the end: the last column's samples again, and no store below
            const int64_t start = frame_start(a.stride, x);

            double re[16], im[16];
            double win[16];
            double2 *const centre = nullptr;   // (no gauge_amps here)
            bool nonfinite = true;   // wave-uniform
#pragma unroll
            for (int e = 0; e < 16; e++) win[e] = wbase[e * T];
            // the frame this slot processes next: the same slot one round on, or its frame in the workgroup's next group
            const int xn = (r + 1 < rounds && (HALVES || fr + FPB < group_frames)) ? xr + (HALVES ? FPB / 2 : FPB)
                                                                         : (g + per_xcd < g_end ? a.frame0 + (g + per_xcd) * group_frames + fs0 : -1);
            if constexpr (PF && LATE_PF) request(xr);
            if constexpr (PF) {
#include "sp_frames_decode_pf.inc.h"
                if (!LATE_PF && xn >= 0) request(xn);           // in flight during this frame's butterflies
            } else {
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
#include "sp_frames_fft.inc.h"

#include "sp_frames_lr_split.inc.h"

#include "sp_frames_power_store.inc.h"
        }
    }
}

SP_DECLARE_LAUNCH_N(launch_frames_power_n, SP_SIZES_6_10, double *)

#ifdef SP_INST_POWER_LOG2N
template <>
int launch_frames_power_n<SP_INST_POWER_LOG2N>(SP_LAUNCH_N_PARAMS, double *power)
{
    constexpr int L = SP_INST_POWER_LOG2N;
    SP_LAUNCH_VARIANT(k_frames_power, power)
}
#endif

// The LUT length k_frames' layout is computed with here: a plane has no colours, so the plan's own must not matter.
constexpr int kPowerLutLen = 2;

// Host-side launch over frames [a.frame0, a.x_end) into the plane at `power` (frame x at power + x * n).  `a.lut_len` must be
// kPowerLutLen and `a.cells` 0 (the shared prologue sizes its table copies by them).  Returns SP_OK or SP_ERR_UNSUPPORTED.
inline int launch_frames_power(const FrameArgs &a, int format, const double2 *stage_tw, double *power, int cu_count, int device, hipStream_t stream)
{
    const int prefetch = frames_prefetch_width(a.sample_width, a.in_bounds, a.stride, a.width);
    FramesLaunch fl;
    if (!frames_power_supports(a.n) || a.lut_len != kPowerLutLen || a.cells != 0
        || frames_launch_rule(a.n, a.lut_len, a.x_end - a.frame0, cu_count, 0, fl))
        return SP_ERR_UNSUPPORTED;
    switch (a.levels) {
#define SP_L(L) case L: return launch_frames_power_n<L>(a, format, stage_tw, fl, prefetch, device, stream, power);
        SP_L(6) SP_L(7) SP_L(8) SP_L(9) SP_L(10)
#undef SP_L
    default: return SP_ERR_UNSUPPORTED;
    }
}

}  // namespace spk2
