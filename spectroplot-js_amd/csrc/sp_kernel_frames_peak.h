// sp_kernel_frames_peak.h — k_frames_peak: the frame loop of k_frames with the peak detector (enum sp_detector), 64 <= n <= 1024.
//
// A peak request with M = floor(stride / n) >= 2 looks at M sub-frames per column: sub-frame j starts j * n samples behind the column's
// frame and exists if j == 0 or it ends inside the capture (include/spectroplot_hip.h states the rule).  A slot of the workgroup loops
// over its column's sub-frames - decode, passes, L/R split as k_frames does a frame - and keeps per bin the largest |X|^2 so far in
// 16 registers (`hold`); sub-frames before the last end in 2 multiplies, an add and a v_max_f64 per bin, the last one runs the pixel
// epilogue of k_frames on the held values (sp_frames_pixels.inc.h with SP_ABS2 defined here).  Tiles, write-out, side outputs, merged
// histogram cells and the request-number handshake are k_frames', per column instead of per frame; groups and grid follow launch_frames'
// rule on the column count.
//   * The hold starts as NaN: v_max_f64 returns the other operand for a quiet NaN, so the first sub-frame's value is taken as it is and
//     a NaN stays only if every sub-frame gives one - the fold the header defines, without a special first iteration.
//   * Every slot runs exactly M sub-frames, whatever its column has: a column with fewer (the last one; a slot past the request's end,
//     which repeats the last column without drawing it) repeats its last existing sub-frame, which the maximum ignores.  The loop is
//     uniform over the workgroup, so the write-out's barriers inside the first sub-frame of a group are met by every wave, and one
//     column in `width` pays for it.
//   * Registers: the hold is 32 VGPRs alive across the butterflies of a loop that sits at ~245 of 256 in k_frames.  The prefetching
//     variants therefore request a sub-frame's samples when it starts (k_frames' LATE_PF order) instead of one sub-frame ahead: the 16 or
//     32 registers of the raw words are then dead during the passes, and the partner wave of the SIMD covers the load.  (Requesting one
//     sub-frame ahead spills in the I/Q variants too: profiles/peak_experiments.txt has both spill tables and the A/B.)
// The stages and the shell of the loop are the fragments sp_frames_*.inc.h (sp_kernel_frames.h says why they are textual and lists
// them); this file keeps what is the detector's: the sub-frame loop, request_at, the hold, peak_count, its launch entry.
#pragma once

#include "sp_kernel_frames.h"

namespace spk2 {

constexpr int kPeakMaxLog2N = 10;   // a frame is at most one wave: the sub-frame loop has no partner waves to meet

__host__ __device__ inline bool frames_peak_supports(int n) { return frames_kernel_supports(n) && n <= (1 << kPeakMaxLog2N); }

// How many of a column's M sub-frames exist: sub-frame j >= 1 must end at or before sample floor(sampleCount) (`nsamp`).
__host__ __device__ inline int peak_count(int64_t nsamp, int64_t p0, int n, int m)
{
    const int64_t c = (nsamp - p0) / n;
    return c < 1 ? 1 : (c > m ? m : (int)c);
}

template <int LOG2N, bool CH, int PFB>
__global__ __launch_bounds__(kFrameThreads, 1) void k_frames_peak(const FrameArgs a, const int format, const double2 *__restrict__ stage_tw,
                                                            const int group_frames, const int groups, const int peak_m,
                                                            const int peak_nsamp)
{
#include "sp_frames_setup.inc.h"
    static_assert(!BLOCK_SYNC, "a sub-frame stays inside one wave");
    (void)LATE_PF;   // (k_frames' switch: every prefetching variant here requests a sub-frame's samples when it starts)

#include "sp_frames_raw_regs.inc.h"
    // the raw words of the sub-frame that starts at sample sv (inside the capture: launch_frames_peak)
    auto request_at = [&](const int sv) {
        if constexpr (PF) {
            constexpr bool UNI = T >= 64;   // a frame per wave: its start is wave-uniform
            const int64_t st = UNI ? __builtin_amdgcn_readfirstlane(sv) : sv;
            if constexpr (PFB == 3) raw_back = (st + N) * 3 + 1 > a.nbytes ? 1 : 0;
            issue_raw<PFB, UNI>(a.bytes, st, T, sidx_pf, raw_lo, raw_hi, raw_back);
        }
    };

    const bool owner = blockIdx.x == 0 && __builtin_amdgcn_readfirstlane(tid >> 6) == 0 && a.first;   // (wave-uniform)
#include "sp_frames_prologue_consts.inc.h"
    static_assert(WIN_LDS, "n <= 1024 keeps the taper in LDS");
    {
#include "sp_frames_table_loads.inc.h"
#include "sp_frames_reply_clear.inc.h"
#include "sp_frames_table_stores.inc.h"
    }

#include "sp_frames_taper.inc.h"

    const spfmt::View view{a.bytes, a.nbytes, a.nelem};
    uint32_t pf_word = 0;
#include "sp_frames_epilogue_consts.inc.h"

#include "sp_frames_writeout.inc.h"
    int drain_x0 = -1;
    int gpar = 0;   // parity of the workgroup's current group (s_amp)
    meet.arrive();
    for (int g = xcd * chunk + lane_in_xcd; g < g_end; g += per_xcd) {
        const int x0 = a.frame0 + g * group_frames;
        for (int r = 0; r < rounds; r++) {
#define SP_X_END a.x_end
#include "sp_frames_slot_deal.inc.h"   // (a frame there is a column here)
#undef SP_X_END
            // the column's frame (sub-frame 0) and how many of its M sub-frames exist
            const int p0 = PF ? frame_start_in_bounds(a.stride, x) : frame_start(a.stride, x);
            const int cnt = peak_count(peak_nsamp, p0, N, peak_m);
            // the largest |X|^2 per bin over the sub-frames so far: v_max_f64 takes the other operand over this NaN
            double hold[16];
#pragma unroll
            for (int e = 0; e < 16; e++) hold[e] = __longlong_as_double(0x7ff8000000000000ll);
#pragma unroll 1
            for (int j = 0; j < peak_m; j++) {
                const bool last_sub = j + 1 == peak_m;
                const int64_t start = (int64_t)p0 + (int64_t)(j < cnt ? j : cnt - 1) * N;

                // thread 0 of the column's FIRST sub-frame: where the raw centre sample of gauge_amps goes
                double2 *const centre = tl == 0 && j == 0 ? &s_amp[gpar * group_frames + fr] : nullptr;
#include "sp_frames_frame_regs.inc.h"
                if constexpr (PF) {
                    request_at((int)start);
#include "sp_frames_decode_pf.inc.h"
                } else {
                    asm volatile("" ::"v"(pf_word));
#include "sp_frames_load_generic.inc.h"
                }

                // (the previous group's write-out goes around the passes of this group's first sub-frame)
#include "sp_frames_passes.inc.h"
                if (!last_sub) {
#pragma unroll
                    for (int e = 0; e < 16; e++) hold[e] = max_raw(hold[e], re[e] * re[e] + im[e] * im[e]);   // worker.js:92, held
                    continue;
                }
#define SP_ABS2(e) max_raw(hold[e], re[e] * re[e] + im[e] * im[e])
#include "sp_frames_pixels.inc.h"
#undef SP_ABS2
            }
#include "sp_frames_publish.inc.h"
        }
        drain_x0 = x0;
        gpar ^= 1;
    }

#include "sp_frames_finale.inc.h"
}

SP_DECLARE_LAUNCH_N(launch_frames_peak_n, SP_SIZES_6_10, int, int)

#ifdef SP_INST_PEAK_LOG2N
template <>
int launch_frames_peak_n<SP_INST_PEAK_LOG2N>(SP_LAUNCH_N_PARAMS, int peak_m, int peak_nsamp)
{
    constexpr int L = SP_INST_PEAK_LOG2N;
    SP_LAUNCH_VARIANT(k_frames_peak, peak_m, peak_nsamp)
}
#endif

// Host-side launch for a request with peak_m >= 2 sub-frames per column; groups and grid by the launch rule on the columns.
// peak_nsamp = floor(sampleCount).  Returns SP_OK or SP_ERR_UNSUPPORTED.
inline int launch_frames_peak(const FrameArgs &a, int format, const double2 *stage_tw, int peak_m, int peak_nsamp, int cu_count, int device,
                              hipStream_t stream)
{
    const int prefetch = frames_prefetch_width(a.sample_width, a.in_bounds, a.stride, a.width);
    FramesLaunch fl;
    if (!frames_peak_supports(a.n) || peak_m < 2 || frames_launch_rule(a.n, a.lut_len, a.x_end - a.frame0, cu_count, 0, fl)) return SP_ERR_UNSUPPORTED;
    SP_LAUNCH_LEVELS(SP_SIZES_6_10, launch_frames_peak_n, peak_m, peak_nsamp)
}

}  // namespace spk2
