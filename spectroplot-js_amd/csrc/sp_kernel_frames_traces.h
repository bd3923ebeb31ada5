// sp_kernel_frames_traces.h — k_frames_traces: the frame loop of k_frames without a picture, 64 <= n <= 1024.
//
// A traces request (include/spectroplot_hip.h, sp_plan_execute_traces) asks per frequency bin for the weakest and the strongest dB
// value any column of the request shows: the min-hold and max-hold traces of a spectrum viewer.  d is monotone in |X|^2 (DESIGN.md
// section 2), so the fold over the columns runs on |X|^2 and the restated log10 is evaluated 2 n times per request, behind the loop
// (k_traces_finish).  Three launches on the context's stream, no request number and no handshake between them:
//   * k_traces_clear (sp_kernel_scratch.h, as k_traces_finish) sets the context's workspace u64[2 n] to the identities of the two
//     reductions, the bit patterns of +inf (bins' minima, words [0, n)) and +0.0 (maxima, words [n, 2 n));
//   * k_frames_traces runs k_frames' frame loop up to the L/R split (sp_frames_plain_body.inc.h; sp_kernel_frames.h lists the
//     fragments).  Its epilogue per bin (sp_frames_traces_fold.inc.h) is |X|^2, v_max_f64 with 0.0 and v_min_f64
//     with +inf (a NaN becomes the reduction's identity; |X|^2 is never negative and never -0, so the u64 order of the bit patterns is
//     the numeric order) and two fire-and-forget 64-bit LDS atomics into the workgroup's pair of arrays u64[n], which sit where k_frames
//     keeps its tile.  (In registers they would be 64 VGPRs held across a loop that sits at ~245 of 256: DESIGN.md section 11.)  A slot
//     past the request's end repeats the last column, which an idempotent fold does not notice, so the loop has no `live` bookkeeping.
//     Behind its last group a workgroup adds its arrays to the workspace, one pair of 64-bit global atomics per bin; a workgroup without
//     a group adds nothing.  There is no reply clear, write-out, publication or finale;
//   * k_traces_finish, n threads: both held values through spjs::log10 in the operation order of worker.js:93, 102 (as side_outputs
//     evaluates a frame's extremes), the fold's start values (0, -200) applied with `<` / `>`, stored at image row y (worker.js:90).
// The reductions are order-free, so the result does not depend on the deal of frames to workgroups.
#pragma once

#include "sp_kernel_frames.h"

namespace spk2 {

constexpr int kTracesMaxLog2N = 10;   // the arrays are 16 n bytes of LDS; a frame is at most one wave

__host__ __device__ inline bool frames_traces_supports(int n) { return frames_kernel_supports(n) && n <= (1 << kTracesMaxLog2N); }

// k_frames' LDS layout with the tile made large enough for the two arrays u64[n] (a group of 16 frames or more has the room already).
__host__ __device__ inline Layout traces_layout(int n, int lut_len, int group_frames)
{
    Layout l = layout(n, lut_len, group_frames);
    const int grow = 2 * n * 8 - (l.off_done - l.off_tile);
    if (grow > 0) {
        l.off_done += grow;   // (a multiple of 16: both sizes are)
        l.off_amp += grow;
        l.off_win += grow;
        l.total += grow;
    }
    return l;
}

template <int LOG2N, bool CH, int PFB>
__global__ __launch_bounds__(kFrameThreads, 1) void k_frames_traces(const FrameArgs a, const int format, const double2 *__restrict__ stage_tw,
                                                              const int group_frames, const int groups, unsigned long long *const ws)
{
#define layout traces_layout
#include "sp_frames_setup.inc.h"
#undef layout
    static_assert(!BLOCK_SYNC, "a frame stays inside one wave");
    (void)edge_g, (void)edge_cb, (void)s_amp, (void)tile_pitch, (void)cmax;   // (the picture's: not used here)
    unsigned long long *const s_tmin = (unsigned long long *)s_tile, *const s_tmax = s_tmin + N;   // the workgroup's extremes per bin
    const double pinf = __longlong_as_double(0x7ff0000000000000ll);

#define SP_AFTER_TABLES                        \
    for (int i = tid; i < N; i += kThreads) {  \
        s_tmin[i] = 0x7ff0000000000000ull;     \
        s_tmax[i] = 0ull;                      \
    }
#define SP_FRAME_TAIL "sp_frames_traces_fold.inc.h"
#include "sp_frames_plain_body.inc.h"
#undef SP_FRAME_TAIL
#undef SP_AFTER_TABLES

    // the workgroup's share goes to the workspace: one pair of atomics per bin, none from a workgroup that had no group
    if (xcd * chunk + lane_in_xcd >= g_end) return;   // (uniform over the workgroup)
    lds_barrier();
    for (int i = tid; i < N; i += kThreads) {
        atomicMin(&ws[i], s_tmin[i]);
        atomicMax(&ws[N + i], s_tmax[i]);
    }
}

SP_DECLARE_LAUNCH_N(launch_frames_traces_n, SP_SIZES_6_10, unsigned long long *)

#ifdef SP_INST_TRACES_LOG2N
template <>
int launch_frames_traces_n<SP_INST_TRACES_LOG2N>(SP_LAUNCH_N_PARAMS, unsigned long long *ws)
{
    constexpr int L = SP_INST_TRACES_LOG2N;
    SP_LAUNCH_VARIANT(k_frames_traces, ws)
}
#endif

// The LUT length k_frames' layout is computed with here: a trace has no colours, so the plan's own must not matter.
constexpr int kTracesLutLen = 2;

// Host-side launch over frames [a.frame0, a.x_end): groups and grid by the launch rule.  `a.lut_len` must be kTracesLutLen and
// `a.cells` 0 (the shared prologue sizes its table copies by them).  Returns SP_OK or SP_ERR_UNSUPPORTED.
inline int launch_frames_traces(const FrameArgs &a, int format, const double2 *stage_tw, unsigned long long *ws, int cu_count, int device,
                                hipStream_t stream)
{
    const int prefetch = frames_prefetch_width(a.sample_width, a.in_bounds, a.stride, a.width);
    FramesLaunch fl;
    if (!frames_traces_supports(a.n) || a.lut_len != kTracesLutLen || a.cells != 0
        || frames_launch_rule(a.n, a.lut_len, a.x_end - a.frame0, cu_count, 0, fl))
        return SP_ERR_UNSUPPORTED;
    fl.lds_bytes = traces_layout(a.n, a.lut_len, fl.gf).total;
    if (fl.lds_bytes > 160 * 1024) return SP_ERR_UNSUPPORTED;
    SP_LAUNCH_LEVELS(SP_SIZES_6_10, launch_frames_traces_n, ws)
}

}  // namespace spk2
