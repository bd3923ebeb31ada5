// sp_kernel_frames_power.h — k_frames_power: the frame loop of k_frames with the numeric spectrogram as its reply, 64 <= n <= 1024.
//
// A power request (include/spectroplot_hip.h, sp_plan_execute_power) asks for |X|^2 of every frame and bin as f64, frame-major:
// power[x * n + y], y the image row of bin i (worker.js:90).  One launch and nothing else: k_frames' frame loop up to the L/R split
// (sp_frames_plain_body.inc.h; sp_kernel_frames.h lists the fragments), and behind it two multiplies and an add per bin and 16
// eight-byte global stores per thread, straight from registers
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

#define SP_FRAME_TAIL "sp_frames_power_store.inc.h"
#include "sp_frames_plain_body.inc.h"
#undef SP_FRAME_TAIL
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
    SP_LAUNCH_LEVELS(SP_SIZES_6_10, launch_frames_power_n, power)
}

}  // namespace spk2
