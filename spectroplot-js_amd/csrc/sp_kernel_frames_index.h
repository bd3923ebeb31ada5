// sp_kernel_frames_index.h — k_frames_index: the frame loop of k_frames with an INDEXED image, 64 <= n <= 8192.
//
// An indexed request (include/spectroplot_hip.h, sp_plan_execute_index) asks for the picture as one colour-index byte per pixel - the
// value `gray` of lib/worker.js that c_hist counts - instead of the RGBA the LUT makes of it.  The frame loop already leaves that byte per
// bin in its LDS tile (sp_frames_pixels.inc.h); this kernel is k_frames' body (sp_frames_request_body.inc.h; sp_kernel_frames.h lists
// the fragments and says why they are textual) with ONE fragment exchanged: the body of drain_rows is sp_frames_drain_rows_index.inc.h,
// which stores the tile's bytes themselves: no LUT read per pixel, a quarter of the store bytes.
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
// that says so: the launcher below compiles by it (SP_LAUNCH_VARIANT_IF), sp_api.hip dispatches by it.
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
#define SP_DRAIN_ROWS_BODY "sp_frames_drain_rows_index.inc.h"
#include "sp_frames_request_body.inc.h"
#undef SP_DRAIN_ROWS_BODY
}

SP_DECLARE_LAUNCH_N(launch_frames_index_n, SP_SIZES_6_13)

#ifdef SP_INST_INDEX_LOG2N
template <>
int launch_frames_index_n<SP_INST_INDEX_LOG2N>(SP_LAUNCH_N_PARAMS)
{
    constexpr int L = SP_INST_INDEX_LOG2N;
    SP_LAUNCH_VARIANT_IF(frames_index_variant_built, k_frames_index)
}
#endif

// Host-side launch over frames [a.frame0, a.x_end) into the index image at a.rgba; groups and grid by the launch rule, as launch_frames.
// Returns SP_OK or SP_ERR_UNSUPPORTED.
inline int launch_frames_index(const FrameArgs &a, int format, const double2 *stage_tw, int cu_count, int device, hipStream_t stream)
{
    const int prefetch = frames_prefetch_width(a.sample_width, a.in_bounds, a.stride, a.width);
    FramesLaunch fl;
    if (frames_launch_rule(a.n, a.lut_len, a.x_end - a.frame0, cu_count, 0, fl)) return SP_ERR_UNSUPPORTED;
    SP_LAUNCH_LEVELS(SP_SIZES_6_13, launch_frames_index_n)
}

}  // namespace spk2
