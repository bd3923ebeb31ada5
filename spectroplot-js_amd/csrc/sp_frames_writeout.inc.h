// Frame-loop fragment (k_frames, k_frames_peak): the lambdas side_outputs, drain_rows and drain of a request's own reply and image.
// (k_frames_batch defines its own around the same body fragments: they read the current item's record.)
// Expects in scope: a, tid, group_frames, kThreads, and what sp_frames_side_outputs.inc.h and sp_frames_drain_rows.inc.h expect.
// SP_DRAIN_ROWS_BODY: the fragment that is drain_rows' body; the RGBA write-out unless the including kernel defines it (k_frames_index:
// sp_frames_drain_rows_index.inc.h, whose image holds one byte per pixel).
#ifndef SP_DRAIN_ROWS_BODY
#define SP_DRAIN_ROWS_BODY "sp_frames_drain_rows.inc.h"
#define SP_DRAIN_ROWS_BODY_DEFAULT
#endif
    // Side outputs of a finished group of frames (worker.js:124-136), by the workgroup's first 3 * group_frames threads: gauge_mins and
    // gauge_maxs from the frame's extreme |X|^2 (d is monotone in |X|^2, so the frame's extreme d belong to them), gauge_amps from its
    // raw centre sample: one software log10 per output.  The frame's clamped extremes are also its share of the request's dBfs range
    // (worker.js:124-125): they are folded into the workgroup's; the frame's slots are reset.
#define SP_X_END a.x_end
    auto side_outputs = [&](const int x0, const int par) {
        if (__builtin_amdgcn_readfirstlane(tid) >= 3 * group_frames) return;   // (wave-uniform: the waves that hold none of those threads)
        const LateArgs la = late_args();
        // three scalar loads, selected per lane below (the compiler turns a select between fields into ONE indexed vector load, whose
        // wait covers every outstanding vector-memory operation of the wave: the sample prefetch, ~2 us)
        uint8_t *out_min = la->gauge_mins, *out_max = la->gauge_maxs, *out_amp = la->gauge_amps;
        asm volatile("" : "+s"(out_min), "+s"(out_max), "+s"(out_amp));
#include "sp_frames_side_outputs.inc.h"
    };
    // write-out of tile rows [f0, f0 + fcount) by the threads [t0, t0 + dthreads), slice `part` of `nparts`
    auto drain_rows = [&](const int x0, const int part, const int nparts, const int f0, const int fcount, const int t0, const int dthreads,
                          const bool nt_rows) {
        const int dt = tid - t0;
        if (dt < 0) return;
        // (the image's address, width and layout are read from the argument segment here, once per write-out, instead of sitting in
        // SGPRs through every frame)
        const LateArgs la = late_args();
        uint8_t *const img = la->rgba;
        const int img_width = la->width, img_waterfall = la->waterfall, img_fast = la->rgba_fast;
#include SP_DRAIN_ROWS_BODY
    };
#undef SP_X_END
    // non-temporal stores where a group's row pieces are whole 128-byte lines (below)
    auto drain = [&](const int x0, const int part, const int nparts) { drain_rows(x0, part, nparts, 0, group_frames, 0, kThreads, group_frames >= SP_NT_MIN_GROUP); };
#ifdef SP_DRAIN_ROWS_BODY_DEFAULT
#undef SP_DRAIN_ROWS_BODY
#undef SP_DRAIN_ROWS_BODY_DEFAULT
#endif
