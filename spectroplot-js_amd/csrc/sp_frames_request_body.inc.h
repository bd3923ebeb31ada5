// Frame-loop fragment: the whole body of a kernel that renders one request's picture - k_frames, and k_frames_index with
// SP_DRAIN_ROWS_BODY defined around it (sp_frames_writeout.inc.h).
// Expects in scope: the kernel's template parameters LOG2N, CH, PFB and its arguments a, format, stage_tw, group_frames, groups.
#include "sp_frames_setup.inc.h"

#include "sp_frames_raw_regs.inc.h"
#include "sp_frames_request.inc.h"
    // n <= 1024 requests the first frame's samples behind the table loads, below (config 2: -1.6 us per launch); above, where the tables
    // are a quarter of the size and the taper goes to registers after them, the old order measures the same (n = 2048) or 1.3 % better
    // (n = 8192: the other order shifts the loop's register allocation)
    constexpr bool REQ_AFTER_TABLES = PF && !LATE_PF && LOG2N <= 10;
    if (PF && !LATE_PF && !REQ_AFTER_TABLES && xcd * chunk + lane_in_xcd < g_end) request(a.frame0 + (xcd * chunk + lane_in_xcd) * group_frames + fs0);

    // workgroup 0's first wave owns the reply's initial state in the first launch of a request (below)
    const bool owner = blockIdx.x == 0 && __builtin_amdgcn_readfirstlane(tid >> 6) == 0 && a.first;   // (wave-uniform)
#include "sp_frames_prologue_consts.inc.h"
    {
#include "sp_frames_table_loads.inc.h"
#include "sp_frames_reply_clear.inc.h"
        // The first frame's samples are requested BEHIND the table loads (vector-memory operations complete in order: requested ahead of
        // them, the wait for the tables - L2 hits - was a wait for the samples from HBM), and unconditionally (a frame past the end is
        // clamped), so that the compiler can count the 16 younger loads in that wait: s_waitcnt vmcnt(16).
        if constexpr (REQ_AFTER_TABLES) request(a.frame0 + (xcd * chunk + lane_in_xcd) * group_frames + fs0);
#include "sp_frames_table_stores.inc.h"
    }
#include "sp_frames_taper.inc.h"

    const spfmt::View view{a.bytes, a.nbytes, a.nelem};
    uint32_t pf_word = 0;
#include "sp_frames_epilogue_consts.inc.h"

#include "sp_frames_writeout.inc.h"
    int drain_x0 = -1;
    int gpar = 0;   // parity of the workgroup's current group (s_amp)
    meet.arrive();   // the first re-distribution only waits (exchange<.., SECOND = false>)
    for (int g = xcd * chunk + lane_in_xcd; g < g_end; g += per_xcd) {
        const int x0 = a.frame0 + g * group_frames;
        for (int r = 0; r < rounds; r++) {
#define SP_X_END a.x_end
#include "sp_frames_slot_deal.inc.h"
#undef SP_X_END
            const int64_t start = frame_start(a.stride, x);
            double2 *const centre = tl == 0 ? &s_amp[gpar * group_frames + fr] : nullptr;   // thread 0 of the frame: where its raw centre sample goes
#include "sp_frames_frame_regs.inc.h"
#define SP_TOUCH_AHEAD
#include "sp_frames_next_frame.inc.h"
#undef SP_TOUCH_AHEAD

#include "sp_frames_passes.inc.h"
#include "sp_frames_pixels.inc.h"
#include "sp_frames_publish.inc.h"
        }
        drain_x0 = x0;
        gpar ^= 1;
    }

#include "sp_frames_finale.inc.h"
