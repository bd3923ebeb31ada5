// Frame-loop fragment: the body of a kernel without a picture (k_frames_traces, k_frames_power) behind its setup - k_frames' loop up to
// the L/R split, without reply clear, write-out, publication or finale.  A slot past the request's end loads the last frame again.
// Expects in scope: what sp_frames_setup.inc.h declares.  SP_FRAME_TAIL: the fragment that is the kernel's epilogue per frame.
// SP_AFTER_TABLES, if defined: statements behind the prologue's table stores.
#include "sp_frames_raw_regs.inc.h"
#include "sp_frames_request.inc.h"
#include "sp_frames_prologue_consts.inc.h"
    static_assert(WIN_LDS, "n <= 1024 keeps the taper in LDS");
    {
#include "sp_frames_table_loads.inc.h"
        // the first frame's samples behind the table loads, unconditionally, as in sp_frames_request_body.inc.h
        if constexpr (PF && !LATE_PF) request(a.frame0 + (xcd * chunk + lane_in_xcd) * group_frames + fs0);
#include "sp_frames_table_stores.inc.h"
#ifdef SP_AFTER_TABLES
        SP_AFTER_TABLES
#endif
    }
#include "sp_frames_taper.inc.h"

    const spfmt::View view{a.bytes, a.nbytes, a.nelem};
    meet.arrive();
    for (int g = xcd * chunk + lane_in_xcd; g < g_end; g += per_xcd) {
        const int x0 = a.frame0 + g * group_frames;
        for (int r = 0; r < rounds; r++) {
#define SP_X_END a.x_end
#include "sp_frames_slot_deal.inc.h"
#undef SP_X_END
            const int64_t start = frame_start(a.stride, x);
            double2 *const centre = nullptr;   // (no gauge_amps here)
#include "sp_frames_frame_regs.inc.h"
#include "sp_frames_next_frame.inc.h"

#define SP_NO_WRITEOUT
#include "sp_frames_passes.inc.h"
#undef SP_NO_WRITEOUT

#include SP_FRAME_TAIL
        }
    }
