// Frame-loop fragment: a frame's passes and L/R split, with the previous group's write-out in two slices around them, so that its stores
// drain while the SIMDs compute.
// Expects in scope: stage_tw, and what sp_frames_fft.inc.h and sp_frames_lr_split.inc.h expect; drain_x0, gpar, LATE_SIDE and the
// lambdas side_outputs and drain, unless the kernel has no write-out and defines SP_NO_WRITEOUT.
            unsigned tw_off = 0;
            asm volatile("" : "+s"(tw_off));
            const double2 *tw = stage_tw + tw_off;
#ifndef SP_NO_WRITEOUT
            if (drain_x0 >= 0) {
                lds_barrier();
                if constexpr (!LATE_SIDE) side_outputs(drain_x0, gpar ^ 1);
                drain(drain_x0, 0, 2);
            }
#endif
#include "sp_frames_fft.inc.h"

#include "sp_frames_lr_split.inc.h"

#ifndef SP_NO_WRITEOUT
            if (drain_x0 >= 0) {
                drain(drain_x0, 1, 2);
                lds_barrier();
                // The previous group's side outputs, here: the two waves that evaluate them (a software log10, ~1 us) next meet the
                // others at the start of the following group, where the first waves of the SIMDs arrive early anyway; in front of this
                // barrier they held everybody up.  (The frames' extremes and centre samples are kept per group parity for it.)
                if constexpr (LATE_SIDE) side_outputs(drain_x0, gpar ^ 1);
                drain_x0 = -1;
            }
#endif
