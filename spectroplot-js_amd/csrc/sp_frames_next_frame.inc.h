// Frame-loop fragment (the kernels of sp_frames_request.inc.h): the frame this slot processes next, and the loaders around its request.
// Expects in scope: request, r, rounds, HALVES, fr, xr, FPB, g, per_xcd, g_end, fs0, group_frames, PF, LATE_PF, a, and what
// sp_frames_decode_pf.inc.h and sp_frames_load_generic.inc.h expect.  SP_TOUCH_AHEAD, if defined: the generic path touches the next
// frame's cache lines into pf_word (also in scope then), which the finale keeps alive.
            // the frame this slot processes next: the same slot one round on, or its frame in the workgroup's next group
            const int xn = (r + 1 < rounds && (HALVES || fr + FPB < group_frames)) ? xr + (HALVES ? FPB / 2 : FPB)
                                                                         : (g + per_xcd < g_end ? a.frame0 + (g + per_xcd) * group_frames + fs0 : -1);
            if constexpr (PF && LATE_PF) request(xr);
            if constexpr (PF) {
#include "sp_frames_decode_pf.inc.h"
                if (!LATE_PF && xn >= 0) request(xn);           // in flight during this frame's butterflies
            } else {
#ifdef SP_TOUCH_AHEAD
                asm volatile("" ::"v"(pf_word));
                if (a.in_bounds && xn >= 0 && xn < a.x_end) {
                    const int lines = (N * a.sample_width + 127) >> 7;
                    const int64_t nb = (int64_t)frame_start(a.stride, xn) * a.sample_width;
                    for (int l = tl; l < lines; l += T) pf_word = *(const uint32_t *)(a.bytes + ((nb + (int64_t)l * 128) & ~(int64_t)3));
                }
#endif
#include "sp_frames_load_generic.inc.h"
            }
