// Frame-loop fragment: the top of a round - which frame of the group this slot has (fr, xr), and the frame whose samples it loads (x:
// a slot past the request's end repeats the last frame, and `live` says so).
// Expects in scope: HALVES, fs, FPB, r, x0, group_frames; SP_X_END, the request's end.  SP_SLOT_RECORD, if defined: statements behind
// the skip that SP_X_END needs (k_frames_batch fetches its item's record there).
            // HALVES: the first waves of the SIMDs (slots 0 .. FPB/2-1) own the group's first half of the frames, the second waves the
            // other half, so that each set can write its half out by itself after the workgroup's last group
            const int fr = HALVES ? (fs / (FPB / 2)) * (group_frames / 2) + r * (FPB / 2) + fs % (FPB / 2) : r * FPB + fs;
            const int xr = x0 + fr;
            if (fr >= group_frames) continue;   // a slot without a frame in the group's last round (its next frame is already requested)
#ifdef SP_SLOT_RECORD
            SP_SLOT_RECORD
#endif
            [[maybe_unused]] const bool live = xr < SP_X_END;
            const int x = live ? xr : SP_X_END - 1;
