// Frame-loop fragment: the FFT passes, from the first pass (literal twiddles) to the last.
// Expects in scope: re, im, tl, xbuf, meet, s_tw, tw, nonfinite, LOG2N, PFB, NPASS, TWMAX, STAGED, PERMLANE_MID, BLOCK_SYNC.
            // ---- first pass: literal twiddles ------------------------------------------------------------------------------
            if constexpr (PFB == 0) {
                fft_pass1<false>(re, im);            // frames may leave the buffer (NaN samples), 16-byte formats
            } else if constexpr (PFB == 8) {
                if (nonfinite) fft_pass1<false>(re, im);
                else fft_pass1<true>(re, im);
            } else {
                fft_pass1<true>(re, im);             // integer samples times a finite taper (sp_api.hip: plan_frames_capable)
            }
            if constexpr (NPASS >= 2) {
                constexpr int WS1 = LOG2N >= 8 ? 4 : LOG2N - 4;
                constexpr int E1 = LOG2N >= 8 ? 8 : LOG2N;
                double *const b0 = xbuf + pad_idx(win_pos(tl, 0, 0)), *const b1 = xbuf + pad_idx(win_pos(tl, 0, WS1));
                PassTw<WS1, 5, STAGED ? 4 : E1, TWMAX> tw1;
                if constexpr (!STAGED) load_pass_tw(tw1, tl, s_tw, tw);
                // The first re-distribution never leaves a wave, whatever n: under window 0 as under window [4,8) the 64 threads of a
                // wave hold exactly the positions [1024 w, 1024 w + 1023] of their frame.  So the waves of a frame (n >= 2048) only
                // wait, before its first writes, for the partners' last reads of the frame before; between its writes and reads the
                // LDS's in-order execution of a wave's operations is all that is needed, as at n <= 1024.
                meet.wait();
                exchange<0, WS1, false, false>(re, b0, b1);
                exchange<0, WS1, false, true>(im, b0, b1);
                exchange_wait(re, im);
                if constexpr (STAGED) fft_pass_staged<WS1, 5, E1, TWMAX>(re, im, tl, s_tw, tw);
                else fft_pass<WS1, 5, E1>(re, im, tw1);
                if constexpr (PERMLANE_MID) {
                    // n = 8192: the second re-distribution stays inside the wave too - the register transpose of the 1024-point
                    // layout (window [4,8) -> [6,10) of the wave's block), two stages there, and only then the one re-distribution
                    // that crosses waves, to window [9,13) for the last three stages.  Four workgroup barriers per frame instead of
                    // eight; the swaps cost the VALU, which has the time at this size.
                    PassTw<6, 9, STAGED ? 8 : 10, TWMAX> tw2;
                    if constexpr (!STAGED) load_pass_tw(tw2, tl, s_tw, tw);
                    exchange_permlane<10>(re);
                    exchange_permlane<10>(im);
                    if constexpr (STAGED) fft_pass_staged<6, 9, 10, TWMAX>(re, im, tl, s_tw, tw);
                    else fft_pass<6, 9, 10>(re, im, tw2);
                    constexpr int WS3 = LOG2N - 4;
                    double *const b2 = xbuf + pad_idx(win_pos(tl, 0, 6)), *const b3 = xbuf + pad_idx(win_pos(tl, 0, WS3));
                    PassTw<WS3, 11, STAGED ? 10 : LOG2N, TWMAX> tw3;
                    if constexpr (!STAGED) load_pass_tw(tw3, tl, s_tw, tw);
                    exchange<6, WS3, BLOCK_SYNC, false, decltype(meet) &, false>(re, b2, b3, meet);
                    exchange<6, WS3, BLOCK_SYNC, true>(im, b2, b3, meet);
                    exchange_wait(re, im);
                    if constexpr (STAGED) fft_pass_staged<WS3, 11, LOG2N, TWMAX>(re, im, tl, s_tw, tw);
                    else fft_pass<WS3, 11, LOG2N>(re, im, tw3);
                } else if constexpr (NPASS >= 3) {
                    constexpr int WS2 = LOG2N >= 12 ? 8 : LOG2N - 4;
                    constexpr int E2 = LOG2N >= 12 ? 12 : LOG2N;
                    double *const b2 = xbuf + pad_idx(win_pos(tl, 0, WS2));
                    PassTw<WS2, 9, STAGED ? 8 : E2, TWMAX> tw2;
                    if constexpr (!STAGED) load_pass_tw(tw2, tl, s_tw, tw);
                    if constexpr (LOG2N == 9 || LOG2N == 10) {
                        // two register bits against lane bits 4 / 5: v_permlane16_swap / v_permlane32_swap.  The swaps cost the VALU
                        // about what the LDS round trip costs the LDS pipe (measured: 1.2 % of the kernel in favour of the swaps)
                        exchange_permlane<LOG2N>(re);
                        exchange_permlane<LOG2N>(im);
                    } else {
                        // (writes the positions the wave itself read last: no wait before them)
                        exchange<WS1, WS2, BLOCK_SYNC, false, decltype(meet) &, false>(re, b1, b2, meet);
                        exchange<WS1, WS2, BLOCK_SYNC, true>(im, b1, b2, meet);
                        exchange_wait(re, im);
                    }
                    if constexpr (STAGED) fft_pass_staged<WS2, 9, E2, TWMAX>(re, im, tl, s_tw, tw);
                    else fft_pass<WS2, 9, E2>(re, im, tw2);
                    static_assert(NPASS <= 3, "four passes (n = 8192) take the register-transpose branch above");
                }
            }
            // now register e of thread tl holds bin i = tl + e*T
