// Frame-loop fragment: the prologue's LDS set-up behind the table loads of sp_frames_table_loads.inc.h (win_r, tw_r, lut_r, ge_r, cb_r).
// Expects in scope: N, kThreads, WIN_LDS, MMS, LATE_SIDE, tid, a, group_frames, lay, smem, s_cells, s_done, s_red, s_mm, s_tw, s_lut,
// s_win, and the loads' WINK, NTW, TWK.
        // what needs no table is set up while the loads are in flight (a table load takes ~2.3 us at the start of a launch)
        for (int i = tid; i < a.cells; i += kThreads) s_cells[i] = 0;
        if (tid < 8) s_done[tid] = 0;
        if (tid < 2) s_red[tid] = tid ? -200.0 : 0.0;                             // worker.js:35-36
        for (int i = tid; i < (LATE_SIDE ? 2 : 1) * group_frames * MMS; i += kThreads) {
            s_mm[2 * i] = 0x7ff0000000000000ull;
            s_mm[2 * i + 1] = 0ull;
        }
#pragma unroll
        for (int k = 0; k < TWK; k++) {
            const int i = tid + k * kThreads;
            if (i < NTW) s_tw[i] = tw_r[k];
        }
        if (tid < a.lut_len) s_lut[tid] = lut_r;
        if (tid < a.lut_len) ((double *)(smem + lay.off_gedge))[tid] = ge_r;
#pragma unroll
        for (int k = 0; k < (SP_CB_HIST_SIZE + kThreads) / kThreads; k++) {
            const int i = tid + k * kThreads;
            if (i <= SP_CB_HIST_SIZE) ((double *)(smem + lay.off_cbedge))[i] = cb_r[k];
        }
        if constexpr (WIN_LDS) {
#pragma unroll
            for (int k = 0; k < WINK; k++) {
                const int i = tid + k * kThreads;
                if (i < N) s_win[i] = win_r[k];
            }
        }
