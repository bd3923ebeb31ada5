// Frame-loop fragment: the prologue's global loads of the tables (taper, twiddles, LUT, edge tables) into registers, all issued before
// the first LDS store; sp_frames_table_stores.inc.h stores them.  Both sit in one block of the kernel, around its own first request.
// Expects in scope: N, T, LOG2N, kThreads, WIN_LDS, tid, a, stage_tw.
        // tables -> LDS: every global load is issued before the first LDS store (one memory latency for the prologue)
        constexpr int WINK = WIN_LDS ? (N + kThreads - 1) / kThreads : 1;
        double win_r[WINK];
        if constexpr (WIN_LDS) {
#pragma unroll
            for (int k = 0; k < WINK; k++) {
                const int i = tid + k * kThreads, e = i / T, t = i % T;
                win_r[k] = i < N ? a.window[rev4(e) * T + (int)(__brev((unsigned)t) >> (32 - (LOG2N - 4)))] : 0.0;
            }
        }
        constexpr int NTW = frames_tw_entries(N);
        constexpr int TWK = (NTW + kThreads - 1) / kThreads;
        double2 tw_r[TWK > 0 ? TWK : 1];
#pragma unroll
        for (int k = 0; k < TWK; k++) {
            const int i = tid + k * kThreads;
            tw_r[k] = i < NTW ? stage_tw[i] : make_double2(0.0, 0.0);
        }
        const unsigned int lut_r = tid < a.lut_len ? a.lut_rgba[tid] : 0u;       // lut_len <= 256 < kThreads
        double cb_r[(SP_CB_HIST_SIZE + kThreads) / kThreads];
        const double ge_r = tid < a.lut_len ? a.gray_edge[tid] : 0.0;
#pragma unroll
        for (int k = 0; k < (SP_CB_HIST_SIZE + kThreads) / kThreads; k++) {
            const int i = tid + k * kThreads;
            cb_r[k] = i <= SP_CB_HIST_SIZE ? a.cb_edge[i] : 0.0;
        }
