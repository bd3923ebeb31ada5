// Frame-loop fragment: where a thread reads its 16 taper values - LDS (n <= 1024) or registers filled here for the whole launch - and
// the barrier that ends the prologue.  Behind the block of sp_frames_table_loads / table_stores.inc.h.
// Expects in scope: WIN_LDS, s_win, tl, T, LOG2N, a.
    const double *const wbase = s_win + tl;   // stored as the threads read it: entry e*T + tl = taper[rev4(e)*T + rev(tl)]
    double win_reg[WIN_LDS ? 1 : 16];
    if constexpr (!WIN_LDS) {
        const int sidx = (int)(__brev((unsigned)tl) >> (32 - (LOG2N - 4)));
#pragma unroll
        for (int e = 0; e < 16; e++) win_reg[e] = a.window[rev4(e) * T + sidx];
    }
    lds_barrier();
