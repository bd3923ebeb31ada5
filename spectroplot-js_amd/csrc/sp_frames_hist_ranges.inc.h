// Histogram-flush fragment: the cell ranges of this thread's histogram outputs.
// Expects in scope: tid, kThreads, la; SP_LUT_LEN: the LUT length.
    const uint16_t *const cell_g = la->cell_g, *const cell_l = la->cell_l;
    const int gi_c = tid < SP_LUT_LEN ? tid : 0;
    const int cg_lo = cell_g[gi_c], cg_hi = cell_g[gi_c + 1];
    int l_lo[2], l_hi[2];
#pragma unroll
    for (int u = 0; u < 2; u++) {
        const int gi = tid + u * kThreads;
        const int l_cb = gi < SP_CB_HIST_SIZE ? SP_CB_HIST_SIZE - 1 - gi : 0;              // bin gi counts level 999 - gi
        l_lo[u] = cell_l[l_cb];
        l_hi[u] = cell_l[l_cb + 1];
    }
