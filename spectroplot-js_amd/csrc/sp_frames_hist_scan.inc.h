// Histogram-flush fragment: the merged cells -> prefix sums s_pre (two barriers).
// Expects in scope: tid, lane, kThreads, kPer, s_cells, s_pre, s_part; SP_CELLS: the cell count; SP_AFTER_CELLS_READ: a statement for
// the moment every thread has read its cells (empty, or the batch's clear for the next item).
        unsigned int v[kPer], run = 0;
#pragma unroll
        for (int k = 0; k < kPer; k++) {
            const int c = tid * kPer + k;
            v[k] = c < SP_CELLS ? s_cells[c] : 0u;
            run += v[k];
        }
        const unsigned int incl = wave_scan_u32(run);
        if (lane == 63) s_part[tid >> 6] = incl;
        lds_barrier();
        SP_AFTER_CELLS_READ
        unsigned int base = incl - run;                                       // sum of the cells below this thread's first
        {
            const uint4 p0 = *(const uint4 *)s_part, p1 = *(const uint4 *)(s_part + 4);   // (one batch of reads, not one per wave below)
            const unsigned int part[8] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w};
            const int wave = tid >> 6;
#pragma unroll
            for (int w = 0; w < 7; w++) base += w < wave ? part[w] : 0u;
        }
#pragma unroll
        for (int k = 0; k < kPer; k++) {
            s_pre[tid * kPer + k] = base;
            base += v[k];
        }
        if (tid == kThreads - 1) s_pre[kThreads * kPer] = base;
        lds_barrier();
