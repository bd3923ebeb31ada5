// Histogram-flush fragment: the workgroup's counts added to the reply's histograms.
// Expects in scope: tid, kThreads, s_pre, cg_lo, cg_hi, l_lo, l_hi; SP_CELLS, SP_LUT_LEN; SP_REPLY: what holds out_c and out_cb.
        const int sp0 = SP_CELLS - 2, sp1 = SP_CELLS - 1;                       // -inf / NaN dB (colour 0, bin 0); +inf dB (last colour, bin 0)
        const unsigned int n0 = s_pre[sp0 + 1] - s_pre[sp0], n1 = s_pre[sp1 + 1] - s_pre[sp1];
        unsigned long long *const out_c = SP_REPLY->out_c, *const out_cb = SP_REPLY->out_cb;
        if (tid < SP_LUT_LEN && out_c) {
            const unsigned int cnt = s_pre[cg_hi] - s_pre[cg_lo] + (tid == 0 ? n0 : 0u) + (tid == SP_LUT_LEN - 1 ? n1 : 0u);
            if (cnt) atomicAdd(&out_c[tid], (unsigned long long)cnt);
        }
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const int gi = tid + u * kThreads;
            if (gi < SP_CB_HIST_SIZE && out_cb) {
                const unsigned int cnt = s_pre[l_hi[u]] - s_pre[l_lo[u]] + (gi == 0 ? n0 + n1 : 0u);
                if (cnt) atomicAdd(&out_cb[gi], (unsigned long long)cnt);
            }
        }
