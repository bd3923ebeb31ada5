// Frame-loop fragment: the L/R split of channel mode (CH), partner bins through LDS.
// Expects in scope: re, im, tl, xbuf, meet, LOG2N, N, T, CH.
            if constexpr (CH) {   // fft_nayuki.js:103-119, partner bin n-i fetched through LDS
                // (the partner values eight at a time where registers are short, n >= 2048: two LDS waits per component instead of one,
                // and 16 registers fewer at the frame's register peak)
                constexpr int PH = LOG2N >= 11 ? 8 : 16;
                double pp[PH];
                meet.wait();   // (announced after the last re-distribution's reads)
#pragma unroll
                for (int e = 0; e < 16; e++) xbuf[pad_idx(tl + e * T)] = re[e];
                meet();
#pragma unroll
                for (int h = 0; h < 16; h += PH) {
#pragma unroll
                    for (int k = 0; k < PH; k++) pp[k] = xbuf[pad_idx((N - (tl + (h + k) * T)) & (N - 1))];
#pragma unroll
                    for (int k = 0; k < PH; k++) {
                        const int e = h + k, i = tl + e * T;
                        const double orr = re[e];
                        if (i == 0) {
                        } else if (i == N / 2) {
                            re[e] = 0.0;
                        } else if (i < N / 2) {
                            re[e] = 0.5 * (orr + pp[k]);
                        } else {
                            re[e] = 0.5 * (-pp[k] + orr);
                        }
                    }
                    if (PH < 16) asm volatile("" ::: "memory");   // the second half's reads stay behind the first half's arithmetic
                }
                meet();
#pragma unroll
                for (int e = 0; e < 16; e++) xbuf[pad_idx(tl + e * T)] = im[e];
                meet();
#pragma unroll
                for (int h = 0; h < 16; h += PH) {
#pragma unroll
                    for (int k = 0; k < PH; k++) pp[k] = xbuf[pad_idx((N - (tl + (h + k) * T)) & (N - 1))];
#pragma unroll
                    for (int k = 0; k < PH; k++) {
                        const int e = h + k, i = tl + e * T;
                        const double oi = im[e];
                        if (i == 0 || i == N / 2) {
                            im[e] = 0.0;
                        } else if (i < N / 2) {
                            im[e] = 0.5 * (oi - pp[k]);
                        } else {
                            im[e] = 0.5 * (pp[k] + oi);
                        }
                    }
                    if (PH < 16) asm volatile("" ::: "memory");
                }
                meet.arrive();   // for the next frame's first re-distribution
            }
