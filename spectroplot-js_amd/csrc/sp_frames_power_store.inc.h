// Frame-loop fragment: the epilogue of k_frames_power - |X|^2 of the frame's 16 bins per thread, one 8-byte global store each.
// Expects in scope: re, im, tl, xr, a, power, N, T.
            // register e of thread tl holds bin i = tl + e*T; its row is y = i <= n/2 ? n/2 - i : n/2 + n - i (worker.js:90).  For a fixed
            // e the frame's T lanes cover T consecutive rows, descending.  From one address per thread, row n/2 - tl of the frame, the
            // rows lie at compile-time offsets (-e*T below the fold, n - e*T above it; e = 8, bin n/2 + tl, is the fold itself: row 0
            // for tl = 0, else n - tl), so the 16 stores share one 64-bit address.  A slot past the launch's end holds the last column
            // again (the loaders' sake): it stores nothing.
            if (xr < a.x_end) {
                double *const row = power + ((size_t)xr * (size_t)N + (size_t)(N / 2 - tl));   // (64-bit: 8 * width * n passes 4 GiB)
#pragma unroll
                for (int e = 0; e < 16; e++) {
                    const double v = re[e] * re[e] + im[e] * im[e];                                 // worker.js:92
                    if (e < 8) row[-e * T] = v;
                    else if (e > 8) row[N - e * T] = v;
                    else row[tl == 0 ? -N / 2 : N / 2] = v;
                }
            }
