// Frame-loop fragment: the epilogue of k_frames_traces - |X|^2 of the frame's 16 bins per thread folded into the workgroup's LDS arrays.
// Expects in scope: re, im, tl, T, s_tmin, s_tmax, pinf.
            // register e of thread tl holds bin i = tl + e*T
#pragma unroll
            for (int e = 0; e < 16; e++) {
                const double v = re[e] * re[e] + im[e] * im[e];                                   // worker.js:92
                atomicMin(&s_tmin[tl + e * T], (unsigned long long)__double_as_longlong(min_raw(pinf, v)));
                atomicMax(&s_tmax[tl + e * T], (unsigned long long)__double_as_longlong(max_raw(0.0, v)));
            }
