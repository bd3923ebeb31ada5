// Prologue fragment (k_frames, k_frames_peak): the reply's initial state, behind the table loads.
// Expects in scope: owner, tid, a.
        // Workgroup 0 of a request's first launch clears the reply's histograms and sets its dBfs range to (0, -200): its first wave
        // alone, so that the wave knows when the stores have landed (sp_frames_publish.inc.h).  Fire-and-forget, behind the table loads.
        if (owner) {
            const LateArgs la = late_args();
            unsigned long long *const out_c = la->out_c, *const out_cb = la->out_cb;
            unsigned long long *const out_mm = (unsigned long long *)la->out_minmax;
            constexpr int kClr = (kLdsMaxLut + SP_CB_HIST_SIZE + 63) / 64;
#pragma unroll
            for (int k = 0; k < kClr; k++) {
                const int i = tid + 64 * k;
                unsigned long long *const dst = i < kLdsMaxLut ? (out_c && i < a.lut_len ? out_c + i : nullptr)
                                                               : (out_cb && i < kLdsMaxLut + SP_CB_HIST_SIZE ? out_cb + (i - kLdsMaxLut) : nullptr);
                if (dst) __hip_atomic_store(dst, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            if (tid < 2 && out_mm)
                __hip_atomic_store(out_mm + tid, tid ? 0xc069000000000000ull : 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // -200.0, 0.0
        }
