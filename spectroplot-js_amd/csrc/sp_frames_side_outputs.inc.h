// Frame-loop fragment: the body of the side_outputs lambda behind the fetch of the gauge pointers (k_frames describes it).
// Expects in scope: x0, par, tid, group_frames, la, out_min, out_max, out_amp, s_mm, s_amp, s_red, MMS, LATE_SIDE;
// SP_X_END: the frame count of the request or item.
        const double gain = la->gain, range = la->range, bn_db = la->block_norm_db;
        if (tid >= 3 * group_frames) return;
        const int role = (tid >= group_frames ? 1 : 0) + (tid >= 2 * group_frames ? 1 : 0), f = tid - role * group_frames;
        double arg;
        if (role < 2) {
            unsigned long long ext = role ? 0ull : 0x7ff0000000000000ull;
#pragma unroll
            for (int k = 0; k < MMS; k++) {
                unsigned long long *slot = s_mm + 2 * (((LATE_SIDE ? par : 0) * group_frames + f) * MMS + k) + role;
                const unsigned long long v = *slot;
                ext = role ? (v > ext ? v : ext) : (v < ext ? v : ext);
                *slot = role ? 0ull : 0x7ff0000000000000ull;
            }
            arg = __longlong_as_double((long long)ext);
        } else {
            const double2 c = s_amp[par * group_frames + f];
            arg = c.x * c.x + c.y * c.y;                                                       // worker.js:130-131
        }
        const double l5 = 5 * spjs::log10(arg);
        double v;
        if (role == 2) {
            v = l5 + gain;
        } else {
            const double d = (l5 + bn_db + gain) - gain;                                       // dBfs - gain, worker.js:100
            v = role ? (d > -200.0 ? d : -200.0) : (d < 0.0 ? d : 0.0);                        // worker.js:82-83, 102-103
            if (role) lds_max_f64(&s_red[1], v);
            else lds_min_f64(&s_red[0], v);
        }
        uint8_t *const out = role == 0 ? out_min : role == 1 ? out_max : out_amp;
        if (out && x0 + f < SP_X_END) out[x0 + f] = clamp_u8(0.5 + (range + v) * 256 / range);   // worker.js:128-136
