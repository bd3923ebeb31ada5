// Frame-loop fragment: the prefetching loaders' decode of the frame's raw words (the PFB switch); sets nonfinite.
// Expects in scope: PFB, format, raw_lo, raw_hi, raw_back, win, re, im, centre, nonfinite.
                if constexpr (PFB == 1) {
                    if (format == SP_FMT_CU4) nonfinite = decode_frame<SP_FMT_CU4, 1>(raw_lo, raw_hi, win, re, im, centre);
                    else nonfinite = decode_frame<SP_FMT_CS4, 1>(raw_lo, raw_hi, win, re, im, centre);
                } else if constexpr (PFB == 3) {
                    if (format == SP_FMT_CU12) nonfinite = decode_frame<SP_FMT_CU12, 1>(raw_lo, raw_hi, win, re, im, centre, 8 * raw_back);
                    else nonfinite = decode_frame<SP_FMT_CS12, 1>(raw_lo, raw_hi, win, re, im, centre, 8 * raw_back);
                } else if constexpr (PFB == 2) {
                    if (format == SP_FMT_CU8) nonfinite = decode_frame<SP_FMT_CU8, 1>(raw_lo, raw_hi, win, re, im, centre);
                    else nonfinite = decode_frame<SP_FMT_CS8, 1>(raw_lo, raw_hi, win, re, im, centre);
                } else if constexpr (PFB == 4) {
                    if (format == SP_FMT_CU16) nonfinite = decode_frame<SP_FMT_CU16, 1>(raw_lo, raw_hi, win, re, im, centre);
                    else nonfinite = decode_frame<SP_FMT_CS16, 1>(raw_lo, raw_hi, win, re, im, centre);
                } else {
                    if (format == SP_FMT_CU32) nonfinite = decode_frame<SP_FMT_CU32, 16>(raw_lo, raw_hi, win, re, im, centre);
                    else if (format == SP_FMT_CS32) nonfinite = decode_frame<SP_FMT_CS32, 16>(raw_lo, raw_hi, win, re, im, centre);
                    else {
                        decode_frame<SP_FMT_CF32, 16>(raw_lo, raw_hi, win, re, im, centre);
                        nonfinite = raw_f32_nonfinite<16>(raw_lo, raw_hi);
                    }
                }
