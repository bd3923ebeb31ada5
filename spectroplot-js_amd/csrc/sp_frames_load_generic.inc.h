// Frame-loop fragment: the generic (checked) loaders - the format switch over load_frame.
// Expects in scope: format, a, view, start, tl, T, LOG2N, win, re, im, centre.
                switch (format) {
#define SP_CASE(F) case F: load_frame<F>(a, view, start, tl, T, LOG2N, win, re, im, centre); break;
                    SP_FORMATS_BUT_CF64(SP_CASE)
#undef SP_CASE
                default: load_frame<SP_FMT_CF64>(a, view, start, tl, T, LOG2N, win, re, im, centre); break;
                }
