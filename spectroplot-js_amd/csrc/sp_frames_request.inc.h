// Frame-loop fragment (k_frames, k_frames_index, k_frames_traces, k_frames_power): the lambda `request`, which asks for the raw words of
// frame xq of the request's capture (a frame past the end is clamped to the last one).  k_frames_batch spells its own: capture, length,
// stride and end come from an item record it fetches first - four macros and a hook.  k_frames_peak has the inner half, request_at.
// Expects in scope: PF, PFB, N, T, a, sidx_pf, raw_lo, raw_hi, raw_back.
    auto request = [&](int xq) {
        if constexpr (PF) {
            // (the prefetching variants only run when every frame lies inside the buffer: frames_prefetch_width)
            const int xc = xq < a.x_end ? xq : a.x_end - 1;
            constexpr bool UNI = T >= 64;   // a frame per wave or more: its start is wave-uniform
            const int sv = frame_start_in_bounds(a.stride, xc);
            const int64_t st = UNI ? __builtin_amdgcn_readfirstlane(sv) : sv;
            if constexpr (PFB == 3) raw_back = (st + N) * 3 + 1 > a.nbytes ? 1 : 0;
            issue_raw<PFB, UNI>(a.bytes, st, T, sidx_pf, raw_lo, raw_hi, raw_back);
        }
    };
