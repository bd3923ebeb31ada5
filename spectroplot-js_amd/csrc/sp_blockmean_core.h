// sp_blockmean_core.h — the two decisions of the averaged spectrogram (include/spectroplot_hip.h, sp_plan_execute_blockmean and
// sp_plan_power_to_index) that are no sums: what becomes of a run of frames, and which colour index a power takes.  Plain integer C++,
// no HIP, in the manner of sp_burst_core.h: the host compiler takes it alone (sp_debug_blockmean_split, sp_debug_gray_index,
// tests/cpp/blockmean_core_check.cpp), and under hipcc the same functions are the device's (sp_kernel_blockmean.h).  The sums themselves
// are sp_exact_sum.h's.
//
// Column c of a request of `width` frames averaged `group` frames at a time covers the frames [c * group, min((c + 1) * group, width)):
// only the last column can be short.  A plane consumer receives the request's frames in runs [x_base, x_base + frames), ascending and
// contiguous, that end wherever a window block or a chunk ends.  split() cuts a run into at most three parts, in this order:
//   head   the frames that continue a column an earlier run began (x_base is no multiple of group); it ends where that column ends, or
//          with the run if the run ends first - the column then stays open and the next run has a head again;
//   body   whole columns, the short last one included where the run reaches `width`;
//   tail   the frames that begin a column a later run will finish.
// Head and tail are CARRIED: added into the per-row cells of a workspace that is cleared where a column begins and finished where it
// ends.  The body's columns are made by one launch of k_blockmean, the DIRECT path, where group <= direct_max, and carried one by one
// otherwise.  Both paths add the same integers into the same cells and round once, so direct_max changes speed only, never a bit.
//
// gray_index() is the colour index of lib/worker.js:105-117 as sp_host.h's Thresholds state it, gray(abs2) = #{ g in 1 .. lut_len - 1 :
// abs2 >= gray_edge[g] }, decided on bit patterns: non-negative doubles and +inf order as their keys do as unsigned integers
// (sp_track_core.h), and the edges are positive doubles or +inf, never a NaN, and do not decrease.  A NaN takes index 0, as does 0;
// +inf reaches every edge, the unreachable ones (+inf) included, and takes the last index.  No floating-point compare.
#pragma once

#include <cstdint>

#include "sp_track_core.h"

namespace spbm {

// ceil(width / group) in 64 bits; 0 where there is no frame or no group
SP_TRACK_FN int64_t columns(int64_t width, int64_t group) { return width <= 0 || group < 1 ? 0 : (width + group - 1) / group; }

struct Split {
    int64_t head = 0, body = 0, tail = 0;   // frames of the three parts: head + body + tail == the run's frames
    int64_t body_column = 0;                // the first column of the body
    int64_t body_columns = 0;               // ... and how many it holds
    int32_t direct = 0;                     // the body goes to k_blockmean
};

// 0 <= x_base, 0 <= frames, x_base + frames <= width, group >= 1 (the caller has checked them)
SP_TRACK_FN Split split(int64_t x_base, int64_t frames, int64_t width, int64_t group, int64_t direct_max)
{
    Split s;
    int64_t x = x_base, left = frames;
    const int64_t into = x % group;
    if (into != 0 && left > 0) {
        const int64_t full = x - into + group, end = full < width ? full : width;
        s.head = left < end - x ? left : end - x;
        x += s.head;
        left -= s.head;
    }
    if (left > 0) {   // (x is a multiple of group here)
        const int64_t whole = left / group, rest = left % group;
        const bool closes = rest != 0 && x + left == width;   // the short last column is a whole one
        s.body_column = x / group;
        s.body_columns = whole + (closes ? 1 : 0);
        s.body = closes ? left : whole * group;
        s.tail = left - s.body;
        s.direct = s.body_columns > 0 && group <= direct_max ? 1 : 0;
    }
    return s;
}

// the colour index of the value `bits` against the lut_len edges' bit patterns (edge_bits[0] is not read)
SP_TRACK_FN int32_t gray_index(const uint64_t *edge_bits, int32_t lut_len, uint64_t bits)
{
    const uint64_t key = spt::key_of(bits);
    if (spt::is_nan_key(key)) return 0;
    int32_t lo = 0, hi = lut_len - 1;   // the answer lies in [lo, hi]
    while (lo < hi) {
        const int32_t mid = (lo + hi + 1) >> 1;
        if (key >= edge_bits[mid]) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

}  // namespace spbm
