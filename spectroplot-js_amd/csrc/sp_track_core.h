// sp_track_core.h — the one comparison of the peak track (include/spectroplot_hip.h, sp_plan_execute_track): which of two values of
// a power plane is the stronger, and which of two equal ones wins.  Plain integer C++, no HIP: the host compiler takes it alone
// (sp_debug_band_peak, tests/cpp/track_core_check.cpp), and under hipcc the same functions are the device's (sp_kernel_track.h).
//
// The KEY of a value is its bit pattern with the sign bit cleared.  Non-negative doubles and +inf order as their keys do as unsigned
// integers (the exponent field lies above the fraction, denormals below every normal, +0.0 is key 0), and a key above that of +inf is a
// NaN - any NaN, of either sign, quiet or signalling.  So there is no floating-point compare here: -ffp-contract, the compare
// semantics of a NaN and the flush of a denormal never enter.  The plane's values are never negative (|X|^2); the sign bit of a value
// is not looked at.
//
// A candidate is a pair (key, row).  better(): the larger key wins, and of two equal keys the SMALLER ROW.  That is a strict total order
// on candidates with distinct rows, so folding a set of them gives the same best in every order and every grouping - over the lanes of
// a wave, the loads of a frame, the blocks of a window.  "Nothing yet" is the candidate (0, kNoRow): every real candidate beats it, key
// 0 included, because a real row is below kNoRow.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define SP_TRACK_FN __host__ __device__ inline
#else
#define SP_TRACK_FN inline
#endif

namespace spt {

constexpr uint64_t kSignBit = 0x8000000000000000ull;
constexpr uint64_t kInfKey = 0x7ff0000000000000ull;    // the key of +inf: the largest key that is a value
constexpr uint64_t kNanKey = 0x7fffffffffffffffull;    // a key that is a NaN (what a lane holds for a row outside its band)
constexpr uint64_t kNanBits = 0x7ff8000000000000ull;   // the NaN a band without a value replies
constexpr int32_t kNoRow = 0x7fffffff;                 // the row of "nothing yet": above every row (a row is below n <= 2^31 - 1)

SP_TRACK_FN uint64_t key_of(uint64_t bits) { return bits & ~kSignBit; }
SP_TRACK_FN bool is_nan_key(uint64_t key) { return key > kInfKey; }

// candidate a before candidate b
SP_TRACK_FN bool better(uint64_t key_a, int32_t row_a, uint64_t key_b, int32_t row_b)
{
    return (key_a > key_b) | ((key_a == key_b) & (row_a < row_b));
}

struct Best {
    uint64_t key = 0;
    int32_t row = kNoRow;
};

// the candidate (key, row) into a running best; a NaN is no candidate
SP_TRACK_FN void fold(Best &best, uint64_t key, int32_t row)
{
    const bool take = !is_nan_key(key) && better(key, row, best.key, best.row);   // (selects, not a branch around stores)
    best.key = take ? key : best.key;
    best.row = take ? row : best.row;
}

// another running best into this one ("nothing yet" loses to everything, and to itself)
SP_TRACK_FN void merge(Best &best, uint64_t key, int32_t row)
{
    const bool take = better(key, row, best.key, best.row);
    best.key = take ? key : best.key;
    best.row = take ? row : best.row;
}

// what a finished best replies: the row, or -1, and the value's bits, or a NaN's
SP_TRACK_FN int32_t row_of(const Best &best) { return best.row == kNoRow ? -1 : best.row; }
SP_TRACK_FN uint64_t peak_bits_of(const Best &best) { return best.row == kNoRow ? kNanBits : best.key; }

// The best of the rows [y0, y1) of one frame's values (bit patterns), ascending: the host side of what the kernel does, and the whole
// of sp_debug_band_peak.
SP_TRACK_FN Best band_peak(const uint64_t *bits, int32_t y0, int32_t y1)
{
    Best best;
    for (int32_t y = y0; y < y1; y++) fold(best, key_of(bits[y]), y);
    return best;
}

}  // namespace spt
