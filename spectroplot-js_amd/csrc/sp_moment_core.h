// sp_moment_core.h — the exact WEIGHTED sum of non-negative doubles with small integer weights: the spectral moments of a band
// (include/spectroplot_hip.h, sp_plan_execute_moments), m_k = RN(sum of (y - y0)^k * power[y]).  sp_exact_sum.h's arithmetic with one
// step in front: the 53-bit integer m of a value is multiplied by its weight before it is cut into pieces.  Plain C++, no HIP: the host
// compiler takes it alone (sp_debug_moment_sum, tests/cpp/moment_core_check.cpp), and under hipcc the same functions are the device's
// (k_band_sum<1> and <2> of sp_kernel_band.h).
//
// The weight does not move a value's cell: with e the exponent field the value is m << (e - 1) in units of 2^-1074, the product is
// (m * w) << (e - 1), and cell = (e - 1) / 32 and the shift s = (e - 1) % 32 are spx::decompose's.  w <= kMaxWeight < 2^40 (a row
// distance below 2^20, squared), so m * w < 2^93 and (m * w) << s < 2^124: FOUR 32-bit pieces for the cells cell .. cell + 3.  cell <= 63,
// so an accumulator has kCells = 68 cells (cell + 3 <= 66; cell 67 only ever takes carries, and keeps the slot count even).  A value
// adds ONE piece below 2^32 to a cell and a (band, frame) has at most 2^20 values: a cell stays below 2^52.  spx::Finisher takes the 68
// cells as it takes 66 - it counts the digits it is pushed and looks at the top three - and gives +inf past DBL_MAX.
// w == 1 gives decompose's three pieces and a fourth of 0: m_0 is the band-power series bit for bit.
#pragma once

#include "sp_exact_sum.h"

namespace spm {

constexpr int kMaxOrder = 2;
constexpr int kCells = 68;
constexpr uint64_t kMaxRows = 1ull << 20;                                 // rows of a band: SP_MAX_N
constexpr uint64_t kMaxWeight = (kMaxRows - 1) * (kMaxRows - 1);          // (y - y0)^2 at the last row

// the high 64 bits of a * b
SP_XSUM_FN uint64_t mul_hi(uint64_t a, uint64_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// (y - y0)^k for the row distance r = y - y0 < 2^20; 0^0 = 1
SP_XSUM_FN uint64_t weight(uint64_t r, int k) { return k == 0 ? 1ull : k == 1 ? r : r * r; }

// The pieces of w times a double's magnitude, w <= kMaxWeight: p[j] goes to cell + j.  The kind, the cell and the shift are
// spx::decompose's; a NaN or an inf has no pieces WHATEVER its weight (the special values are the band's, not the term's).
SP_XSUM_FN int decompose_weighted(uint64_t bits, uint64_t w, int &cell, uint32_t p[4])
{
    const uint32_t e = (uint32_t)(bits >> 52) & 0x7ffu;
    const uint64_t frac = bits & 0x000fffffffffffffull;
    if (e == 0x7ffu) {
        cell = 0;
        p[0] = p[1] = p[2] = p[3] = 0;
        return frac ? spx::kNan : spx::kInf;
    }
    const uint64_t m = e ? frac | (1ull << 52) : frac;
    const uint32_t e1 = e ? e - 1 : 0;
    const uint32_t s = e1 & 31u;
    cell = (int)(e1 >> 5);
    const uint64_t lo = m * w, hi = mul_hi(m, w);                          // hi < 2^29
    const uint64_t a = lo << s;
    const uint64_t b = (hi << s) | (s ? lo >> (64 - s) : 0ull);            // (hi << 31 < 2^60: nothing is lost)
    p[0] = (uint32_t)a;
    p[1] = (uint32_t)(a >> 32);
    p[2] = (uint32_t)b;
    p[3] = (uint32_t)(b >> 32);
    return spx::kFinite;
}

// The host's accumulators of one (band, frame): one per moment, the counters shared (tests; the device keeps its own in LDS).
struct Accumulator {
    uint64_t slot[kMaxOrder + 1][kCells] = {};
    uint64_t nans = 0, infs = 0;
    // the value `bits` of the row r = y - y0 < kMaxRows
    void add(uint64_t bits, uint64_t r, int order)
    {
        for (int k = 0; k <= order; k++) {
            int cell;
            uint32_t p[4];
            const int kind = decompose_weighted(bits, weight(r, k), cell, p);
            if (kind != spx::kFinite) {
                if (k == 0) (kind == spx::kNan ? nans : infs)++;
                continue;
            }
            for (int j = 0; j < 4; j++) slot[k][cell + j] += p[j];
        }
    }
    uint64_t finish(int k) const
    {
        spx::Finisher f;
        for (int c = 0; c < kCells; c++) f.push(slot[k][c]);
        return spx::apply_specials(f.result(), nans, infs);
    }
};

// out[k] = RN(exact sum of r^k * value r), k <= order, of `count` <= kMaxRows doubles given as bit patterns, with the NaN and inf rule.
// false, and nothing written: an order outside 0 .. 2, more than kMaxRows values, or a pattern with the sign bit set that is no NaN.
inline bool moment_sum_bits(const uint64_t *bits, size_t count, int order, uint64_t *out)
{
    if (order < 0 || order > kMaxOrder || count > kMaxRows) return false;
    Accumulator acc;
    for (size_t r = 0; r < count; r++) {
        const bool nan = (bits[r] & 0x7fffffffffffffffull) > spx::kInfBits;
        if ((bits[r] >> 63) && !nan) return false;
    }
    for (size_t r = 0; r < count; r++) acc.add(bits[r], r, order);
    for (int k = 0; k <= order; k++) out[k] = acc.finish(k);
    return true;
}

}  // namespace spm
