// sp_variance_core.h — the exact second-order sums of a row of non-negative doubles over the frames of a request: the variance and
// spectral-kurtosis traces (include/spectroplot_hip.h, sp_plan_execute_variance).  With W values p of a row
//     out[0] = RN(S1),  S1 = sum p        out[1] = RN(S2),  S2 = sum p^2        out[2] = RN(W * S2 - S1^2)
// each the EXACT real number rounded once.  sp_exact_sum.h's arithmetic, applied to the product of two doubles, with the subtraction
// done in integers as well: W * S2 - S1^2 is W^2 times the population variance, and for a steady row it lies tens of orders of magnitude
// below either term - in floating point it is noise; here it is one integer.  Plain C++, no HIP: the host compiler takes it alone
// (sp_debug_variance_sums, tests/cpp/variance_core_check.cpp), and under hipcc the same functions are the device's
// (sp_kernel_variance.h).
//
// THE SQUARES.  A value is m << e1 in units of 2^-1074 (spx::decompose: m < 2^53, e1 = e - 1 <= 2045, e = 0 read as e = 1 without the
// hidden bit), so its square is m^2 << 2 e1 in units of 2^-2148, m^2 < 2^106.  The S2 accumulator's cell k weighs 2^(32 k) * 2^-2148:
// cell = (2 e1) >> 5 <= 127, the shift s = (2 e1) & 31 is even and at most 30, and m^2 << s < 2^136 is cut into FIVE 32-bit pieces for
// the cells cell .. cell + 4 <= 131.  kSquareCells = 132 = 128 + 4: cells 0 .. 127 are where a square can begin and 128 .. 131 are what
// DBL_MAX^2 reaches beyond them.  There is no cell for carries: a value adds ONE piece below 2^32 to a cell and a request has at most
// 2^31 frames, so a 64-bit cell stays below 2^63 and never carries out while it accumulates - the mean's argument - and the carry out
// of cell 131 when the cells are normalised (S2 < 2^31 * 2^4196 = 2^4227 > 2^(32 * 132)) is digit 132 of the digit string, which the
// finish makes on the fly.  S1 has spx::kCells = 66 cells and the digits 0 .. 66 (S1 < 2^31 * 2^2098 = 2^2129).
//
// THE DIFFERENCE.  W * S2 < 2^31 * 2^4227 and S1^2 < 2^4258 both fit kDigits = 134 32-bit digits (4288 bits) in units of 2^-2148.
// finish_row walks the digits from the low one up: S2's next digit (cell + carry), times W with a 64-bit carry; the column k of S1^2,
// the sum of d1[i] * d1[k - i], in a 128-bit accumulator (at most 67 products below 2^64 and the carry of the column before: below 2^72);
// their difference with a borrow; and that digit goes into the rounder.  W * S2 >= S1^2 by Cauchy-Schwarz, so the last borrow is zero.
//
// THE COST.  Only the digits between a row's lowest and highest non-zero one are visited.  If a row's finite non-zero values lie between
// 2^a and 2^b, S1 has at most s1 = (b - a) / 32 + 4 non-zero digits (three pieces of the smallest value, the cells between, one of
// carries), the walk takes at most 2 * s1 + 2 digit steps and s1 products per step: with all of a request's values within 2^64 of each
// other (192 dB) that is s1 <= 6, 14 steps and at most 84 multiplications.  The worst case - a row with denormals and DBL_MAX - is 134
// steps and 67^2 = 4489 multiplications.
#pragma once

#include "sp_exact_sum.h"

namespace spv {

constexpr int kSquareCells = 132;                  // the cells of S2: 2 e1 <= 4090, cells 127 .. 131 take DBL_MAX^2
constexpr int kSumDigits = spx::kCells + 1;        // the digits of S1: its 66 cells and the carry out of the last
constexpr int kDigits = 134;                       // the digits of W * S2, of S1^2 and of their difference
constexpr int kSumSlot = 0;                        // a row's 64-bit words: the cells of S1 ...
constexpr int kSquareSlot = spx::kCells;           // ... the cells of S2 ...
constexpr int kNanSlot = kSquareSlot + kSquareCells;   // ... and the counts of NaN and of +inf addends
constexpr int kInfSlot = kNanSlot + 1;
constexpr int kSlots = kInfSlot + 1;               // 200

// the high 64 bits of a * b
SP_XSUM_FN uint64_t mul_hi(uint64_t a, uint64_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// The pieces of the SQUARE of a double's magnitude in units of 2^-2148: p[j] goes to cell + j of the S2 cells.  The kind is
// spx::decompose's; a NaN or an inf has no pieces.
SP_XSUM_FN int decompose_squared(uint64_t bits, int &cell, uint32_t p[5])
{
    const uint32_t e = (uint32_t)(bits >> 52) & 0x7ffu;
    const uint64_t frac = bits & 0x000fffffffffffffull;
    if (e == 0x7ffu) {
        cell = 0;
        p[0] = p[1] = p[2] = p[3] = p[4] = 0;
        return frac ? spx::kNan : spx::kInf;
    }
    const uint64_t m = e ? frac | (1ull << 52) : frac;
    const uint32_t e2 = 2u * (e ? e - 1 : 0);
    const uint32_t s = e2 & 31u;                                           // even, <= 30
    cell = (int)(e2 >> 5);
    const uint64_t lo = m * m, hi = mul_hi(m, m);                          // hi < 2^42
    const uint64_t a = lo << s;
    const uint64_t b = (hi << s) | (s ? lo >> (64 - s) : 0ull);            // (hi << 30 < 2^72: its top goes to c)
    const uint64_t c = s ? hi >> (64 - s) : 0ull;                          // below 2^8
    p[0] = (uint32_t)a;
    p[1] = (uint32_t)(a >> 32);
    p[2] = (uint32_t)b;
    p[3] = (uint32_t)(b >> 32);
    p[4] = (uint32_t)c;
    return spx::kFinite;
}

// RN of a digit string in units of 2^-2148, the digits pushed from the low one up (skip() stands for a run of zero digits).  Where
// spx::Finisher's units are 2^-1074 and every integer below 2^53 IS the pattern, here the low 1074 bits lie below the denormal grid:
// with T the highest set bit the result's last place is bit q = max(T - 52, 1074), the mantissa is the string >> q, and what lies
// below q rounds it, to nearest, ties to even.  T >= 1126 is a normal number with the exponent field T - 1125, and the rounder keeps
// what spx::Finisher keeps - the three digits that end at the highest non-zero one and whether anything below them is set.  T < 1126
// is a denormal (or rounds up to the smallest normal): q = 1074 is bit 18 of digit 33 and the mantissa ends in digit 35, so the
// rounder also keeps the digits 33 .. 35 and whether anything below digit 33 is set.
struct Rounder {
    uint32_t w0 = 0, w1 = 0, w2 = 0, below = 0;   // the last three digits pushed (w2 the latest) and the OR of every digit before them
    uint32_t t0 = 0, t1 = 0, t2 = 0, tbelow = 0;  // ... as they stood at the highest non-zero digit
    uint32_t f0 = 0, f1 = 0, f2 = 0, fbelow = 0;  // the digits 33, 34, 35 and the OR of the digits below 33
    int top = -1, count = 0;

    SP_XSUM_FN void skip(int digits)
    {
        // (only in front of the first non-zero digit: everything kept so far is zero)
        count += digits;
    }
    SP_XSUM_FN void digit(uint32_t d)
    {
        below |= w0;
        w0 = w1, w1 = w2, w2 = d;
        if (d) top = count, t0 = w0, t1 = w1, t2 = w2, tbelow = below;
        if (count < 33) fbelow |= d;
        else if (count == 33) f0 = d;
        else if (count == 34) f1 = d;
        else if (count == 35) f2 = d;
        count++;
    }
    SP_XSUM_FN uint64_t result() const
    {
        if (top < 0) return 0;   // +0.0
        int lz = 0;
        for (uint32_t v = t2; !(v & 0x80000000u); v <<= 1) lz++;
        const int T = 32 * top + 31 - lz;      // the highest set bit, in units of 2^-2148
        if (T < 1126) {
            // bits 1074 .. 1125 are the pattern; bit 1073 is the half and everything below it is sticky
            const uint64_t mant = ((uint64_t)f2 << 46) | ((uint64_t)f1 << 14) | (uint64_t)(f0 >> 18);   // (f2 < 2^6 here)
            const bool half = (f0 & 0x20000u) != 0;
            const bool sticky = (f0 & 0x1ffffu) != 0 || fbelow != 0;
            return mant + (half && (sticky || (mant & 1u)) ? 1u : 0u);
        }
        const int e = T - 1125;                // the exponent field
        if (e > 0x7fe) return spx::kInfBits;
        const uint64_t hi = ((uint64_t)t2 << 32) | t1;
        const uint64_t A = lz ? (hi << lz) | (uint64_t)(t0 >> (32 - lz)) : hi;   // the window's top 64 bits, bit 63 set (T >= 64: top >= 2)
        const uint32_t L = lz ? t0 << lz : t0;
        const uint64_t mant = A >> 11;
        const bool half = (A & 0x400u) != 0;
        const bool sticky = (A & 0x3ffu) != 0 || L != 0 || tbelow != 0;
        const uint64_t up = half && (sticky || (mant & 1u)) ? 1u : 0u;
        // (the hidden bit adds 1 to the field, and so does a mantissa that rounds up to 2^53; from field 0x7fe that is +inf's pattern)
        return ((uint64_t)(e - 1) << 52) + mant + up;
    }
};

// The three results of one row as bit patterns from its words: word k of the row is at row[k * stride] (kSlots of them: the host's
// accumulator has stride 1, the device's workspace is slot-major with stride n), W = `width` frames, 0 <= W < 2^31.
SP_XSUM_FN void finish_row(const uint64_t *row, size_t stride, uint32_t width, uint64_t out[3])
{
    const uint64_t nans = row[(size_t)kNanSlot * stride], infs = row[(size_t)kInfSlot * stride];

    // S1: carry-normalised into d1, rounded by the mean's finisher; lo1 .. hi1 are its non-zero digits
    uint32_t d1[kSumDigits];
    int lo1 = kSumDigits, hi1 = -1;
    {
        spx::Finisher f;
        for (int k = 0; k < spx::kCells; k++) {
            f.push(row[(size_t)(kSumSlot + k) * stride]);
            d1[k] = f.w2;
        }
        d1[spx::kCells] = (uint32_t)f.carry;
        for (int k = 0; k < kSumDigits; k++)
            if (d1[k]) {
                if (lo1 > k) lo1 = k;
                hi1 = k;
            }
        out[0] = spx::apply_specials(f.result(), nans, infs);
    }

    // S2's non-zero cells lo2 .. hi2
    int lo2 = kSquareCells, hi2 = -1;
    for (int k = 0; k < kSquareCells; k++)
        if (row[(size_t)(kSquareSlot + k) * stride]) {
            if (lo2 > k) lo2 = k;
            hi2 = k;
        }
    if (hi2 < 0) {   // no finite non-zero value: both are zero, and so is S1
        out[1] = out[2] = spx::apply_specials(0, nans, infs);
        return;
    }

    // Every digit below `first` is zero in S2, in W * S2 and in S1^2 (whose lowest column is 2 lo1; a non-zero value has non-zero
    // pieces in both accumulators, so hi1 >= 0 here).
    const int first = lo2 < 2 * lo1 ? lo2 : 2 * lo1;
    Rounder r2, r3;
    r2.skip(first), r3.skip(first);
    uint64_t c2 = 0, cw = 0;            // the carries of S2's normalisation and of the multiplication by W
    uint64_t acc_lo = 0, acc_hi = 0;    // the column accumulator of S1^2, 128 bits
    uint32_t borrow = 0;
    for (int k = first; k < kDigits; k++) {
        if (k > hi2 && k > 2 * hi1 && !c2 && !cw && !acc_lo && !acc_hi) break;   // nothing but zero digits from here on
        const uint64_t v = (k < kSquareCells ? row[(size_t)(kSquareSlot + k) * stride] : 0ull) + c2;
        const uint32_t d2 = (uint32_t)v;
        c2 = v >> 32;
        r2.digit(d2);
        const uint64_t pw = (uint64_t)d2 * width + cw;   // below 2^32 * 2^31 + 2^31
        const uint32_t a = (uint32_t)pw;
        cw = pw >> 32;
        const int i0 = k - hi1 > lo1 ? k - hi1 : lo1, i1 = k - lo1 < hi1 ? k - lo1 : hi1;
        for (int i = i0; i <= i1; i++) {
            const uint64_t prod = (uint64_t)d1[i] * d1[k - i];
            acc_lo += prod;
            acc_hi += acc_lo < prod ? 1u : 0u;
        }
        const uint32_t b = (uint32_t)acc_lo;
        acc_lo = (acc_lo >> 32) | (acc_hi << 32);
        acc_hi >>= 32;
        const uint64_t t = (uint64_t)a - b - borrow;     // (wraps below zero: bit 32 and up are then set)
        borrow = (uint32_t)(t >> 63);
        r3.digit((uint32_t)t);
    }
    out[1] = spx::apply_specials(r2.result(), nans, infs);
    out[2] = spx::apply_specials(r3.result(), nans, infs);
}

// The host's accumulator of one row (tests; the device keeps its rows side by side in a workspace).
struct Accumulator {
    uint64_t slot[kSlots] = {};
    uint64_t count = 0;
    void add(uint64_t bits)
    {
        int cell;
        uint32_t p3[3], p5[5];
        count++;
        const int kind = spx::decompose(bits, cell, p3);
        if (kind == spx::kNan) slot[kNanSlot]++;
        else if (kind == spx::kInf) slot[kInfSlot]++;
        else {
            for (int j = 0; j < 3; j++) slot[kSumSlot + cell + j] += p3[j];
            decompose_squared(bits, cell, p5);
            for (int j = 0; j < 5; j++) slot[kSquareSlot + cell + j] += p5[j];
        }
    }
    // another accumulator's addends, cell by cell: integer adds, in any order
    void merge(const Accumulator &o)
    {
        for (int k = 0; k < kSlots; k++) slot[k] += o.slot[k];
        count += o.count;
    }
    void finish(uint64_t out[3]) const { finish_row(slot, 1, (uint32_t)count, out); }
};

// out[0 .. 2] = RN(S1), RN(S2), RN(count * S2 - S1^2) of `count` < 2^31 doubles given as bit patterns, with the NaN and inf rule.
// false, and nothing written: 2^31 values or more, or a pattern with the sign bit set that is no NaN (a negative value, -0.0 or -inf).
inline bool variance_sums_bits(const uint64_t *bits, size_t count, uint64_t out[3])
{
    if (count >= ((size_t)1 << 31)) return false;
    for (size_t k = 0; k < count; k++) {
        const bool nan = (bits[k] & 0x7fffffffffffffffull) > spx::kInfBits;
        if ((bits[k] >> 63) && !nan) return false;
    }
    Accumulator acc;
    for (size_t k = 0; k < count; k++) acc.add(bits[k]);
    acc.finish(out);
    return true;
}

}  // namespace spv
