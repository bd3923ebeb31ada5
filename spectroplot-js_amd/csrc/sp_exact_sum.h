// sp_exact_sum.h — the exact sum of non-negative doubles: integer arithmetic only, so the result does not depend on the order of the
// addends.  Plain C++, no HIP: the host compiler takes it alone (sp_debug_exact_sum, tests/cpp/exact_sum_check.cpp), and under hipcc
// the same functions are the device's (sp_kernel_mean.h).
//
// A non-negative finite double is a 53-bit integer m times a power of two.  A row's accumulator is kCells unsigned 64-bit cells, cell
// k weighing 2^(32 k) * 2^-1074 (bit 0 of cell 0 is the smallest denormal).  With e the exponent field (e = 0 read as e = 1 without the
// hidden bit) the value is m << (e - 1) in units of 2^-1074: m << ((e - 1) % 32), at most 84 bits, is cut into three 32-bit pieces for
// the cells (e - 1) / 32, + 1 and + 2.  A value adds ONE piece below 2^32 to a cell, so a cell holds any 2^31 values without a carry
// out, and integer adds commute.  finish() propagates the carries from the low cell up and rounds ONCE, to nearest, ties to even:
// the correctly rounded sum (Python: math.fsum).  Two counters beside the cells hold how many NaNs and how many +inf came.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define SP_XSUM_FN __host__ __device__ inline
#else
#define SP_XSUM_FN inline
#endif

namespace spx {

constexpr int kCells = 66;            // e - 1 <= 2045: cells 63, 64, 65 take DBL_MAX
constexpr int kNanSlot = kCells;      // the count of NaN addends
constexpr int kInfSlot = kCells + 1;  // the count of +inf addends
constexpr int kSlots = kCells + 2;    // 64-bit words per row

enum Kind { kFinite = 0, kNan = 1, kInf = 2 };

constexpr uint64_t kInfBits = 0x7ff0000000000000ull, kNanBits = 0x7ff8000000000000ull;

// The pieces of a double's magnitude (the sign bit is ignored: the callers' addends are never negative): p[j] goes to cell + j.
SP_XSUM_FN int decompose(uint64_t bits, int &cell, uint32_t p[3])
{
    const uint32_t e = (uint32_t)(bits >> 52) & 0x7ffu;
    const uint64_t frac = bits & 0x000fffffffffffffull;
    if (e == 0x7ffu) {
        cell = 0;
        p[0] = p[1] = p[2] = 0;
        return frac ? kNan : kInf;
    }
    const uint64_t m = e ? frac | (1ull << 52) : frac;
    const uint32_t e1 = e ? e - 1 : 0;
    const uint32_t s = e1 & 31u;
    cell = (int)(e1 >> 5);
    const uint64_t lo = m << s;
    p[0] = (uint32_t)lo;
    p[1] = (uint32_t)(lo >> 32);
    p[2] = s > 11 ? (uint32_t)(m >> (64 - s)) : 0u;   // (m < 2^53: nothing passes bit 63 while s <= 11)
    return kFinite;
}

// The digits of a sum from the low cell up: push() takes cell k's raw 64-bit word in order of k, keeps the carry and remembers the
// three digits that end at the highest non-zero one together with whether anything below them is set - all that rounding needs.
struct Finisher {
    uint64_t carry = 0;
    uint32_t w0 = 0, w1 = 0, w2 = 0;   // the last three digits pushed (w2 the latest)
    uint32_t below = 0;                // the OR of every digit before them
    uint32_t t0 = 0, t1 = 0, t2 = 0, tbelow = 0;
    int top = -1, count = 0;

    SP_XSUM_FN void digit(uint32_t d)
    {
        below |= w0;
        w0 = w1, w1 = w2, w2 = d;
        if (d) top = count, t0 = w0, t1 = w1, t2 = w2, tbelow = below;
        count++;
    }
    SP_XSUM_FN void push(uint64_t cell_word)
    {
        const uint64_t v = cell_word + carry;   // (a cell stays below 2^63 within a request and the carry below 2^32)
        digit((uint32_t)v);
        carry = v >> 32;
    }
    // RN(sum) as the bits of a double, once every cell has been pushed
    SP_XSUM_FN uint64_t result()
    {
        digit((uint32_t)carry);   // (the carry out of the last cell: such a sum is far beyond DBL_MAX)
        carry = 0;
        if (top < 0) return 0;    // +0.0
        if (top <= 1) {
            // below 2^64 units: up to 2^53 the integer IS the pattern (denormals, and 2^52 is exponent field 1), exactly
            const uint64_t N = top ? ((uint64_t)t2 << 32) | t1 : (uint64_t)t2;
            if (N < (1ull << 53)) return N;
        }
        int lz = 0;
        for (uint32_t v = t2; !(v & 0x80000000u); v <<= 1) lz++;
        const int T = 32 * top + 31 - lz;      // the sum's highest bit, in units of 2^-1074; T >= 53 here
        const int e = T - 51;                  // its exponent field
        if (e > 0x7fe) return kInfBits;
        const uint64_t hi = ((uint64_t)t2 << 32) | t1;
        const uint64_t A = lz ? (hi << lz) | (uint64_t)(t0 >> (32 - lz)) : hi;   // the window's top 64 bits, bit 63 set
        const uint32_t L = lz ? t0 << lz : t0;                                   // ... and what is left of it
        const uint64_t mant = A >> 11;                                           // 53 bits, the hidden one on top
        const bool half = (A & 0x400u) != 0;
        const bool sticky = (A & 0x3ffu) != 0 || L != 0 || tbelow != 0;
        const uint64_t up = half && (sticky || (mant & 1u)) ? 1u : 0u;
        // (the hidden bit adds 1 to the field, and so does a mantissa that rounds up to 2^53; from field 0x7fe that is +inf's pattern)
        return ((uint64_t)(e - 1) << 52) + mant + up;
    }
};

// What a row's counters make of the rounded sum: any NaN addend gives NaN, otherwise any +inf addend gives +inf.
SP_XSUM_FN uint64_t apply_specials(uint64_t sum_bits, uint64_t nans, uint64_t infs)
{
    return nans ? kNanBits : infs ? kInfBits : sum_bits;
}

// The host's accumulator of one row (tests; the device keeps its rows side by side in a workspace).
struct Accumulator {
    uint64_t slot[kSlots] = {};
    void add(uint64_t bits)
    {
        int cell;
        uint32_t p[3];
        const int kind = decompose(bits, cell, p);
        if (kind == kNan) slot[kNanSlot]++;
        else if (kind == kInf) slot[kInfSlot]++;
        else {
            slot[cell] += p[0];
            slot[cell + 1] += p[1];
            slot[cell + 2] += p[2];
        }
    }
    uint64_t finish() const
    {
        Finisher f;
        for (int k = 0; k < kCells; k++) f.push(slot[k]);
        return apply_specials(f.result(), slot[kNanSlot], slot[kInfSlot]);
    }
};

// RN(exact sum) of `count` doubles given as bit patterns, with the NaN and inf rule.  false, and nothing written: a pattern with the
// sign bit set that is no NaN (a negative value, -0.0 or -inf) - the accumulator has no subtraction.
inline bool exact_sum_bits(const uint64_t *bits, size_t count, uint64_t *sum_bits)
{
    Accumulator acc;
    for (size_t k = 0; k < count; k++) {
        const bool nan = (bits[k] & 0x7fffffffffffffffull) > kInfBits;
        if ((bits[k] >> 63) && !nan) return false;
        acc.add(bits[k]);
    }
    *sum_bits = acc.finish();
    return true;
}

}  // namespace spx
