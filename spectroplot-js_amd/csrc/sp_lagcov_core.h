// sp_lagcov_core.h — the exact lagged covariance sums of two series of non-negative doubles (include/spectroplot_hip.h,
// sp_plan_execute_lagcov).  With N terms, a[x] of the first series and b[x + l] of the second one at lag l
//     out[0] = RN(P),  P = sum a[x] * b[x + l]        out[1] = RN(N * P - A * B),  A = sum a[x],  B = sum b[x + l]        out[2] = RN(B)
// each the EXACT real number rounded once, and out[1] SIGNED.  sp_variance_core.h's arithmetic with two changes: the product of two
// DIFFERENT doubles, and a difference that may be negative.  sp_variance_core.h itself is used as it stands (its slots, its mul_hi and
// its Rounder).  Plain C++, no HIP: the host compiler takes it alone (sp_debug_lagcov, tests/cpp/lagcov_core_check.cpp), and under
// hipcc the same functions are the device's (sp_kernel_lagcov.h).
//
// THE PRODUCTS.  The operands are ma << ea1 and mb << eb1 in units of 2^-1074 (spx::decompose: m < 2^53, e1 <= 2045), so the product
// is ma * mb << (ea1 + eb1) in units of 2^-2148, ma * mb < 2^106.  cell = (ea1 + eb1) >> 5 <= 127 as for a square, but the shift
// s = (ea1 + eb1) & 31 is now anything in 0 .. 31: ma * mb << 31 < 2^137 is still FIVE 32-bit pieces for the cells cell .. cell + 4 <=
// 131, the variance's 132 cells.  A term adds ONE piece below 2^32 to a cell and a request has fewer than 2^31 terms: no cell carries
// out while it accumulates.
//
// THE ROWS.  A (pair, lag) has a row of exactly spv::kSlots = 200 words in the variance's layout - the 66 cells of B, the 132 cells of
// P, a NaN count and an inf count (of the operands of its terms: presence is all the rule asks) - and a pair has one row of 66 cells of
// A, which does not depend on the lag.
//
// THE DIFFERENCE.  N * P < 2^31 * 2^4227 and A * B < 2^2129 * 2^2129 both fit spv::kDigits = 134 digits.  finish_row walks the digits
// from the low one up as the variance's does: P's next digit times N with a carry; the column k of A * B, the sum of dA[i] * dB[k - i]
// over both digit strings' spans, in 128 bits (at most 67 products below 2^64 and a carry: below 2^72); their difference with a borrow.
// Nothing orders N * P and A * B, so a FINAL BORROW OF 1 SAYS THE DIFFERENCE IS NEGATIVE, and its magnitude is the two's complement of
// the digit string: ~d + carry from the low digit up, the carry 1 up to and including the first non-zero digit.  Which of the two it is
// is known only behind the last digit, so two rounders run side by side, one on the digits and one on their complement, and the final
// borrow picks.  The walk ends early where nothing but zero digits can follow; with a borrow pending the digits that would follow are
// all ones, their complement is zero (the first negative step leaves a non-zero digit, so the complement's carry is spent by then), and
// the complement's rounder has seen all it needs.  Rounding to nearest, ties to even, is symmetric: the sign is put on afterwards.
#pragma once

#include "sp_variance_core.h"

namespace spl {

constexpr int kMaxPairs = 16;     // SP_MAX_LAG_PAIRS
constexpr int kMaxLags = 1024;    // SP_MAX_LAGS
constexpr int kSlots = spv::kSlots;           // a (pair, lag)'s words: B's cells at spv::kSumSlot, P's at spv::kSquareSlot, the two counts
constexpr int kPairCells = spx::kCells;       // a pair's words: A's cells
constexpr uint64_t kSignBit = 0x8000000000000000ull;

// the terms of every lag of a request over `width` frames with `lags` lags: the fixed window
SP_XSUM_FN long long terms(long long width, long long lags) { return width - lags + 1 >= 1 ? width - lags + 1 : 0; }

// The pieces of the PRODUCT of two doubles' magnitudes in units of 2^-2148: p[j] goes to cell + j of the P cells.  The kind: a NaN if
// either is one, else an inf if either is one, else finite; only a finite product has pieces.
SP_XSUM_FN int decompose_product(uint64_t bits_a, uint64_t bits_b, int &cell, uint32_t p[5])
{
    const uint32_t ea = (uint32_t)(bits_a >> 52) & 0x7ffu, eb = (uint32_t)(bits_b >> 52) & 0x7ffu;
    const uint64_t fa = bits_a & 0x000fffffffffffffull, fb = bits_b & 0x000fffffffffffffull;
    if (ea == 0x7ffu || eb == 0x7ffu) {
        cell = 0;
        p[0] = p[1] = p[2] = p[3] = p[4] = 0;
        return (ea == 0x7ffu && fa) || (eb == 0x7ffu && fb) ? spx::kNan : spx::kInf;
    }
    const uint64_t ma = ea ? fa | (1ull << 52) : fa, mb = eb ? fb | (1ull << 52) : fb;
    const uint32_t e2 = (ea ? ea - 1 : 0) + (eb ? eb - 1 : 0);             // <= 4090
    const uint32_t s = e2 & 31u;                                           // any of 0 .. 31
    cell = (int)(e2 >> 5);
    const uint64_t lo = ma * mb, hi = spv::mul_hi(ma, mb);                 // hi < 2^42
    const uint64_t a = lo << s;
    const uint64_t b = (hi << s) | (s ? lo >> (64 - s) : 0ull);            // (hi << 31 < 2^73: its top goes to c)
    const uint64_t c = s ? hi >> (64 - s) : 0ull;                          // below 2^9
    p[0] = (uint32_t)a;
    p[1] = (uint32_t)(a >> 32);
    p[2] = (uint32_t)b;
    p[3] = (uint32_t)(b >> 32);
    p[4] = (uint32_t)c;
    return spx::kFinite;
}

// The digits of a sum's 66 cells, carry-normalised into d[spv::kSumDigits]; lo .. hi are its non-zero digits (hi < 0: the sum is zero).
// Returns RN(sum) as bits.
SP_XSUM_FN uint64_t sum_digits(const uint64_t *cells, size_t stride, uint32_t d[spv::kSumDigits], int &lo, int &hi)
{
    spx::Finisher f;
    for (int k = 0; k < spx::kCells; k++) {
        f.push(cells[(size_t)k * stride]);
        d[k] = f.w2;
    }
    d[spx::kCells] = (uint32_t)f.carry;
    lo = spv::kSumDigits, hi = -1;
    for (int k = 0; k < spv::kSumDigits; k++)
        if (d[k]) {
            if (lo > k) lo = k;
            hi = k;
        }
    return f.result();
}

// The three results of one (pair, lag) as bit patterns.  Word k of its row is at row[k * stride] (kSlots of them) and cell k of its
// pair's A at arow[k * astride] (kPairCells of them); `count` = N terms, 0 <= N < 2^31.
SP_XSUM_FN void finish_row(const uint64_t *row, size_t stride, const uint64_t *arow, size_t astride, uint32_t count, uint64_t out[3])
{
    const uint64_t nans = row[(size_t)spv::kNanSlot * stride], infs = row[(size_t)spv::kInfSlot * stride];

    uint32_t da[spv::kSumDigits], db[spv::kSumDigits];
    int loa, hia, lob, hib;
    (void)sum_digits(arow, astride, da, loa, hia);
    out[2] = spx::apply_specials(sum_digits(row + (size_t)spv::kSumSlot * stride, stride, db, lob, hib), nans, infs);

    // P's non-zero cells lo2 .. hi2, and whether A * B is non-zero at all: its columns are loa + lob .. hia + hib (+ 1 of carries)
    int lo2 = spv::kSquareCells, hi2 = -1;
    for (int k = 0; k < spv::kSquareCells; k++)
        if (row[(size_t)(spv::kSquareSlot + k) * stride]) {
            if (lo2 > k) lo2 = k;
            hi2 = k;
        }
    const bool ab = hia >= 0 && hib >= 0;
    if (hi2 < 0 && !ab) {
        out[0] = out[1] = spx::apply_specials(0, nans, infs);
        return;
    }
    if (!ab) loa = lob = hia = hib = 0, da[0] = db[0] = 0;   // (one column of zero)

    // every digit below `first` is zero in P, in N * P and in A * B
    int first = ab ? loa + lob : lo2;
    if (hi2 >= 0 && lo2 < first) first = lo2;
    spv::Rounder rp, rpos, rneg;
    rp.skip(first), rpos.skip(first), rneg.skip(first);
    uint64_t c2 = 0, cw = 0;            // the carries of P's normalisation and of the multiplication by N
    uint64_t acc_lo = 0, acc_hi = 0;    // the column accumulator of A * B, 128 bits
    uint32_t borrow = 0, ncarry = 1;    // ... of the subtraction, and the two's complement's carry
    for (int k = first; k < spv::kDigits; k++) {
        if (k > hi2 && k > hia + hib && !c2 && !cw && !acc_lo && !acc_hi) break;   // nothing but zero digits (or, borrowed, all ones)
        const uint64_t v = (k < spv::kSquareCells ? row[(size_t)(spv::kSquareSlot + k) * stride] : 0ull) + c2;
        const uint32_t d2 = (uint32_t)v;
        c2 = v >> 32;
        rp.digit(d2);
        const uint64_t pw = (uint64_t)d2 * count + cw;   // below 2^32 * 2^31 + 2^31
        const uint32_t a = (uint32_t)pw;
        cw = pw >> 32;
        const int i0 = k - hib > loa ? k - hib : loa, i1 = k - lob < hia ? k - lob : hia;
        for (int i = i0; i <= i1; i++) {
            const uint64_t prod = (uint64_t)da[i] * db[k - i];
            acc_lo += prod;
            acc_hi += acc_lo < prod ? 1u : 0u;
        }
        const uint32_t b = (uint32_t)acc_lo;
        acc_lo = (acc_lo >> 32) | (acc_hi << 32);
        acc_hi >>= 32;
        const uint64_t t = (uint64_t)a - b - borrow;     // (wraps below zero: bit 32 and up are then set)
        borrow = (uint32_t)(t >> 63);
        const uint32_t d = (uint32_t)t;
        rpos.digit(d);
        rneg.digit(~d + ncarry);
        if (d) ncarry = 0;
    }
    out[0] = spx::apply_specials(rp.result(), nans, infs);
    out[1] = spx::apply_specials(borrow ? rneg.result() | kSignBit : rpos.result(), nans, infs);
}

// The host's accumulator of one (pair, lag) (tests and sp_debug_lagcov; the device keeps its rows side by side in a workspace).
struct Accumulator {
    uint64_t slot[kSlots] = {};
    uint64_t aslot[kPairCells] = {};
    uint64_t count = 0;
    // the term a * b
    void add(uint64_t bits_a, uint64_t bits_b)
    {
        int cell;
        uint32_t p3[3], p5[5];
        count++;
        const int ka = spx::decompose(bits_a, cell, p3);
        if (ka == spx::kNan) slot[spv::kNanSlot]++;
        else if (ka == spx::kInf) slot[spv::kInfSlot]++;
        else
            for (int j = 0; j < 3; j++) aslot[cell + j] += p3[j];
        const int kb = spx::decompose(bits_b, cell, p3);
        if (kb == spx::kNan) slot[spv::kNanSlot]++;
        else if (kb == spx::kInf) slot[spv::kInfSlot]++;
        else
            for (int j = 0; j < 3; j++) slot[spv::kSumSlot + cell + j] += p3[j];
        if (decompose_product(bits_a, bits_b, cell, p5) == spx::kFinite)
            for (int j = 0; j < 5; j++) slot[spv::kSquareSlot + cell + j] += p5[j];
    }
    // another accumulator's terms, cell by cell: integer adds, in any order
    void merge(const Accumulator &o)
    {
        for (int k = 0; k < kSlots; k++) slot[k] += o.slot[k];
        for (int k = 0; k < kPairCells; k++) aslot[k] += o.aslot[k];
        count += o.count;
    }
    void finish(uint64_t out[3]) const { finish_row(slot, 1, aslot, 1, (uint32_t)count, out); }
};

// sp_debug_lagcov: out[k * lags + l], k = 0 .. 2, of the series a and b of `width` doubles given as bit patterns, for the lags
// [0, lags).  false, and nothing written: width < 0, lags outside 1 .. kMaxLags, or a pattern with the sign bit set that is no NaN.
inline bool lagcov_bits(const uint64_t *a, const uint64_t *b, long long width, long long lags, uint64_t *out)
{
    if (width < 0 || width >= (1ll << 31) || lags < 1 || lags > kMaxLags) return false;
    for (long long k = 0; k < width; k++)
        for (const uint64_t v : {a[k], b[k]}) {
            const bool nan = (v & 0x7fffffffffffffffull) > spx::kInfBits;
            if ((v >> 63) && !nan) return false;
        }
    const long long n = terms(width, lags);
    for (long long l = 0; l < lags; l++) {
        Accumulator acc;
        for (long long x = 0; x < n; x++) acc.add(a[x], b[x + l]);
        uint64_t r[3];
        acc.finish(r);
        for (int k = 0; k < 3; k++) out[(size_t)k * (size_t)lags + (size_t)l] = r[k];
    }
    return true;
}

}  // namespace spl
