// coflux_exact_sum.hpp — the exact sum of doubles behind cf_normalize_salinity_flux_exact (include/coflux.h): the format of an
// accumulator, how a term enters it and how it is rounded to a double.  Plain C++: it builds without HIP (tests/
// exact_sum_driver.cpp includes it and nothing else) and is included by the device code (coflux_exact_sum.hip).
//
// An accumulator is XS_DIGITS = 67 signed 64-bit digits; digit k has weight 2^(32k − 1088).  A finite double is ±m·2^e with m a
// 53-bit integer and e ≥ −1074; m shifted to the digit boundary below it, m << ((e + 1088) mod 32), has at most 84 bits: three
// adjacent digits take one 32-bit piece each, with the term's sign.  A digit therefore absorbs 2³¹ terms before it can
// overflow, the top digit (weight 2¹⁰²⁴) has 32 bits of headroom, and — integer adds being associative — the digits of a sum
// do not depend on the order, the grouping or the number of partial accumulators the terms went through.  Three counters
// beside the digits count the terms that are no number: NaN, +Inf, −Inf.  The accumulator is rounded to a double once.
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define XS_FN __host__ __device__ inline
#else
#define XS_FN inline
#endif

namespace coflux {

constexpr int XS_DIGITS = 67;
constexpr int XS_BIAS = 1088;                 // digit k weighs 2^(32k − XS_BIAS)
constexpr int XS_COUNTERS = 3;                // NaN, +Inf, −Inf terms
constexpr int XS_WORDS = XS_DIGITS + XS_COUNTERS;   // one accumulator as 64-bit words: the digits, then the counters
enum { XS_NAN = 0, XS_PINF = 1, XS_NINF = 2 };

struct XsAccumulator {
    int64_t digit[XS_DIGITS];
    uint64_t nonfinite[XS_COUNTERS];
};
static_assert(sizeof(XsAccumulator) == XS_WORDS * 8, "an accumulator is XS_WORDS 64-bit words");

// A term as it enters an accumulator: digit[first + n] += piece[n] (n = 0, 1, 2) where first ≥ 0, or nonfinite[−1 − first] += 1.
// A zero of either sign has three zero pieces.
struct XsTerm {
    int first;
    int64_t piece[3];
};

XS_FN uint64_t xs_bits(double x) {
    uint64_t u;
    memcpy(&u, &x, sizeof u);
    return u;
}
XS_FN double xs_double(uint64_t u) {
    double x;
    memcpy(&x, &u, sizeof x);
    return x;
}

XS_FN XsTerm xs_split(double x) {
    const uint64_t u = xs_bits(x);
    const int field = (int)((u >> 52) & 0x7ffu);
    const uint64_t fraction = u & 0x000fffffffffffffull;
    const bool negative = (u >> 63) != 0;
    XsTerm t;
    if (field == 0x7ff) {
        t.first = -1 - (fraction ? XS_NAN : negative ? XS_NINF : XS_PINF);
        t.piece[0] = t.piece[1] = t.piece[2] = 0;
        return t;
    }
    const uint64_t m = field ? fraction | (1ull << 52) : fraction;   // x = ±m · 2^e
    const int e = (field ? field : 1) - 1075;
    const int at = e + XS_BIAS;                                      // ≥ 14: bit `at` of the accumulator is m's bit 0
    const int shift = at & 31;
    const uint64_t low = m << shift, high = shift > 11 ? m >> (64 - shift) : 0;   // (m has 53 bits: nothing leaves `low` up to 11)
    t.first = at >> 5;
    t.piece[0] = (int64_t)(low & 0xffffffffull);
    t.piece[1] = (int64_t)(low >> 32);
    t.piece[2] = (int64_t)high;
    if (negative) {
        t.piece[0] = -t.piece[0];
        t.piece[1] = -t.piece[1];
        t.piece[2] = -t.piece[2];
    }
    return t;
}

XS_FN void xs_clear(XsAccumulator* A) {
    for (int k = 0; k < XS_DIGITS; ++k) A->digit[k] = 0;
    for (int k = 0; k < XS_COUNTERS; ++k) A->nonfinite[k] = 0;
}

XS_FN void xs_add(XsAccumulator* A, double x) {
    const XsTerm t = xs_split(x);
    if (t.first < 0) {
        A->nonfinite[-1 - t.first] += 1;
        return;
    }
    // (the largest double starts at digit 64 and its third piece is zero: first + 2 ≤ 66)
    for (int n = 0; n < 3; ++n) A->digit[t.first + n] += t.piece[n];
}

// A += B, digit-wise: what joins partial accumulators (workgroups, ranks)
XS_FN void xs_merge(XsAccumulator* A, const XsAccumulator* B) {
    for (int k = 0; k < XS_DIGITS; ++k) A->digit[k] += B->digit[k];
    for (int k = 0; k < XS_COUNTERS; ++k) A->nonfinite[k] += B->nonfinite[k];
}

// digits 0 … 65 into [0, 2³²), the carries upwards; the top digit keeps the sign of the whole
XS_FN void xs_carry(int64_t* digit) {
    int64_t carry = 0;   // (kept in a register: the loads of the digits do not wait for one another)
    for (int k = 0; k + 1 < XS_DIGITS; ++k) {
        const int64_t v = digit[k] + carry;
        carry = v >> 32;   // floor: the remainder is non-negative
        digit[k] = v - carry * 4294967296ll;
    }
    digit[XS_DIGITS - 1] += carry;
}

XS_FN int xs_bit(const int64_t* digit, int b) { return (int)((digit[b >> 5] >> (b & 31)) & 1); }

// The accumulator as a double, rounded once to nearest-even (at 2⁻¹⁰⁷⁴ where the result is subnormal): ±Inf beyond the largest
// double, +0.0 for a zero sum; NaN with a NaN term or both infinities among the terms, the infinity with one of them.
// `digit` is scratch of the caller: XS_DIGITS words that hold the digits on entry and garbage on return.
XS_FN double xs_round_digits(int64_t* digit, const uint64_t* nonfinite) {
    if (nonfinite[XS_NAN] || (nonfinite[XS_PINF] && nonfinite[XS_NINF])) return xs_double(0x7ff8000000000000ull);
    if (nonfinite[XS_PINF]) return xs_double(0x7ff0000000000000ull);
    if (nonfinite[XS_NINF]) return xs_double(0xfff0000000000000ull);
    xs_carry(digit);
    const bool negative = digit[XS_DIGITS - 1] < 0;
    if (negative) {   // the magnitude: every digit negated (none is INT64_MIN after the carries), carried again
        for (int k = 0; k < XS_DIGITS; ++k) digit[k] = -digit[k];
        xs_carry(digit);
    }
    const uint64_t sign = negative ? 0x8000000000000000ull : 0;
    if (digit[XS_DIGITS - 1] != 0) return xs_double(sign | 0x7ff0000000000000ull);   // ≥ 2¹⁰²⁴
    int top = -1;   // the highest set bit among digits 0 … 65
    for (int k = XS_DIGITS - 2; k >= 0 && top < 0; --k)
        if (digit[k])
            for (int b = 31; b >= 0; --b)
                if ((digit[k] >> b) & 1) {
                    top = 32 * k + b;
                    break;
                }
    if (top < 0) return 0.0;
    // every term is a multiple of 2⁻¹⁰⁷⁴ = bit 14: nothing is set below it, a subnormal result is exact
    int low = top - 52 > 14 ? top - 52 : 14;   // the bit the mantissa's bit 0 is
    // bits low … top, 53 at the most, lie in three adjacent digits (low ≤ 2059: the third is digit 66 at the most, and zero there)
    const int k0 = low >> 5, shift = low & 31;
    uint64_t m = (uint64_t)digit[k0] >> shift | (uint64_t)digit[k0 + 1] << (32 - shift);
    if (shift > 11) m |= (uint64_t)digit[k0 + 2] << (64 - shift);
    m &= (2ull << (top - low)) - 1;
    if (low > 14 && xs_bit(digit, low - 1)) {
        const int below = low - 2;   // ≥ 13: anything set in bits 0 … below breaks the tie
        bool sticky = (digit[below >> 5] & ((int64_t)((2ull << (below & 31)) - 1))) != 0;
        for (int k = (below >> 5) - 1; k >= 0 && !sticky; --k) sticky = digit[k] != 0;
        if (sticky || (m & 1)) ++m;
        if (m >> 53) {
            m >>= 1;
            ++low;
        }
    }
    if (!(m >> 52)) return xs_double(sign | m);           // subnormal (low = 14)
    const int field = low - 13;                           // m · 2^(low − 1088) = 1.f · 2^(field − 1023)
    if (field >= 0x7ff) return xs_double(sign | 0x7ff0000000000000ull);
    return xs_double(sign | ((uint64_t)field << 52) | (m & 0x000fffffffffffffull));
}

XS_FN double xs_round(const XsAccumulator* A) {
    int64_t digit[XS_DIGITS];
    for (int k = 0; k < XS_DIGITS; ++k) digit[k] = A->digit[k];
    return xs_round_digits(digit, A->nonfinite);
}

}  // namespace coflux
