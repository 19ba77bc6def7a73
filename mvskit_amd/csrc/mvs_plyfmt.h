// mvs_plyfmt.h -- the text of one PLY vertex line as std::ostream writes it (PatchManager::writePly, patch_manager.cpp:542-633),
// in plain C++ for the device (k_ply_emit, mvs_ply.hip) and the host (tests/test_ply_format.py compiles it with g++).
//
// ostream << float is printf("%g", (double)f): 6 significant digits, round-half-even on the exact binary value, trailing zeros
// dropped, exponent form with at least two exponent digits when the decimal exponent X is < -4 or >= 6.  The digits come from exact
// integer comparisons, never from floating-point arithmetic that could round the wrong way at a tie:
//   x = m 2^e (m < 2^24), compared with B 10^q as  m 2^e  vs  B 5^q 2^q  (q >= 0)  or  m 5^-q 2^(e-q)  vs  B  (q < 0),
// in 128-bit integers.  Every product that is formed is below 2^125 for the comparisons the search makes (|q| <= 50, B < 2^22), and a
// shift that would leave 128 bits decides the comparison by itself.  A double estimate only picks where the search starts.
// Writers take `char* out`; out == nullptr counts the characters only.  No array is indexed at run time: no scratch memory on the GPU.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MVS_PLY_HD __host__ __device__ inline
#else
#define MVS_PLY_HD inline
#endif

#define MVS_PLY_LINE_MAX 96  // longest ASCII vertex line: 6 x "-1.23456e-05" + 3 x "255" + 8 blanks + '\n' = 90

namespace mvsply {

typedef unsigned __int128 u128;

MVS_PLY_HD int bitlen128(u128 v) {
    const uint64_t hi = (uint64_t)(v >> 64), lo = (uint64_t)v;
    if (hi) return 128 - __builtin_clzll(hi);
    return lo ? 64 - __builtin_clzll(lo) : 0;
}
// sign of a 2^s - b (a, b >= 0, any s): a shift past 127 bits makes a 2^s the larger of the two
MVS_PLY_HD int cmp_shifted(u128 a, int s, u128 b) {
    if (s >= 0) {
        if (a == 0) return b == 0 ? 0 : -1;
        if (bitlen128(a) + s > 128) return 1;
        const u128 as = a << s;
        return as < b ? -1 : (as > b ? 1 : 0);
    }
    if (b == 0) return a == 0 ? 0 : 1;
    if (bitlen128(b) - s > 128) return -1;
    const u128 bs = b << (-s);
    return a < bs ? -1 : (a > bs ? 1 : 0);
}
// 5^p for 0 <= p <= 55 (5^55 < 2^128)
MVS_PLY_HD u128 pow5(int p) {
    u128 r = 1;
    for (int i = 0; i < p; ++i) r *= 5u;
    return r;
}
// sign of m 2^e - B 10^q; p5 = 5^|q|.  A product of more than 128 bits is at least 2^127: with B < 2^22 that happens only for q >= 46
// (B 10^q beyond every float) or q <= -45 (x 10^-q above 2^23 > B), so the sign is known without it
MVS_PLY_HD int cmp_dec(uint32_t m, int e, uint64_t B, int q, u128 p5) {
    if (q >= 0) {
        if (bitlen128((u128)B) + bitlen128(p5) > 128) return -1;
        return cmp_shifted((u128)m, e - q, (u128)B * p5);
    }
    if (bitlen128((u128)m) + bitlen128(p5) > 128) return 1;
    return cmp_shifted((u128)m * p5, e - q, (u128)B);
}
// |x| = m 2^e, finite and nonzero -> the 6-digit decimal M (100000 <= M <= 999999) and exponent X of printf's "%.5e" of it
MVS_PLY_HD void round6(uint32_t m, int e, double ax, uint32_t* M, int* X) {
    // 10^E <= x < 10^(E+1); the start floor(log2(x) * 0.30103) is at most one off
    const int l2 = e + bitlen128((u128)m) - 1;
    int E = (l2 * 78913) >> 18;
    for (;;) {
        if (cmp_dec(m, e, 1, E, pow5(E < 0 ? -E : E)) < 0) { --E; continue; }
        if (cmp_dec(m, e, 1, E + 1, pow5(E + 1 < 0 ? -(E + 1) : E + 1)) >= 0) { ++E; continue; }
        break;
    }
    // F = floor(x / 10^q) in [10^5, 10^6), q = E - 5
    const int q = E - 5;
    const u128 p5 = pow5(q < 0 ? -q : q);
    double est = ax;
    for (int i = 0; i < (q < 0 ? -q : q); ++i) est = q < 0 ? est * 10.0 : est / 10.0;
    int64_t F = (int64_t)est;
    if (F < 100000) F = 100000;
    if (F > 999999) F = 999999;
    while (F > 100000 && cmp_dec(m, e, (uint64_t)F, q, p5) < 0) --F;
    while (F < 999999 && cmp_dec(m, e, (uint64_t)(F + 1), q, p5) >= 0) ++F;
    // x against (F + 1/2) 10^q, i.e. 2x against (2F + 1) 10^q; ties to even
    const int c = cmp_dec(m, e + 1, (uint64_t)(2 * F + 1), q, p5);
    if (c > 0 || (c == 0 && (F & 1))) ++F;
    if (F == 1000000) { F = 100000; ++E; }
    *M = (uint32_t)F;
    *X = E;
}

MVS_PLY_HD int put(char* out, int n, char c) {
    if (out) out[n] = c;
    return n + 1;
}
// the decimal digits of v (v >= 0), most significant first
MVS_PLY_HD int put_uint(char* out, int n, uint32_t v) {
    uint32_t p = 1;
    while (v / p >= 10u) p *= 10u;
    for (; p > 0; p /= 10u) n = put(out, n, (char)('0' + (v / p) % 10u));
    return n;
}

// printf("%g", (double)f) into out[0..); returns the number of characters (at most 12)
MVS_PLY_HD int format_g(float f, char* out) {
    union { float f; uint32_t u; } cv;
    cv.f = f;
    const uint32_t bits = cv.u;
    const uint32_t bexp = (bits >> 23) & 0xffu, frac = bits & 0x7fffffu;
    int n = 0;
    if (bits >> 31) n = put(out, n, '-');
    if (bexp == 0xffu) {
        if (frac) { n = put(out, n, 'n'); n = put(out, n, 'a'); return put(out, n, 'n'); }
        n = put(out, n, 'i'); n = put(out, n, 'n'); return put(out, n, 'f');
    }
    if (bexp == 0 && frac == 0) return put(out, n, '0');
    const uint32_t m = bexp ? (frac | 0x800000u) : frac;
    const int e = bexp ? (int)bexp - 150 : -149;
    union { uint64_t u; double d; } p2;
    p2.u = (uint64_t)(e + 1023) << 52;  // 2^e as a double (e >= -149)
    const double ax = (double)m * p2.d;
    uint32_t M = 0;
    int X = 0;
    round6(m, e, ax, &M, &X);
    int nd = 6;  // significant digits left after the trailing zeros go
    while (nd > 1 && M % 10u == 0) { M /= 10u; --nd; }
    // digit i (0 = most significant) of the nd-digit M: M / 10^(nd-1-i) % 10
    uint32_t p = 1;
    for (int i = 1; i < nd; ++i) p *= 10u;
    if (X < -4 || X >= 6) {  // d[.ddddd]e+XX
        n = put(out, n, (char)('0' + M / p));
        if (nd > 1) n = put(out, n, '.');
        for (uint32_t pp = p / 10u; pp > 0; pp /= 10u) n = put(out, n, (char)('0' + (M / pp) % 10u));
        n = put(out, n, 'e');
        n = put(out, n, X < 0 ? '-' : '+');
        const int ax10 = X < 0 ? -X : X;
        n = put(out, n, (char)('0' + ax10 / 10));
        return put(out, n, (char)('0' + ax10 % 10));
    }
    if (X < 0) {  // 0.000ddd
        n = put(out, n, '0');
        n = put(out, n, '.');
        for (int i = -1; i > X; --i) n = put(out, n, '0');
        for (uint32_t pp = p; pp > 0; pp /= 10u) n = put(out, n, (char)('0' + (M / pp) % 10u));
        return n;
    }
    // X + 1 integer digits, then the fraction digits that are left
    int i = 0;
    for (uint32_t pp = p; pp > 0; pp /= 10u, ++i) {
        if (i == X + 1) n = put(out, n, '.');
        n = put(out, n, (char)('0' + (M / pp) % 10u));
    }
    for (; i < X + 1; ++i) n = put(out, n, '0');
    return n;
}

// one vertex line "x y z nx ny nz r g b\n" (ostream's output for floats and ints); returns its length (at most 90).  The values are
// picked by a chain of selects, not from an array: nothing is indexed at run time
MVS_PLY_HD int format_line(float x, float y, float z, float nx, float ny, float nz, uint32_t r, uint32_t g, uint32_t b, char* out) {
    int n = 0;
    for (int k = 0; k < 6; ++k) {
        const float v = k == 0 ? x : k == 1 ? y : k == 2 ? z : k == 3 ? nx : k == 4 ? ny : nz;
        n += format_g(v, out ? out + n : out);
        n = put(out, n, ' ');
    }
    for (int k = 0; k < 3; ++k) {
        n = put_uint(out, n, k == 0 ? r : k == 1 ? g : b);
        n = put(out, n, k < 2 ? ' ' : '\n');
    }
    return n;
}

}  // namespace mvsply
