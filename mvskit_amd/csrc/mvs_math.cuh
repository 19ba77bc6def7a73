// mvs_math.cuh -- the arithmetic every device unit may use, none of it about a patch: the F3 / F4 vectors with their fmaf-chain dot
// products, the correctly rounded square root, reciprocal and quotient, the deterministic libm subset (pm_*) and the counter-based RNG.
// Arithmetic rules: mvs_device.cuh and DESIGN.md, "engine arithmetic".
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mvsdev {

struct F3 { float x, y, z; };
struct F4 { float x, y, z, w; };

#define DEV __device__ __forceinline__

DEV float fma_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
DEV float dot4(F4 a, F4 b) { return fma_(a.w, b.w, fma_(a.z, b.z, fma_(a.y, b.y, a.x * b.x))); }
DEV float dot3(F3 a, F3 b) { return fma_(a.z, b.z, fma_(a.y, b.y, a.x * b.x)); }
// Correctly rounded square root (== the oracle's sqrtf) for +-0, +inf and every argument from 2^-96 up: v_sqrt_f32 is within one
// ulp, and the residuals of its two neighbours (one fma each) decide which of the three is the rounded root.  This is
// the compiler's own IEEE expansion without the rescaling of arguments below 2^-96, which this path never produces
// (squared lengths and texture variances), and at half its instruction count.  tools/microbench/math_exact.hip runs it against
// (float)sqrt((double)x) for EVERY float from 2^-96 to +inf (1.88 * 10^9 inputs: no difference).  Measured below that: right down
// to 2^-104; the largest float at which it differs is 0x0b6e9372 = 4.5948e-32 (3.95 * 10^6 normal floats differ, and every
// subnormal).
DEV float sqrt_rn(float x) {
    float s = __builtin_amdgcn_sqrtf(x);
    const float dn = __int_as_float(__float_as_int(s) - 1), up = __int_as_float(__float_as_int(s) + 1);
    const float rd = __builtin_fmaf(-dn, s, x), ru = __builtin_fmaf(-up, s, x);
    s = rd <= 0.0f ? dn : s;
    s = ru > 0.0f ? up : s;
    return s;
}
// Correctly rounded reciprocal and quotient in 3 and 6 instructions where the compiler's IEEE expansion takes 11 (v_div_scale x 2,
// v_rcp, four fma, v_div_fmas, v_div_fixup): v_rcp_f32 is within one ulp, one Newton step in fma lands on RN(1 / x); the quotient is
// Markstein's q' = RN(q + (a - b q) y) with y = RN(1 / b).  tools/microbench/div_exact.hip runs rcp_rn against `1.0f / x` for EVERY
// float with 2^-120 <= |x| < 2^121 (4.04 * 10^9 inputs: no difference) and div_rn against `a / b` on 1.18 * 10^10 pairs (none) --
// profiles/r04_div_exact.txt.  Outside that range (zero, subnormal, infinite or NaN divisors, quotients that over- or underflow) they
// differ from IEEE division; they are used only where the divisor is a length, a depth, a focal scale or 1 + 3 incc of this path.
DEV float rcp_rn(float x) {
    const float r = __builtin_amdgcn_rcpf(x);
    return __builtin_fmaf(__builtin_fmaf(-x, r, 1.0f), r, r);
}
DEV float div_rn(float a, float b) {
    const float y = rcp_rn(b), q = a * y;
    return __builtin_fmaf(__builtin_fmaf(-b, q, a), y, q);
}
DEV float norm4(F4 a) { return sqrt_rn(dot4(a, a)); }
DEV float norm3(F3 a) { return sqrt_rn(dot3(a, a)); }
DEV F4 sub4(F4 a, F4 b) { return {a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w}; }
DEV F4 add4(F4 a, F4 b) { return {a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w}; }
DEV F3 sub3(F3 a, F3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
// v / |v| as v * (1/|v|) (Eigen 3.2 vector / scalar semantics; one IEEE division instead of three or four)
DEV F4 nrm4(F4 a) { const float inv = rcp_rn(norm4(a)); return {a.x * inv, a.y * inv, a.z * inv, a.w * inv}; }
DEV F3 nrm3(F3 a) { const float inv = rcp_rn(norm3(a)); return {a.x * inv, a.y * inv, a.z * inv}; }
DEV F4 scl4(F4 a, float s) { return {a.x * s, a.y * s, a.z * s, a.w * s}; }
DEV F3 scl3(F3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
DEV F3 cross3(F3 a, F3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
DEV F4 ld4(const float* p) { return {p[0], p[1], p[2], p[3]}; }
DEV F3 ld3(const float* p) { return {p[0], p[1], p[2]}; }


// ------------------------------------------------------------------ deterministic libm subset
// (same kernels, constants and evaluation order as the oracle's pm_* functions)
// Largest |pm_f(x) - f(x)| against fp64 over EVERY float of the domain (tools/microbench/math_exact.hip, section c), in rad:
//   pm_sinf  1.0636e-07 at 0x40274eb8, pm_cosf 1.3457e-07 at 0x40170bc5   (|x| <= MVS_PI)
//   pm_asinf 1.6525e-07 at 0x3f5db809, pm_acosf 3.0491e-07 at 0xbf003df1   (|x| <= 1)
//   pm_atanf 1.7068e-07 at 0x403f4d05                                      (every finite float, +-inf)
// Beyond the domains: pm_asinf clamps |x| > 1 to 1; pm_acosf is NaN there (its callers clamp); pm_sinf / pm_cosf are not reduced
// beyond pi.  pm_sincosf returns the bits of pm_sinf and pm_cosf for all 2^32 arguments (section b).
#define MVS_PIO2_HI 1.57079625129699707031f
#define MVS_PIO2_LO 7.54978941586159635335e-08f
#define MVS_PIO4 0.78539816339744830962f
#define MVS_PI 3.14159265358979323846f
DEV float k_sinf(float x) {
    float z = x * x;
    float p = -1.9515295891e-4f * z + 8.3321608736e-3f;
    p = p * z - 1.6666654611e-1f;
    return x + x * z * p;
}
DEV float k_cosf(float x) {
    float z = x * x;
    float p = 2.443315711809948e-5f * z - 1.388731625493765e-3f;
    p = p * z + 4.166664568298827e-2f;
    return (1.0f - 0.5f * z) + z * z * p;
}
DEV float pm_sinf(float x) {
    float a = fabsf(x), r;
    if (a <= MVS_PIO4) r = k_sinf(a);
    else if (a <= 3.0f * MVS_PIO4) r = k_cosf((MVS_PIO2_HI - a) + MVS_PIO2_LO);
    else r = k_sinf(MVS_PI - a);
    return x < 0.0f ? -r : r;
}
DEV float pm_cosf(float x) {
    float a = fabsf(x);
    if (a <= MVS_PIO4) return k_cosf(a);
    if (a <= 3.0f * MVS_PIO4) return k_sinf((MVS_PIO2_HI - a) + MVS_PIO2_LO);
    return -k_cosf(MVS_PI - a);
}
// sin and cos of one angle: the same three ranges, kernels and reduced arguments as pm_sinf / pm_cosf, evaluated once
// and selected (lanes of one wave usually fall in different ranges, so the branches of the two calls would all run)
DEV void pm_sincosf(float x, float& s, float& c) {
    const float a = fabsf(x);
    const bool r0 = a <= MVS_PIO4, r1 = a <= 3.0f * MVS_PIO4;
    const float t = r0 ? a : (r1 ? (MVS_PIO2_HI - a) + MVS_PIO2_LO : MVS_PI - a);
    const float ks = k_sinf(t), kc = k_cosf(t);
    const float sr = (r0 || !r1) ? ks : kc;
    s = x < 0.0f ? -sr : sr;
    c = r0 ? kc : (r1 ? ks : -kc);
}
DEV float pm_asinf(float x) {
    float a = fabsf(x);
    if (a > 1.0f) a = 1.0f;
    float z, xx;
    bool flag = a > 0.5f;
    if (flag) { z = 0.5f * (1.0f - a); xx = sqrt_rn(z); }
    else { z = a * a; xx = a; }
    float p = 4.2163199048e-2f * z + 2.4181311049e-2f;
    p = p * z + 4.5470025998e-2f;
    p = p * z + 7.4953002686e-2f;
    p = p * z + 1.6666752422e-1f;
    float r = p * z * xx + xx;
    if (flag) { r = r + r; r = (MVS_PIO2_HI - r) + MVS_PIO2_LO; }
    return x < 0.0f ? -r : r;
}
DEV float pm_acosf(float x) {
    if (x < -0.5f) return MVS_PI - 2.0f * pm_asinf(sqrt_rn(0.5f * (1.0f + x)));
    if (x > 0.5f) return 2.0f * pm_asinf(sqrt_rn(0.5f * (1.0f - x)));
    return MVS_PIO2_HI - pm_asinf(x);
}
DEV float pm_atanf(float v) {
    float x = fabsf(v), y;
    if (x > 2.414213562373095f) { y = MVS_PIO2_HI; x = -(1.0f / x); }
    else if (x > 0.4142135623730950f) { y = MVS_PIO4; x = (x - 1.0f) / (x + 1.0f); }
    else y = 0.0f;
    float z = x * x;
    float p = 8.05374449538e-2f * z - 1.38776856032e-1f;
    p = p * z + 1.99777106478e-1f;
    p = p * z - 3.33329491539e-1f;
    y = y + (p * z * x + x);
    return v < 0.0f ? -y : y;
}

// ------------------------------------------------------------------ counter-based RNG
DEV uint32_t mix32(uint32_t h) {
    h ^= h >> 16; h *= 0x7feb352du; h ^= h >> 15; h *= 0x846ca68bu; h ^= h >> 16;
    return h;
}
DEV float rng_uniform(uint32_t seed, uint32_t a, uint32_t b, uint32_t c, uint32_t d, uint32_t e) {
    uint32_t h = mix32(seed ^ 0x9e3779b9u);
    h = mix32(h ^ a) + 0x85ebca6bu;
    h = mix32(h ^ b) + 0xc2b2ae35u;
    h = mix32(h ^ c) + 0x27d4eb2fu;
    h = mix32(h ^ d) + 0x165667b1u;
    h = mix32(h ^ e);
    return (float)(h >> 8) * (1.0f / 16777216.0f) - 0.5f;
}

// rng_uniform in two parts, rng_tail(seed-to-d prefix, e): where two keys d share a wave, the prefix of each is taken once
DEV uint32_t rng_prefix(uint32_t seed, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    uint32_t h = mix32(seed ^ 0x9e3779b9u);
    h = mix32(h ^ a) + 0x85ebca6bu;
    h = mix32(h ^ b) + 0xc2b2ae35u;
    h = mix32(h ^ c) + 0x27d4eb2fu;
    return mix32(h ^ d) + 0x165667b1u;
}
DEV float rng_tail(uint32_t h, uint32_t e) {
    h = mix32(h ^ e);
    return (float)(h >> 8) * (1.0f / 16777216.0f) - 0.5f;
}

}  // namespace mvsdev
