// tools/microbench/math_exact.hip -- the arithmetic of mvskit_amd/csrc/mvs_math.cuh over its whole domain, from the header itself
// (included below by relative path: what runs here is what the engine's kernels run).
//   h  the reference of section a checked on the host: (float)sqrt((double)x) == sqrtf(x) for the inputs of section a (no GPU needed)
//   a  sqrt_rn EXHAUSTIVELY: every float from 2^-96 to +inf and +-0 against (float)sqrt((double)x) -- the fp64 root of a float rounded
//      to fp32 is the correctly rounded fp32 root (53 >= 2 * 24 + 2).  Printed, not asserted: where it first differs below 2^-96.
//   b  pm_sincosf against pm_sinf and pm_cosf on all 2^32 bit patterns: equal bits, or both NaN.
//   c  |pm_f(x) - f((double)x)| with the device's fp64 sin, cos, asin, acos, atan: every float with |x| <= MVS_PI (sin, cos), |x| <= 1
//      (asin, acos), every finite float and +-inf (atan).  Each maximum must be <= 1e-6 rad.
//   d  rng_tail(rng_prefix(s, a, b, c, d), e) against rng_uniform(s, a, b, c, d, e) on 2^30 hashed key tuples and the 64 tuples of words
//      0 / 0xffffffff; every value in [-0.5, 0.5); the first 2^20 values against an integer restatement on the host.
// One line per section, PASS / FAIL last, exit status 1 on failure (2: a HIP call failed).  `math_exact c` runs section c alone.
// Every thread keeps its own counts and maxima and merges them once, in LDS; a block writes one record, the host merges the records.
//   hipcc <mvskit_amd.build.FLAGS without -shared -fPIC> -o math_exact math_exact.hip && ./math_exact
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>
#include "../../mvskit_amd/csrc/mvs_math.cuh"

using namespace mvsdev;

#define HIPCHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { \
    fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); exit(2); } } while (0)

constexpr int kThreads = 256, kBlocks = 2048;
constexpr uint32_t kSqrtLo = 0x0F800000u, kInf = 0x7F800000u;      // 2^-96, +inf
constexpr uint64_t kSqrtRange = (uint64_t)(kInf - kSqrtLo) + 1ull;  // section a: this range, then +0 and -0

struct Tally { unsigned long long bad; uint32_t lo, hi; };           // differing inputs: how many, smallest and largest pattern
struct Peak { double err; uint32_t arg; unsigned long long nan; };   // largest error, the smallest pattern that has it, NaN errors

__device__ void merge_tally(unsigned long long bad, uint32_t lo, uint32_t hi, Tally* out) {
    __shared__ unsigned long long s_bad;
    __shared__ uint32_t s_lo, s_hi;
    if (threadIdx.x == 0) { s_bad = 0ull; s_lo = 0xffffffffu; s_hi = 0u; }
    __syncthreads();
    if (bad) { atomicAdd(&s_bad, bad); atomicMin(&s_lo, lo); atomicMax(&s_hi, hi); }
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = {s_bad, s_lo, s_hi};
}

__device__ __forceinline__ bool same(float a, float b) { return __float_as_uint(a) == __float_as_uint(b) || (a != a && b != b); }

// ------------------------------------------------------------------ a: sqrt_rn
// input i < range: pattern first + i; with_zeros: two more inputs, +0 and -0
__global__ __launch_bounds__(kThreads) void k_sqrt(uint32_t first, uint64_t range, int with_zeros, Tally* out) {
    const uint64_t n = range + (with_zeros ? 2ull : 0ull), step = (uint64_t)gridDim.x * blockDim.x;
    unsigned long long bad = 0ull;
    uint32_t lo = 0xffffffffu, hi = 0u;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
        const uint32_t bits = i < range ? first + (uint32_t)i : (i == range ? 0u : 0x80000000u);
        const float x = __uint_as_float(bits);
        const float want = (float)sqrt((double)x), got = sqrt_rn(x);
        if (__float_as_uint(want) != __float_as_uint(got)) { ++bad; lo = min(lo, bits); hi = max(hi, bits); }
    }
    merge_tally(bad, lo, hi, out);
}

// ------------------------------------------------------------------ b: pm_sincosf
__global__ __launch_bounds__(kThreads) void k_sincos(Tally* out) {
    const uint64_t n = 1ull << 32, step = (uint64_t)gridDim.x * blockDim.x;
    unsigned long long bad = 0ull;
    uint32_t lo = 0xffffffffu, hi = 0u;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
        const uint32_t bits = (uint32_t)i;
        const float x = __uint_as_float(bits);
        float s, c;
        pm_sincosf(x, s, c);
        if (!same(s, pm_sinf(x)) || !same(c, pm_cosf(x))) { ++bad; lo = min(lo, bits); hi = max(hi, bits); }
    }
    merge_tally(bad, lo, hi, out);
}

// ------------------------------------------------------------------ c: accuracy against fp64
template <int FN> __device__ __forceinline__ double err_of(float x) {
    const double d = (double)x;
    if (FN == 0) return fabs((double)pm_sinf(x) - sin(d));
    if (FN == 1) return fabs((double)pm_cosf(x) - cos(d));
    if (FN == 2) return fabs((double)pm_asinf(x) - asin(d));
    if (FN == 3) return fabs((double)pm_acosf(x) - acos(d));
    return fabs((double)pm_atanf(x) - atan(d));
}
// inputs: the patterns 0 .. top with the sign bit clear, then the same with it set
template <int FN> __global__ __launch_bounds__(kThreads) void k_accuracy(uint32_t top, Peak* out) {
    __shared__ unsigned long long s_err, s_nan;
    __shared__ uint32_t s_arg;
    if (threadIdx.x == 0) { s_err = 0ull; s_nan = 0ull; s_arg = 0xffffffffu; }
    __syncthreads();
    const uint64_t half = (uint64_t)top + 1ull, n = 2ull * half, step = (uint64_t)gridDim.x * blockDim.x;
    double worst = 0.0;
    uint32_t arg = 0xffffffffu;
    unsigned long long nan = 0ull;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
        const uint32_t bits = i < half ? (uint32_t)i : (0x80000000u | (uint32_t)(i - half));
        const double e = err_of<FN>(__uint_as_float(bits));
        if (e != e) ++nan;
        else if (e > worst || (e == worst && bits < arg)) { worst = e; arg = bits; }
    }
    // a non-negative double orders as its bit pattern does
    const unsigned long long wb = (unsigned long long)__double_as_longlong(worst);
    atomicMax(&s_err, wb);
    if (nan) atomicAdd(&s_nan, nan);
    __syncthreads();
    if (wb == s_err) atomicMin(&s_arg, arg);
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = {__longlong_as_double((long long)s_err), s_arg, s_nan};
}

// ------------------------------------------------------------------ d: RNG
// the inputs of section d (not the code under test): six words from a draw's number
__host__ __device__ inline uint32_t key_mix(uint32_t h) { h ^= h >> 15; h *= 0x2c1b3c6du; h ^= h >> 12; h *= 0x297a2d39u; h ^= h >> 15; return h; }
__host__ __device__ inline void draw_keys(uint64_t i, uint32_t k[6]) {
    if (i >= (1ull << 30)) { for (int j = 0; j < 6; ++j) k[j] = ((i >> j) & 1ull) ? 0xffffffffu : 0u; return; }  // the 64 tuples of 0 / ~0
    uint32_t h = key_mix((uint32_t)i + 0x68e31da4u);
    for (int j = 0; j < 6; ++j) { h = key_mix(h + 0x9e3779b9u * (uint32_t)(j + 1) + (uint32_t)i); k[j] = h; }
}
constexpr uint64_t kRngDraws = (1ull << 30) + 64ull, kRngKept = 1ull << 20;
__global__ __launch_bounds__(kThreads) void k_rng(Tally* differ, Tally* outside, float* kept) {
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    unsigned long long bad = 0ull, out_of_range = 0ull;
    uint32_t lo = 0xffffffffu, hi = 0u, rlo = 0xffffffffu, rhi = 0u;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < kRngDraws; i += step) {
        uint32_t k[6];
        draw_keys(i, k);
        const float whole = rng_uniform(k[0], k[1], k[2], k[3], k[4], k[5]);
        const float parts = rng_tail(rng_prefix(k[0], k[1], k[2], k[3], k[4]), k[5]);
        const uint32_t tag = (uint32_t)i;  // a draw's number (the 64 extra ones wrap to 0 .. 63: the count tells)
        if (__float_as_uint(whole) != __float_as_uint(parts)) { ++bad; lo = min(lo, tag); hi = max(hi, tag); }
        if (!(whole >= -0.5f && whole < 0.5f) || !(parts >= -0.5f && parts < 0.5f)) { ++out_of_range; rlo = min(rlo, tag); rhi = max(rhi, tag); }
        if (i < kRngKept) kept[i] = parts;
    }
    merge_tally(bad, lo, hi, differ);
    __syncthreads();  // merge_tally's shared words are used again
    merge_tally(out_of_range, rlo, rhi, outside);
}
// the hash once more, in plain integer C++ on the host: the value is ((h >> 8) - 2^23) / 2^24, exact in fp32
static uint32_t host_mix(uint32_t h) { h ^= h >> 16; h *= 0x7feb352du; h ^= h >> 15; h *= 0x846ca68bu; h ^= h >> 16; return h; }
static float host_rng(const uint32_t k[6]) {
    static const uint32_t add[4] = {0x85ebca6bu, 0xc2b2ae35u, 0x27d4eb2fu, 0x165667b1u};
    uint32_t h = host_mix(k[0] ^ 0x9e3779b9u);
    for (int j = 0; j < 4; ++j) h = host_mix(h ^ k[j + 1]) + add[j];
    h = host_mix(h ^ k[5]);
    return std::ldexp((float)((int32_t)(h >> 8) - (1 << 23)), -24);
}

// ------------------------------------------------------------------ host
static Tally sum_tallies(const Tally* d_out) {
    std::vector<Tally> h(kBlocks);
    HIPCHK(hipMemcpy(h.data(), d_out, sizeof(Tally) * kBlocks, hipMemcpyDeviceToHost));
    Tally t{0ull, 0xffffffffu, 0u};
    for (const Tally& b : h) { t.bad += b.bad; t.lo = std::min(t.lo, b.lo); t.hi = std::max(t.hi, b.hi); }
    return t;
}
static float as_float(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }
static uint32_t as_bits(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }

static bool host_sqrt_reference() {
    const uint64_t n = kSqrtRange + 2ull;
    const unsigned nt = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    std::vector<unsigned long long> bad(nt, 0ull);
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < nt; ++t)
        pool.emplace_back([&, t] {
            unsigned long long b = 0ull;
            for (uint64_t i = n * t / nt; i < n * (t + 1) / nt; ++i) {
                const float x = as_float(i < kSqrtRange ? kSqrtLo + (uint32_t)i : (i == kSqrtRange ? 0u : 0x80000000u));
                volatile double root = std::sqrt((double)x);  // volatile: a compiler may otherwise narrow (float)sqrt((double)x) to sqrtf(x)
                b += as_bits((float)root) != as_bits(sqrtf(x));
            }
            bad[t] = b;
        });
    for (auto& th : pool) th.join();
    unsigned long long total = 0ull;
    for (unsigned long long b : bad) total += b;
    printf("sqrt reference on the host: %llu inputs, %llu differ between (float)sqrt((double)x) and sqrtf(x)\n", (unsigned long long)n, total);
    return total == 0ull;
}

static void print_below(const char* what, const Tally& t) {
    if (t.bad) printf("sqrt_rn, %s below 2^-96: %llu differ, the largest 0x%08x (%.9g)\n", what, t.bad, t.hi, (double)as_float(t.hi));
    else printf("sqrt_rn, %s below 2^-96: none differs\n", what);
}

template <int FN> static bool accuracy(const char* name, uint32_t top, const char* domain, Peak* d_out) {
    hipLaunchKernelGGL(k_accuracy<FN>, dim3(kBlocks), dim3(kThreads), 0, 0, top, d_out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    std::vector<Peak> h(kBlocks);
    HIPCHK(hipMemcpy(h.data(), d_out, sizeof(Peak) * kBlocks, hipMemcpyDeviceToHost));
    Peak p{0.0, 0xffffffffu, 0ull};
    for (const Peak& b : h) {
        p.nan += b.nan;
        if (b.err > p.err || (b.err == p.err && b.arg < p.arg)) { p.err = b.err; p.arg = b.arg; }
    }
    const bool ok = p.nan == 0ull && p.err <= 1e-6;
    printf("pm_%sf: %llu inputs (%s), max |pm - fp64| %.4e rad at 0x%08x (%.9g), %llu NaN: %s 1e-6\n", name, 2ull * ((unsigned long long)top + 1ull), domain,
           p.err, p.arg, (double)as_float(p.arg), p.nan, ok ? "within" : "ABOVE");
    return ok;
}

int main(int argc, char** argv) {
    const char* sections = argc > 1 ? argv[1] : "habcd";
    bool ok = true;
    if (strchr(sections, 'h')) ok &= host_sqrt_reference();
    if (!strpbrk(sections, "abcd")) { printf(ok ? "PASS\n" : "FAIL\n"); return ok ? 0 : 1; }

    Tally *d_tally, *d_tally2;
    Peak* d_peak;
    float* d_kept;
    HIPCHK(hipMalloc(&d_tally, sizeof(Tally) * kBlocks));
    HIPCHK(hipMalloc(&d_tally2, sizeof(Tally) * kBlocks));
    HIPCHK(hipMalloc(&d_peak, sizeof(Peak) * kBlocks));
    HIPCHK(hipMalloc(&d_kept, sizeof(float) * kRngKept));

    if (strchr(sections, 'a')) {
        hipLaunchKernelGGL(k_sqrt, dim3(kBlocks), dim3(kThreads), 0, 0, kSqrtLo, kSqrtRange, 1, d_tally);
        HIPCHK(hipGetLastError());
        HIPCHK(hipDeviceSynchronize());
        const Tally t = sum_tallies(d_tally);
        printf("sqrt_rn: %llu inputs (every float from 2^-96 to +inf, +0 and -0), %llu differ from (float)sqrt((double)x)", (unsigned long long)(kSqrtRange + 2ull), t.bad);
        if (t.bad) printf("; smallest and largest differing pattern 0x%08x 0x%08x", t.lo, t.hi);
        printf("\n");
        ok &= t.bad == 0ull;
        hipLaunchKernelGGL(k_sqrt, dim3(kBlocks), dim3(kThreads), 0, 0, 0x00800000u, (uint64_t)(kSqrtLo - 0x00800000u), 0, d_tally);
        HIPCHK(hipGetLastError());
        HIPCHK(hipDeviceSynchronize());
        print_below("normal floats", sum_tallies(d_tally));
        hipLaunchKernelGGL(k_sqrt, dim3(kBlocks), dim3(kThreads), 0, 0, 1u, (uint64_t)0x007fffffu, 0, d_tally);
        HIPCHK(hipGetLastError());
        HIPCHK(hipDeviceSynchronize());
        print_below("subnormals", sum_tallies(d_tally));
    }
    if (strchr(sections, 'b')) {
        hipLaunchKernelGGL(k_sincos, dim3(kBlocks), dim3(kThreads), 0, 0, d_tally);
        HIPCHK(hipGetLastError());
        HIPCHK(hipDeviceSynchronize());
        const Tally t = sum_tallies(d_tally);
        printf("pm_sincosf: %llu inputs (every bit pattern), %llu differ from pm_sinf / pm_cosf", 1ull << 32, t.bad);
        if (t.bad) printf("; smallest and largest differing pattern 0x%08x 0x%08x", t.lo, t.hi);
        printf("\n");
        ok &= t.bad == 0ull;
    }
    if (strchr(sections, 'c')) {
        ok &= accuracy<0>("sin", 0x40490FDBu, "|x| <= MVS_PI", d_peak);
        ok &= accuracy<1>("cos", 0x40490FDBu, "|x| <= MVS_PI", d_peak);
        ok &= accuracy<2>("asin", 0x3F800000u, "|x| <= 1", d_peak);
        ok &= accuracy<3>("acos", 0x3F800000u, "|x| <= 1", d_peak);
        ok &= accuracy<4>("atan", kInf, "finite and +-inf", d_peak);
    }
    if (strchr(sections, 'd')) {
        hipLaunchKernelGGL(k_rng, dim3(kBlocks), dim3(kThreads), 0, 0, d_tally, d_tally2, d_kept);
        HIPCHK(hipGetLastError());
        HIPCHK(hipDeviceSynchronize());
        const Tally t = sum_tallies(d_tally), r = sum_tallies(d_tally2);
        std::vector<float> kept(kRngKept);
        HIPCHK(hipMemcpy(kept.data(), d_kept, sizeof(float) * kRngKept, hipMemcpyDeviceToHost));
        unsigned long long host_bad = 0ull;
        for (uint64_t i = 0; i < kRngKept; ++i) {
            uint32_t k[6];
            draw_keys(i, k);
            host_bad += as_bits(host_rng(k)) != as_bits(kept[i]);
        }
        printf("rng: %llu draws, %llu differ between rng_tail(rng_prefix()) and rng_uniform, %llu outside [-0.5, 0.5); "
               "first %llu draws on the host, %llu differ from the integer restatement\n",
               (unsigned long long)kRngDraws, t.bad, r.bad, (unsigned long long)kRngKept, host_bad);
        ok &= t.bad == 0ull && r.bad == 0ull && host_bad == 0ull;
    }
    HIPCHK(hipFree(d_tally)); HIPCHK(hipFree(d_tally2)); HIPCHK(hipFree(d_peak)); HIPCHK(hipFree(d_kept));
    printf(ok ? "PASS\n" : "FAIL\n");
    return ok ? 0 : 1;
}
