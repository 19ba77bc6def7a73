"""A second reading of the engine arithmetic's libm subset and counter RNG (oracle/pmmvs_oracle.cpp pm_* / rng_uniform,
mvskit_amd/csrc/mvs_math.cuh): the five pm_* functions in numpy float32, the same constants and operation order, every operation a
float32 numpy operation, np.sqrt for the root; the hash in numpy uint32; the float64 references; and the structured inputs both are
run on -- every float around each branch threshold, the subnormals, zeros, infinities, a NaN, and a stride through the domain.
Shares no code with the oracle.  numpy only, no GPU (a helper module like second_reading.py)."""
import numpy as np

F = np.float32
U = np.uint32

FNS = ("sin", "cos", "asin", "acos", "atan")  # the order of orc_math_batch's fn and of MVS_PROBE_MATH's columns

PIO2_HI = F(1.57079625129699707031)
PIO2_LO = F(7.54978941586159635335e-08)
PIO4 = F(0.78539816339744830962)
PI = F(3.14159265358979323846)
THREE_PIO4 = F(3.0) * PIO4            # the float product the branches compare with
ATAN_LO = F(0.4142135623730950)
ATAN_HI = F(2.414213562373095)
FLT_MAX_BITS = 0x7F7FFFFF
INF_BITS = 0x7F800000
QNAN_BITS = 0x7FC00000
PI_BITS = 0x40490FDB
ONE_BITS = 0x3F800000


def bits_of(x):
    return np.ascontiguousarray(x, dtype=F).view(U)


def pattern(v):
    """the bit pattern of one float32, as an int"""
    return int(F(v).view(U))


def floats_of(bits):
    return np.ascontiguousarray(bits, dtype=U).view(F)


# ------------------------------------------------------------------ the structured inputs
def _both_signs(mag_bits):
    mag_bits = np.asarray(mag_bits, dtype=np.int64)
    return np.concatenate([mag_bits, mag_bits | 0x80000000])


def _around(centre, ulps=2048):
    """the patterns of every non-negative float within `ulps` ulps of centre, up to +inf"""
    c = pattern(centre)
    return np.arange(max(c - ulps, 0), min(c + ulps, INF_BITS) + 1, dtype=np.int64)


def _stride(top_bits, step):
    return np.arange(0, top_bits + 1, step, dtype=np.int64)


def structured_inputs(fn):
    """The inputs of function fn (0..4 = FNS), float32, sorted by bit pattern, each pattern once:
    every float within 2048 ulps of 0, MVS_PIO4, 3.0f * MVS_PIO4, pi/2, MVS_PI, 0.5, 1, the two thresholds of pm_atanf, 2^-126 and
    FLT_MAX, both signs; the 4096 smallest subnormals, +-0, +-inf, a quiet NaN; 1 + k ulps for k <= 2048 (the a > 1 clamp of
    pm_asinf); every 509th float of the function's domain, and every 1021st of all finite floats for atan and for sin / cos."""
    centres = [F(0), PIO4, THREE_PIO4, PIO2_HI, PI, F(0.5), F(1), ATAN_LO, ATAN_HI, F(2.0) ** F(-126), U(FLT_MAX_BITS).view(F)]
    parts = [_both_signs(_around(c)) for c in centres]
    parts.append(_both_signs(np.arange(1, 4097)))                              # the smallest subnormals
    parts.append(_both_signs([0, INF_BITS]))
    parts.append(np.array([QNAN_BITS], dtype=np.int64))
    parts.append(_both_signs(ONE_BITS + np.arange(0, 2049)))
    if fn in (0, 1):
        parts += [_both_signs(_stride(PI_BITS, 509)), _both_signs(_stride(FLT_MAX_BITS, 1021))]
    elif fn in (2, 3):
        parts.append(_both_signs(_stride(ONE_BITS, 509)))
    elif fn == 4:
        parts.append(_both_signs(_stride(FLT_MAX_BITS, 1021)))
    else:
        raise ValueError(fn)
    return floats_of(np.unique(np.concatenate(parts)).astype(U))


def in_domain(fn, x):
    """where the function is specified: |x| <= MVS_PI (sin, cos), |x| <= 1 (asin, acos), everything but NaN (atan)"""
    x = np.asarray(x, dtype=F)
    if fn in (0, 1):
        return np.abs(x) <= PI
    if fn in (2, 3):
        return np.abs(x) <= F(1)
    return ~np.isnan(x)


# ------------------------------------------------------------------ the five functions in float32
def _k_sin(x):
    z = x * x
    p = F(-1.9515295891e-4) * z + F(8.3321608736e-3)
    p = p * z - F(1.6666654611e-1)
    return x + x * z * p


def _k_cos(x):
    z = x * x
    p = F(2.443315711809948e-5) * z - F(1.388731625493765e-3)
    p = p * z + F(4.166664568298827e-2)
    return (F(1.0) - F(0.5) * z) + z * z * p


def _signed(x, r):
    return np.where(x < F(0.0), -r, r)


def reading_sin(x):
    a = np.abs(x)
    r = np.where(a <= PIO4, _k_sin(a), np.where(a <= THREE_PIO4, _k_cos((PIO2_HI - a) + PIO2_LO), _k_sin(PI - a)))
    return _signed(x, r)


def reading_cos(x):
    a = np.abs(x)
    return np.where(a <= PIO4, _k_cos(a), np.where(a <= THREE_PIO4, _k_sin((PIO2_HI - a) + PIO2_LO), -_k_cos(PI - a)))


def reading_asin(x):
    a = np.abs(x)
    a = np.where(a > F(1.0), F(1.0), a)
    flag = a > F(0.5)
    half = F(0.5) * (F(1.0) - a)
    z = np.where(flag, half, a * a)
    xx = np.where(flag, np.sqrt(half), a)
    p = F(4.2163199048e-2) * z + F(2.4181311049e-2)
    p = p * z + F(4.5470025998e-2)
    p = p * z + F(7.4953002686e-2)
    p = p * z + F(1.6666752422e-1)
    r = p * z * xx + xx
    r2 = r + r
    r = np.where(flag, (PIO2_HI - r2) + PIO2_LO, r)
    return _signed(x, r)


def reading_acos(x):
    low = PI - F(2.0) * reading_asin(np.sqrt(F(0.5) * (F(1.0) + x)))
    high = F(2.0) * reading_asin(np.sqrt(F(0.5) * (F(1.0) - x)))
    return np.where(x < F(-0.5), low, np.where(x > F(0.5), high, PIO2_HI - reading_asin(x)))


def reading_atan(v):
    x = np.abs(v)
    big = x > ATAN_HI
    mid = ~big & (x > ATAN_LO)
    y = np.where(big, PIO2_HI, np.where(mid, PIO4, F(0.0)))
    x = np.where(big, -(F(1.0) / x), np.where(mid, (x - F(1.0)) / (x + F(1.0)), x))
    z = x * x
    p = F(8.05374449538e-2) * z - F(1.38776856032e-1)
    p = p * z + F(1.99777106478e-1)
    p = p * z - F(3.33329491539e-1)
    y = y + (p * z * x + x)
    return _signed(v, y)


_READINGS = (reading_sin, reading_cos, reading_asin, reading_acos, reading_atan)
_FLOAT64 = (np.sin, np.cos, np.arcsin, np.arccos, np.arctan)


def reading(fn, x):
    """pm_<FNS[fn]>f of every float32 of x, in float32 numpy operations"""
    x = np.ascontiguousarray(x, dtype=F)
    with np.errstate(all="ignore"):
        out = _READINGS[fn](x)
    assert out.dtype == F
    return out


def float64_reference(fn, x):
    with np.errstate(all="ignore"):
        return _FLOAT64[fn](np.asarray(x, dtype=F).astype(np.float64))


def same_bits_or_both_nan(a, b):
    """per element: equal bit patterns, or a NaN on both sides"""
    a, b = np.asarray(a, dtype=F), np.asarray(b, dtype=F)
    return (bits_of(a) == bits_of(b)) | (np.isnan(a) & np.isnan(b))


# ------------------------------------------------------------------ the counter RNG in uint32
def _mix32(h):
    h = h ^ (h >> U(16))
    h = h * U(0x7feb352d)
    h = h ^ (h >> U(15))
    h = h * U(0x846ca68b)
    return h ^ (h >> U(16))


def reading_rng(seed, keys):
    """rng_uniform(seed, a, b, c, d, e) for every row (a, b, c, d, e) of keys [n, 5]: the hash in uint32 arithmetic (mod 2^32), the
    value (h >> 8) / 2^24 - 0.5 in float32, where it is exact"""
    k = np.ascontiguousarray(keys, dtype=U)
    with np.errstate(over="ignore"):
        h = _mix32(np.full(k.shape[0], U(int(seed) & 0xffffffff) ^ U(0x9e3779b9), dtype=U))
        for j, add in enumerate((0x85ebca6b, 0xc2b2ae35, 0x27d4eb2f, 0x165667b1)):
            h = _mix32(h ^ k[:, j]) + U(add)
        h = _mix32(h ^ k[:, 4])
    return (h >> U(8)).astype(F) * F(1.0 / 16777216.0) - F(0.5)


RNG_FIXED = (3, 1, 2, 5, 4)          # the key words that stay put while one of them runs
RNG_SEEDS = (0, 7, 0xffffffff)
RNG_DRAWS = 1 << 20


def rng_stream_keys(word, n=RNG_DRAWS):
    """keys [n, 5]: word `word` (0..4 = a..e) runs 0 .. n - 1, the others stay at RNG_FIXED"""
    k = np.empty((n, 5), dtype=U)
    k[:] = np.asarray(RNG_FIXED, dtype=U)
    k[:, word] = np.arange(n, dtype=U)
    return k
