"""The oracle's libm subset (pm_sinf .. pm_atanf through orc_math_batch) and counter RNG (orc_rng_batch) against a second reading in
numpy (math_reading.py) on structured inputs: every float within 2048 ulps of each branch threshold, the subnormals, +-0, +-inf, NaN,
arguments beyond the domains, and a stride through the domains -- a few million values a function.  Bit for bit against the float32
restatement, within 1e-6 rad of float64 inside the domains (a thousandth of the project's 1e-3 rad contract).  The RNG: bit for bit
against the uint32 restatement on fifteen streams of 2^20 draws, and on each the 256-bin chi-square, the lag-1 correlation and the
range.  The inputs are fixed, so every figure is deterministic; the caps are conditions, met by the restatement alone.  No GPU:
tests/test_gpu_math_domain.py holds the engine to the same oracle on the same inputs."""
import functools

import numpy as np
import pytest

import math_reading as mr
import oracle_binding as ob


@functools.lru_cache(maxsize=None)
def _inputs_and_oracle(fn):
    x = mr.structured_inputs(fn)
    out = ob.math_batch(fn, x)
    x.setflags(write=False)
    out.setflags(write=False)
    return x, out


def test_constants_are_the_headers():
    """the decimal constants of the reading round to the floats the C sources' literals are"""
    want = {"PIO2_HI": 0x3FC90FDA, "PIO2_LO": 0x33A22168, "PIO4": 0x3F490FDB, "PI": 0x40490FDB, "THREE_PIO4": 0x4016CBE4,
            "ATAN_LO": 0x3ED413CD, "ATAN_HI": 0x401A827A}
    for name, bits in want.items():
        assert mr.pattern(getattr(mr, name)) == bits, name


@pytest.mark.parametrize("fn", range(5), ids=mr.FNS)
def test_structured_inputs_hold_the_edges(fn):
    x, _ = _inputs_and_oracle(fn)
    b = mr.bits_of(x)
    assert 4_000_000 < x.size < 10_000_000
    assert (b[1:] > b[:-1]).all()  # sorted by pattern, each once

    def holds(patterns):
        patterns = np.asarray(patterns, dtype=np.uint32)
        at = np.minimum(np.searchsorted(b, patterns), b.size - 1)
        return (b[at] == patterns).all()

    for centre in (mr.PIO4, mr.THREE_PIO4, mr.PIO2_HI, mr.PI, mr.F(0.5), mr.F(1), mr.ATAN_LO, mr.ATAN_HI):
        c = mr.pattern(centre)
        for sign in (0, 0x80000000):
            assert holds(np.arange(c - 2048, c + 2049, dtype=np.uint32) | np.uint32(sign)), (centre, sign)
    for pattern in (0, 0x80000000, 1, 4096, 0x80000001, 0x007FFFFF, 0x00800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000):
        assert holds([pattern]), hex(pattern)
    beyond = int((~mr.in_domain(fn, x)).sum())
    assert beyond >= (2_000_000 if fn in (0, 1) else 1 if fn == 4 else 20_000), beyond  # atan: the NaN alone


@pytest.mark.parametrize("fn", range(5), ids=mr.FNS)
def test_oracle_equals_the_float32_reading_bit_for_bit(fn):
    x, got = _inputs_and_oracle(fn)
    want = mr.reading(fn, x)
    same = mr.same_bits_or_both_nan(got, want)
    bad = np.flatnonzero(~same)
    assert bad.size == 0, (f"{bad.size} of {x.size} differ; first: x 0x{int(mr.bits_of(x)[bad[0]]):08x} "
                           f"oracle 0x{int(mr.bits_of(got)[bad[0]]):08x} reading 0x{int(mr.bits_of(want)[bad[0]]):08x}")


@pytest.mark.parametrize("fn", range(5), ids=mr.FNS)
def test_oracle_within_1e6_of_float64_inside_the_domain(fn):
    x, got = _inputs_and_oracle(fn)
    dom = mr.in_domain(fn, x)
    assert dom.sum() > 4_000_000
    assert not np.isnan(got[dom]).any()
    err = np.abs(got[dom].astype(np.float64) - mr.float64_reference(fn, x[dom]))
    worst = int(np.argmax(err))
    print(f"pm_{mr.FNS[fn]}f: {int(dom.sum())} inputs, max |pm - float64| {err[worst]:.4e} at 0x{int(mr.bits_of(x[dom])[worst]):08x}")
    assert err[worst] <= 1e-6


def test_asin_clamps_and_acos_is_nan_beyond_one():
    """pm_asinf clamps |x| > 1 to 1 (infinities included): the value at +-1, bit for bit.  pm_acosf has no clamp: beyond 1 the root of
    a negative number makes it NaN, which is why its callers clamp the cosine first (decode / encode)."""
    x, asin = _inputs_and_oracle(2)
    at_one = ob.math_batch(2, np.array([1.0, -1.0], np.float32))
    assert mr.bits_of(at_one).tolist() == [0x3FC90FDB, 0xBFC90FDB]  # +-float(pi / 2)
    above, below = x > 1, x < -1
    assert above.sum() > 10_000 and below.sum() > 10_000
    assert (mr.bits_of(asin[above]) == 0x3FC90FDB).all() and (mr.bits_of(asin[below]) == 0xBFC90FDB).all()
    x, acos = _inputs_and_oracle(3)
    outside = np.abs(x) > 1
    assert outside.sum() > 20_000 and np.isnan(acos[outside]).all()
    assert np.isnan(asin[np.isnan(x)]).all() and np.isnan(acos[np.isnan(x)]).all()


@pytest.mark.parametrize("seed", mr.RNG_SEEDS, ids=lambda s: f"seed{s:x}")
@pytest.mark.parametrize("word", range(5), ids=list("abcde"))
def test_rng_stream(seed, word):
    """2^20 draws along one key word: the oracle's bits equal the uint32 restatement's; every value in [-0.5, 0.5); the 256-bin
    chi-square (255 degrees of freedom: mean 255, sd 22.6) below 400 = 6.4 sd; |corr(u(k), u(k + 1))| below 0.005 = 5 / sqrt(2^20)."""
    keys = mr.rng_stream_keys(word)
    u = ob.rng_batch(seed, keys)
    assert u.size == mr.RNG_DRAWS
    np.testing.assert_array_equal(mr.bits_of(u), mr.bits_of(mr.reading_rng(seed, keys)))
    assert u.min() >= -0.5 and u.max() < 0.5
    counts = np.bincount(np.floor((u.astype(np.float64) + 0.5) * 256).astype(np.int64), minlength=256)
    assert counts.size == 256
    expect = mr.RNG_DRAWS / 256
    chi2 = float(((counts - expect) ** 2 / expect).sum())
    corr = float(np.corrcoef(u[:-1].astype(np.float64), u[1:].astype(np.float64))[0, 1])
    print(f"seed {seed:#x} word {word}: chi-square {chi2:.1f}, lag-1 correlation {corr:+.5f}")
    assert chi2 < 400
    assert abs(corr) < 0.005
