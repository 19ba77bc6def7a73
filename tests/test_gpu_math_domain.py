"""The engine's libm subset over its whole domain against the oracle's: the structured inputs of math_reading.py -- every float
within 2048 ulps of each branch threshold (pi/4, 3 pi/4, pi/2, pi, 0.5, 1, tan(pi/8), tan(3 pi/8)), the subnormals, +-0, +-inf, NaN,
FLT_MAX, a stride through the domains and through all finite floats -- run through MVS_PROBE_MATH and compared with orc_math_batch.
All five columns must have the oracle's bits (or be NaN where the oracle's is) for EVERY input: sin / cos beyond pi/2 and pi,
asin / acos beyond 1 included, which test_gpu_parity.py::test_math_probe_bit_exact masks out.  tests/test_math_reading.py holds the
oracle to a numpy restatement and to float64 on the same inputs."""
import numpy as np
import pytest

import math_reading as mr
import oracle_binding as ob
from mvskit_amd import engine
from parity_support import pair

pytestmark = pytest.mark.gpu

CHUNK = 1 << 21  # values a probe call: the probe stages a patch record per value
COUNTS = (8509689, 8509689, 4272015, 4272015, 4276151)  # structured_inputs(fn).size: an emptied input set must not pass


@pytest.fixture(scope="module")
def plane_engine(small_plane_scene):
    o, e = pair(small_plane_scene, minImageNum=2)
    yield e
    o.close()
    e.close()


@pytest.mark.parametrize("fn", range(5), ids=mr.FNS)
def test_math_probe_equals_the_oracle_on_the_structured_inputs(plane_engine, fn):
    x = mr.structured_inputs(fn)
    assert x.size == COUNTS[fn]
    got = np.concatenate([plane_engine.probe(engine.PROBE_MATH, values=x[i:i + CHUNK]) for i in range(0, x.size, CHUNK)])
    assert got.shape == (COUNTS[fn], 5)
    for col, name in enumerate(mr.FNS):
        want = ob.math_batch(col, x)
        same = mr.same_bits_or_both_nan(got[:, col], want)
        bad = np.flatnonzero(~same)
        assert same.size == COUNTS[fn] and bad.size == 0, (
            f"pm_{name}f: {bad.size} of {x.size} differ; first: x 0x{int(mr.bits_of(x)[bad[0]]):08x} "
            f"engine 0x{int(mr.bits_of(got[:, col])[bad[0]]):08x} oracle 0x{int(mr.bits_of(want)[bad[0]]):08x}")
