"""rcp_rn / div_rn of mvs_math.cuh -- v_rcp_f32 + one Newton step in fma; Markstein's quotient correction on top -- stand in for
IEEE-754 division in the hot geometry (projection, ray normalisation, units, 1 / msd, robust INCC, isNeighbor): 3 and 6 instructions
where the compiler's expansion takes 11.  They must return the very bits `1.0f / x` and `a / b` return, or the engine would leave
the oracle's arithmetic.  tools/microbench/div_exact.hip checks that on the device: the reciprocal EXHAUSTIVELY -- every float with
2^-120 <= |x| < 2^121, 4.04e9 inputs -- and the quotient on 1.18e10 pairs (pseudo-random and hard mantissa patterns)."""
import os
import shutil
import subprocess

import pytest

from mvskit_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the device programs that include mvs_math.cuh are built as the engine is: its arithmetic flags, as an executable
ENGINE_FLAGS = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]


@pytest.mark.gpu
def test_rcp_and_div_return_the_ieee_quotient(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "div_exact")
    subprocess.check_call([hipcc, *ENGINE_FLAGS, "-Wno-unused-result", "-o", exe,
                           os.path.join(ROOT, "tools", "microbench", "div_exact.hip")], stderr=subprocess.DEVNULL)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout + r.stderr
    assert "4043309056 inputs" in r.stdout and ", 0 differ from 1.0f / x" in r.stdout


@pytest.mark.gpu
def test_engine_arithmetic_over_its_whole_domain(tmp_path):
    """tools/microbench/math_exact.hip, which includes mvs_math.cuh: sqrt_rn against the fp64 root on every float from 2^-96 to +inf
    (and that reference against sqrtf on the host), pm_sincosf against pm_sinf / pm_cosf on all 2^32 patterns, the five pm_*
    functions against the device's fp64 libm on every float of their domains (each maximum at most 1e-6 rad), rng_tail(rng_prefix())
    against rng_uniform on 2^30 draws and against an integer restatement on the host.  The program takes 0.56 to 0.67 s on an MI355X
    (about 0.3 s of it the host's loop over the square roots, on 16 threads); the limit is ten times that."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "math_exact")
    subprocess.check_call([hipcc, *ENGINE_FLAGS, "-Wno-unused-result", "-o", exe,
                           os.path.join(ROOT, "tools", "microbench", "math_exact.hip")], stderr=subprocess.DEVNULL)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=6)
    print(r.stdout)
    out = r.stdout
    assert r.returncode == 0 and "PASS" in out and "FAIL" not in out, out + r.stderr
    assert "sqrt reference on the host: 1879048195 inputs, 0 differ between" in out
    assert "sqrt_rn: 1879048195 inputs" in out and ", 0 differ from (float)sqrt((double)x)" in out
    assert "pm_sincosf: 4294967296 inputs" in out and ", 0 differ from pm_sinf / pm_cosf" in out
    for name, count in (("sin", 2157060024), ("cos", 2157060024), ("asin", 2130706434), ("acos", 2130706434), ("atan", 4278190082)):
        assert f"pm_{name}f: {count} inputs" in out, name
    assert out.count(", 0 NaN: within 1e-6") == 5
    assert "rng: 1073741888 draws, 0 differ between rng_tail(rng_prefix()) and rng_uniform, 0 outside [-0.5, 0.5)" in out
    assert "first 1048576 draws on the host, 0 differ from the integer restatement" in out


@pytest.mark.gpu
def test_run_lookup_by_marks_is_the_search(tmp_path):
    """findNeighbors' row walk (mvs_check.cuh, MK): the run an id belongs to comes from marks and four DPP running maxima instead of
    a binary search per id.  tools/microbench/run_lookup.hip runs both on 65536 waves of 64 runs of random lengths (empty runs, runs
    longer than the 256-position window) and counts the positions that differ."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "run_lookup")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-Wno-unused-result", "-o", exe,
                           os.path.join(ROOT, "tools", "microbench", "run_lookup.hip")], stderr=subprocess.DEVNULL)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "PASS" in r.stdout and " 0 positions differ" in r.stdout, r.stdout + r.stderr
