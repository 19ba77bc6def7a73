"""format_g of mvskit_amd/csrc/mvs_plyfmt.h as the GPU runs it (k_ply_colour / k_ply_emit): tools/microbench/ply_format.hip formats
EVERY float bit pattern (2^32) on the device and compares each with the host's printf("%g", (double)f)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_device_format_g_is_printf_for_every_float(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "ply_format")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "mvskit_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tools", "microbench", "ply_format.hip")], stderr=subprocess.DEVNULL)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout + r.stderr
    assert "4294967296 inputs" in r.stdout and ", 0 differ" in r.stdout
