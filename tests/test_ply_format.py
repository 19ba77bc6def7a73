"""The vertex text of mvs_engine_export_ply (mvskit_amd/csrc/mvs_plyfmt.h) against the C library's printf("%g", (double)f), which is
what PatchManager::writePly's std::ostream wrote (patch_manager.cpp:542-633): the header compiled with g++ into a throwaway driver that
formats 4.3e7 floats -- every float of four whole binades, samples of every exponent of both signs, exact half-way cases, the edges
of the float range and the non-finite values -- and prints each mismatch.  Plus the C ABI's argument checks of the new call, which need
no GPU."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from mvskit_amd import build, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mvskit_amd", "csrc")

DRIVER = r"""
#include "mvs_plyfmt.h"
#include <atomic>
#include <cstdio>
#include <cstring>
#include <cstdint>
#include <mutex>
#include <thread>
#include <vector>
static std::atomic<unsigned long long> n_checked{0}, n_bad{0};
static std::mutex mu;
static void check(uint32_t bits) {
    float f;
    memcpy(&f, &bits, 4);
    char want[64], got[64];
    snprintf(want, sizeof want, "%g", (double)f);
    const int len = mvsply::format_g(f, got);
    got[len] = 0;
    const int len0 = mvsply::format_g(f, nullptr);  // the length pass counts what the emit pass writes
    ++n_checked;
    if (strcmp(want, got) != 0 || len0 != len || len > 12) {
        if (n_bad++ < 50) { std::lock_guard<std::mutex> g(mu); printf("MISMATCH 0x%08x want '%s' got '%s' (%d / %d chars)\n", bits, want, got, len, len0); }
    }
}
static void binade(uint32_t bexp, uint32_t sign) { for (uint32_t m = 0; m < (1u << 23); ++m) check((sign << 31) | (bexp << 23) | m); }
static uint32_t mix(uint32_t h) { h ^= h >> 16; h *= 0x7feb352du; h ^= h >> 15; h *= 0x846ca68bu; h ^= h >> 16; return h; }
int main() {
    std::vector<std::thread> th;
    // every float of four binades: around 1e-5 (2^-17), 1, 1e5 (2^16) and 1e6 (2^20: the integers and half-integers with ties)
    th.emplace_back(binade, 127u - 17u, 0u);
    th.emplace_back(binade, 127u, 1u);
    th.emplace_back(binade, 127u + 16u, 0u);
    th.emplace_back(binade, 127u + 20u, 0u);
    th.emplace_back([] {
        // every exponent of both signs (subnormals and non-finite included): the mantissa edges and 8192 pseudo-random mantissas
        for (uint32_t s = 0; s < 2; ++s)
            for (uint32_t ex = 0; ex < 256; ++ex) {
                const uint32_t fixed[5] = {0u, 1u, 2u, 0x400000u, 0x7fffffu};
                for (uint32_t m : fixed) check((s << 31) | (ex << 23) | m);
                for (uint32_t k = 0; k < 8192; ++k) check((s << 31) | (ex << 23) | (mix(k * 2654435761u + ex * 977u + s) & 0x7fffffu));
            }
        // exact half-way cases (F + 1/2) 10^q that are floats: 6-digit F, q = 0 .. 4, and the same scaled by powers of two
        for (uint32_t k = 0; k < (1u << 20); ++k) {
            const uint32_t F = 100000u + mix(k ^ 0x5bd1e995u) % 900000u;
            const int q = (int)(k % 5u);
            double v = (2.0 * F + 1.0) / 2.0;
            for (int i = 0; i < q; ++i) v *= 10.0;
            const float f = (float)v;
            if ((double)f != v) continue;
            uint32_t b;
            memcpy(&b, &f, 4);
            check(b);
            check(b ^ 0x80000000u);
        }
        const uint32_t named[] = {0x00000000u, 0x80000000u, 0x00000001u, 0x80000001u, 0x007fffffu, 0x00800000u, 0x7f7fffffu, 0xff7fffffu,
                                  0x7f800000u, 0xff800000u, 0x7fc00000u, 0xffc00000u, 0x7f800001u, 0x3f800000u, 0x49969a28u /* 1234565 */,
                                  0x49969b18u /* 1234575 */, 0x47f12040u /* 123456.5 */};
        for (uint32_t b : named) check(b);
    });
    for (auto& t : th) t.join();
    printf("%s %llu inputs, %llu differ\n", n_bad == 0 ? "PASS" : "FAIL", (unsigned long long)n_checked, (unsigned long long)n_bad);
    return n_bad == 0 ? 0 : 1;
}
"""


def test_format_g_equals_printf(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to compile the formatter for the CPU"
    src = tmp_path / "ply_format_driver.cpp"
    src.write_text(DRIVER)
    exe = str(tmp_path / "ply_format_driver")
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-pthread", "-Wall", "-I", CSRC, str(src), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("differ") and " 0 differ" in r.stdout, r.stdout + r.stderr
    n = int(r.stdout.split("PASS ")[1].split(" inputs")[0])
    assert n >= 4 * 2 ** 23 + 2 ** 22, n


def test_format_line_is_the_ostream_line(tmp_path):
    """The whole vertex line: six floats and three colour values, blanks between, one newline."""
    gxx = shutil.which("g++")
    src = tmp_path / "line.cpp"
    src.write_text(r"""
#include "mvs_plyfmt.h"
#include <cstdio>
int main() {
    char buf[MVS_PLY_LINE_MAX + 1];
    const int n = mvsply::format_line(-0.0f, 1234565.0f, 1e-5f, 0.5f, -0.333333343f, 123456.5f, 0, 128, 255, buf);
    buf[n] = 0;
    printf("%d|%s", mvsply::format_line(-0.0f, 1234565.0f, 1e-5f, 0.5f, -0.333333343f, 123456.5f, 0, 128, 255, nullptr), buf);
}
""")
    exe = str(tmp_path / "line")
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-I", CSRC, str(src), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    line = "-0 1.23456e+06 1e-05 0.5 -0.333333 123456 0 128 255\n"
    assert out == f"{len(line)}|{line}"


@pytest.fixture(scope="module")
def lib():
    return C.CDLL(build.build_engine())


def test_export_ply_symbol_and_argument_checks(lib):
    assert "mvs_engine_export_ply" in engine.EXPORTS
    f = lib.mvs_engine_export_ply
    f.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.POINTER(C.c_int64)]
    f.restype = C.c_int
    n = C.c_int64(-7)
    assert f(None, 0, 0, None, C.byref(n)) == -1  # MVS_ERR_ARG: no engine
    assert f(None, 1, 0, None, C.byref(n)) == -1
    # a configured engine needs a device; the format is checked before anything else of the handle is looked at
    assert f(C.c_void_p(1), 2, 0, None, C.byref(n)) == -1  # MVS_ERR_ARG: bad format
    assert f(C.c_void_p(1), -1, 0, None, C.byref(n)) == -1
    assert f(C.c_void_p(1), 0, 0, None, None) == -1  # MVS_ERR_ARG: no nbytes
    assert n.value == -7  # nothing was written
