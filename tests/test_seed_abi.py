"""CPU-side checks of mvs_engine_seed_patches (include/mvskit_engine.h): every engine library exports it and it refuses bad arguments
before it reads the handle or touches a device (no compute calls here)."""
import ctypes as C

import numpy as np
import pytest

from mvskit_amd import build, engine
from mvskit_amd.engine import MVS_ERR_ARG


@pytest.mark.parametrize("cap", [16, 32, 64])
def test_seed_patches_symbol_and_argument_checks(cap):
    build.build_engine(cap=cap)
    lib = engine.load_library(cap=cap)
    assert hasattr(lib, "mvs_engine_seed_patches"), f"libmvskit_engine (cap {cap}) has no mvs_engine_seed_patches"
    assert "mvs_engine_seed_patches" in engine.EXPORTS
    xyz = np.zeros((4, 3), np.float32)
    views = (engine.SeedView * 3)()
    added = C.c_int64(-7)
    xp = xyz.ctypes.data_as(C.c_void_p)
    # no engine
    assert lib.mvs_engine_seed_patches(None, 4, xp, views, C.byref(added)) == MVS_ERR_ARG
    assert b"no engine" in lib.mvs_last_error()
    assert added.value == -7  # nothing is written on a refused call
    # the arguments are looked at before the handle: none of these reads the (null) engine
    assert lib.mvs_engine_seed_patches(None, -1, xp, views, C.byref(added)) == MVS_ERR_ARG
    assert b"negative" in lib.mvs_last_error()
    assert lib.mvs_engine_seed_patches(None, 4, None, views, C.byref(added)) == MVS_ERR_ARG
    assert lib.mvs_engine_seed_patches(None, 4, xp, None, C.byref(added)) == MVS_ERR_ARG
    assert lib.mvs_engine_seed_patches(None, 2 ** 31, xp, views, C.byref(added)) == MVS_ERR_ARG
    assert C.sizeof(engine.SeedView) == 16


def test_host_mirror_links_the_seed_entry_point():
    """DepthNormInit::createPatches calls the engine: the host library resolves the symbol, and keeps its CPU yardstick."""
    build.build_engine()
    engine.load_library()
    host = C.CDLL(build.build_host())
    for name in ("mvshost_seeds_from_plys", "mvshost_seed_cpu_probe", "mvshost_seed_cpu_ms"):
        assert hasattr(host, name), name
