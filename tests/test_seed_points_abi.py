"""CPU-side checks of the warm-start entry points (include/mvskit_engine.h: mvs_seed_points, mvs_default_seed_points,
mvs_engine_seed_points, mvs_engine_seed_points_hypotheses, mvs_engine_depth_ranges): every engine library exports them, the parameter
struct has the declared layout and defaults, and bad arguments are refused in the header's order before the handle is read or a device
is touched (no compute calls here)."""
import ctypes as C

import numpy as np
import pytest

from mvskit_amd import build, engine
from mvskit_amd.engine import MVS_ERR_ARG

SYMBOLS = ("mvs_default_seed_points", "mvs_engine_seed_points", "mvs_engine_seed_points_hypotheses", "mvs_engine_depth_ranges")


@pytest.mark.parametrize("cap", [16, 32, 64])
def test_seed_points_symbols_layout_defaults_and_argument_checks(cap):
    build.build_engine(cap=cap)
    lib = engine.load_library(cap=cap)
    for name in SYMBOLS:
        assert hasattr(lib, name), f"libmvskit_engine (cap {cap}) has no {name}"
        assert name in engine.EXPORTS
    # the struct: 8 bytes, the fields where the header declares them
    S = engine.SeedPoints
    assert C.sizeof(S) == 8
    assert [(n, getattr(S, n).offset) for n, _ in S._fields_] == [("hypotheses", 0), ("min_ncc", 4)]
    # the defaults: K 4, min_ncc -1 (= nccThresholdBefore at the call); nothing written past 8 bytes
    raw = (C.c_uint8 * 16)(*([0xAB] * 16))
    lib.mvs_default_seed_points(C.cast(raw, C.POINTER(S)))
    d = S.from_buffer_copy(bytes(raw[:8]))
    assert (d.hypotheses, d.min_ncc) == (4, -1.0)
    assert bytes(raw[8:]) == b"\xab" * 8

    def err(word):
        return word in lib.mvs_last_error()

    xyz = np.ones((2, 3), np.float32)
    xp = xyz.ctypes.data_as(C.c_void_p)
    good = S(4, -1.0)
    # mvs_engine_seed_points: the refusals in the header's order, every one of them with a null engine, which none of them reads
    added = C.c_int64(-7)
    assert lib.mvs_engine_seed_points(None, None, 2, xp, C.byref(added)) == MVS_ERR_ARG and err(b"null")
    for k in (0, -1, 65):
        assert lib.mvs_engine_seed_points(None, C.byref(S(k, -1.0)), -1, None, C.byref(added)) == MVS_ERR_ARG and err(b"hypotheses"), k
    assert lib.mvs_engine_seed_points(None, C.byref(good), -1, None, C.byref(added)) == MVS_ERR_ARG and err(b"negative")
    assert lib.mvs_engine_seed_points(None, C.byref(good), 2, None, C.byref(added)) == MVS_ERR_ARG and err(b"xyz")
    assert lib.mvs_engine_seed_points(None, C.byref(good), 2, xp, C.byref(added)) == MVS_ERR_ARG and err(b"no engine")
    assert lib.mvs_engine_seed_points(None, C.byref(good), 0, None, C.byref(added)) == MVS_ERR_ARG and err(b"no engine")
    assert lib.mvs_engine_seed_points(None, C.byref(good), (1 << 30) + 1, xp, C.byref(added)) == MVS_ERR_ARG and err(b"no engine")  # before the limit
    assert added.value == -7  # nothing is written on a refused call
    # the diagnostic window: the same checks, then its own
    out = np.zeros(8, dtype=engine.synth.patch_dtype((lib.mvs_patch_bytes() - 64) // 2))
    count = np.full(2, -7, np.int32)
    op, cp = out.ctypes.data_as(C.c_void_p), count.ctypes.data_as(C.c_void_p)
    hyp = lib.mvs_engine_seed_points_hypotheses
    assert hyp(None, None, 2, xp, op, cp) == MVS_ERR_ARG and err(b"null")
    for k in (0, -1, 65):
        assert hyp(None, C.byref(S(k, -1.0)), -1, None, None, None) == MVS_ERR_ARG and err(b"hypotheses"), k
    assert hyp(None, C.byref(good), -1, None, None, None) == MVS_ERR_ARG and err(b"negative")
    assert hyp(None, C.byref(good), 2, None, None, None) == MVS_ERR_ARG and err(b"xyz")
    assert hyp(None, C.byref(good), 2, xp, None, cp) == MVS_ERR_ARG and err(b"out or count")
    assert hyp(None, C.byref(good), 2, xp, op, None) == MVS_ERR_ARG and err(b"out or count")
    assert hyp(None, C.byref(good), 2, xp, op, cp) == MVS_ERR_ARG and err(b"no engine")
    assert not out.view(np.uint8).any() and (count == -7).all()
    # the depth ranges
    lo, hi, cnt = np.full(3, -7, np.float32), np.full(3, -7, np.float32), np.full(3, -7, np.int64)
    lp, hp, np_ = (a.ctypes.data_as(C.c_void_p) for a in (lo, hi, cnt))
    rng = lib.mvs_engine_depth_ranges
    m = C.c_float(0.1)
    assert rng(None, -1, None, C.c_float(-0.1), None, None, None) == MVS_ERR_ARG and err(b"negative")
    assert rng(None, 2, None, C.c_float(-0.1), None, None, None) == MVS_ERR_ARG and err(b"xyz")
    for ptrs in ((None, hp, np_), (lp, None, np_), (lp, hp, None)):
        assert rng(None, 2, xp, C.c_float(-0.1), *ptrs) == MVS_ERR_ARG and err(b"count null"), ptrs
    for bad in (-0.1, float("nan"), float("inf")):
        assert rng(None, 2, xp, C.c_float(bad), lp, hp, np_) == MVS_ERR_ARG and err(b"margin"), bad
    assert rng(None, 2, xp, m, lp, hp, np_) == MVS_ERR_ARG and err(b"no engine")
    assert rng(None, 0, None, C.c_float(0.0), lp, hp, np_) == MVS_ERR_ARG and err(b"no engine")
    assert (lo == -7).all() and (hi == -7).all() and (cnt == -7).all()


@pytest.mark.parametrize("cap", [16, 32, 64])
def test_existing_struct_sizes_are_unchanged(cap):
    """mvs_config, mvs_timing and mvs_patch keep their sizes: the new calls brought their own struct."""
    build.build_engine(cap=cap)
    lib = engine.load_library(cap=cap)
    assert C.sizeof(engine.Config) == 96
    assert C.sizeof(engine.Timing) == 40
    assert C.sizeof(engine.SeedRandom) == 32
    assert lib.mvs_patch_bytes() == (192 if cap == 64 else 128)
    raw = (C.c_uint8 * 104)(*([0xCD] * 104))
    lib.mvs_default_config(C.cast(raw, C.POINTER(engine.Config)))
    assert bytes(raw[96:]) == b"\xcd" * 8  # nothing written past 96 bytes
