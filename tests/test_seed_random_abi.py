"""CPU-side checks of the cold-start entry points (include/mvskit_engine.h: mvs_seed_random, mvs_default_seed_random,
mvs_engine_seed_random, mvs_engine_seed_random_hypotheses): every engine library exports them, the parameter struct has the declared
layout and defaults, and bad arguments are refused before the handle is read or a device is touched (no compute calls here)."""
import ctypes as C
import math

import numpy as np
import pytest

from mvskit_amd import build, engine
from mvskit_amd.engine import MVS_ERR_ARG

SYMBOLS = ("mvs_default_seed_random", "mvs_engine_seed_random", "mvs_engine_seed_random_hypotheses")


def _args(lib, n=3, **kw):
    s = engine.SeedRandom()
    lib.mvs_default_seed_random(C.byref(s))
    lo, hi = np.full(n, 2.0, np.float32), np.full(n, 5.0, np.float32)
    s.depth_min, s.depth_max = lo.ctypes.data, hi.ctypes.data
    for k, v in kw.items():
        setattr(s, k, v)
    return s, (lo, hi)


@pytest.mark.parametrize("cap", [16, 32, 64])
def test_seed_random_symbols_layout_defaults_and_argument_checks(cap):
    build.build_engine(cap=cap)
    lib = engine.load_library(cap=cap)
    for name in SYMBOLS:
        assert hasattr(lib, name), f"libmvskit_engine (cap {cap}) has no {name}"
        assert name in engine.EXPORTS
    # the struct: 32 bytes, the fields where the header declares them
    S = engine.SeedRandom
    assert C.sizeof(S) == 32
    assert [(n, getattr(S, n).offset) for n, _ in S._fields_] == [("hypotheses", 0), ("seed", 4), ("max_tilt", 8), ("min_ncc", 12),
                                                                   ("depth_min", 16), ("depth_max", 24)]
    # the defaults: K 8, seed 1, max_tilt pi / 3, min_ncc -1 (= nccThresholdBefore at the call), no ranges
    raw = (C.c_uint8 * 32)(*([0xAB] * 32))
    lib.mvs_default_seed_random(C.cast(raw, C.POINTER(S)))
    d = S.from_buffer_copy(raw)
    assert (d.hypotheses, d.seed, d.min_ncc, d.depth_min, d.depth_max) == (8, 1, -1.0, None, None)
    assert d.max_tilt == np.float32(math.pi / 3)
    # the refusals, in the header's order; every one of them with a null engine, which none of them reads
    added = C.c_int64(-7)

    def run(s):
        return lib.mvs_engine_seed_random(None, C.byref(s) if s is not None else None, C.byref(added))

    assert run(None) == MVS_ERR_ARG and b"null" in lib.mvs_last_error()
    for k in (0, -1, 65):
        s, keep = _args(lib, hypotheses=k)
        assert run(s) == MVS_ERR_ARG and b"hypotheses" in lib.mvs_last_error(), k
    for name in ("depth_min", "depth_max"):
        s, keep = _args(lib, **{name: None})
        assert run(s) == MVS_ERR_ARG and b"range" in lib.mvs_last_error(), name
    for tilt in (0.0, -0.1, float(np.nextafter(np.float32(math.pi / 3), np.float32(2))), float("nan"), float("inf")):
        s, keep = _args(lib, max_tilt=tilt)
        assert run(s) == MVS_ERR_ARG and b"max_tilt" in lib.mvs_last_error(), tilt
    s, keep = _args(lib)
    assert run(s) == MVS_ERR_ARG and b"no engine" in lib.mvs_last_error()
    assert added.value == -7  # nothing is written on a refused call
    # the diagnostic window: the same checks, then its own
    cells = np.zeros(2, np.int32)
    out = np.zeros(16, dtype=engine.synth.patch_dtype((lib.mvs_patch_bytes() - 64) // 2))
    cp, op = cells.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    assert lib.mvs_engine_seed_random_hypotheses(None, None, 0, 2, cp, op) == MVS_ERR_ARG
    s, keep = _args(lib, hypotheses=65)
    assert lib.mvs_engine_seed_random_hypotheses(None, C.byref(s), 0, 2, cp, op) == MVS_ERR_ARG and b"hypotheses" in lib.mvs_last_error()
    s, keep = _args(lib)
    assert lib.mvs_engine_seed_random_hypotheses(None, C.byref(s), 0, -1, cp, op) == MVS_ERR_ARG
    assert lib.mvs_engine_seed_random_hypotheses(None, C.byref(s), 0, 2, None, op) == MVS_ERR_ARG
    assert lib.mvs_engine_seed_random_hypotheses(None, C.byref(s), 0, 2, cp, None) == MVS_ERR_ARG
    assert lib.mvs_engine_seed_random_hypotheses(None, C.byref(s), 0, 2, cp, op) == MVS_ERR_ARG and b"no engine" in lib.mvs_last_error()
    assert not out.view(np.uint8).any()


@pytest.mark.parametrize("cap", [16, 32, 64])
def test_existing_struct_sizes_are_unchanged(cap):
    """mvs_config, mvs_timing and mvs_patch keep their sizes: the new call brought its own struct."""
    build.build_engine(cap=cap)
    lib = engine.load_library(cap=cap)
    assert C.sizeof(engine.Config) == 96
    assert C.sizeof(engine.Timing) == 40
    assert lib.mvs_patch_bytes() == (192 if cap == 64 else 128)
    # the library agrees with the binding about mvs_config: the last field of the defaults lands where the binding reads it
    cfg = engine.Config()
    raw = (C.c_uint8 * 104)(*([0xCD] * 104))
    lib.mvs_default_config(C.cast(raw, C.POINTER(engine.Config)))
    assert bytes(raw[96:]) == b"\xcd" * 8  # nothing written past 96 bytes
    cfg = engine.Config.from_buffer_copy(bytes(raw[:96]))
    assert cfg.max_patches == 0 and cfg.csize == 2
