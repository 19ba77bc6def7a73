"""CPU-side checks of the dense-map entry points (include/mvskit_engine.h: mvs_maps_config, mvs_view_maps, mvs_fused_point,
mvs_default_maps_config, mvs_engine_render_maps, mvs_engine_fused_points): every engine library exports them, the structs have the
declared sizes and layouts, the defaults are the header's, and bad arguments are refused in the header's order before the handle is read
or a device is touched -- with nothing written through an output pointer (no compute calls here)."""
import ctypes as C

import numpy as np
import pytest

from mvskit_amd import build, engine
from mvskit_amd.engine import MVS_ERR_ARG

SYMBOLS = ("mvs_default_maps_config", "mvs_engine_render_maps", "mvs_engine_fused_points")


@pytest.mark.parametrize("cap", [16, 32, 64])
def test_maps_symbols_layout_defaults_and_argument_checks(cap):
    build.build_engine(cap=cap)
    lib = engine.load_library(cap=cap)
    for name in SYMBOLS:
        assert hasattr(lib, name), f"libmvskit_engine (cap {cap}) has no {name}"
        assert name in engine.EXPORTS
    # the three structs: 24, 40 and 32 bytes, the fields where the header declares them
    S, V, F = engine.MapsConfig, engine.ViewMaps, engine.FUSED_POINT_DTYPE
    assert (C.sizeof(S), C.sizeof(V), F.itemsize) == (24, 40, 32)
    assert [(n, getattr(S, n).offset) for n, _ in S._fields_] == [("source", 0), ("min_consistent", 4), ("depth_tol", 8), ("normal_cos", 12),
                                                                   ("dedupe", 16), ("pad", 20)]
    assert [(n, getattr(V, n).offset) for n, _ in V._fields_] == [("depth", 0), ("normal", 8), ("conf", 16), ("ids", 24), ("agree", 32)]
    assert [(n, F.fields[n][1]) for n in F.names] == [("xyz", 0), ("normal", 12), ("conf", 24), ("rgb", 28), ("view", 31)]
    # the defaults: source 0, min_consistent 1, depth_tol 0.01, normal_cos 0.9, dedupe 1; nothing written past 24 bytes
    raw = (C.c_uint8 * 32)(*([0xAB] * 32))
    lib.mvs_default_maps_config(C.cast(raw, C.POINTER(S)))
    d = S.from_buffer_copy(bytes(raw[:24]))
    assert (d.source, d.min_consistent, d.dedupe) == (0, 1, 1)
    assert (np.float32(d.depth_tol), np.float32(d.normal_cos)) == (np.float32(0.01), np.float32(0.9))
    assert bytes(raw[24:]) == b"\xab" * 8

    def err(word):
        return word in lib.mvs_last_error()

    def cfg(**kw):
        c = S.from_buffer_copy(bytes(raw[:24]))
        for k, v in kw.items():
            setattr(c, k, v)
        return C.byref(c)

    nan, inf = float("nan"), float("inf")
    # the ladder, every rung with a null engine, which none of them reads; every later field is bad too, so the order shows
    depth = np.full(4, -7, np.float32)
    slots = (V * 1)()
    slots[0].depth = depth.ctypes.data
    nvalid = np.full(1, -7, np.int64)
    nv = nvalid.ctypes.data_as(C.c_void_p)
    render = lib.mvs_engine_render_maps
    assert render(None, None, slots, nv) == MVS_ERR_ARG and err(b"config null")
    for s in (-1, 2):
        assert render(None, cfg(source=s, min_consistent=-1, depth_tol=nan, normal_cos=nan), slots, nv) == MVS_ERR_ARG and err(b"source"), s
    assert render(None, cfg(min_consistent=-1, depth_tol=nan, normal_cos=nan), slots, nv) == MVS_ERR_ARG and err(b"min_consistent")
    for t in (0.0, -0.01, nan, inf):
        assert render(None, cfg(depth_tol=t, normal_cos=nan), slots, nv) == MVS_ERR_ARG and err(b"depth_tol"), t
    for c in (1.5, nan, inf, -inf):
        assert render(None, cfg(normal_cos=c), slots, nv) == MVS_ERR_ARG and err(b"normal_cos"), c
    assert render(None, cfg(), slots, nv) == MVS_ERR_ARG and err(b"no engine")
    assert render(None, cfg(normal_cos=-2.0, source=1, min_consistent=63), None, None) == MVS_ERR_ARG and err(b"no engine")
    assert (depth == -7).all() and nvalid[0] == -7  # nothing is written on a refused call
    # mvs_engine_fused_points: the same ladder, then cap and n, then the engine
    out = np.zeros(4, dtype=F)
    op = out.ctypes.data_as(C.c_void_p)
    n = C.c_int64(-7)
    fused = lib.mvs_engine_fused_points
    assert fused(None, None, -1, op, None) == MVS_ERR_ARG and err(b"config null")
    assert fused(None, cfg(source=2, min_consistent=-1), -1, op, None) == MVS_ERR_ARG and err(b"source")
    assert fused(None, cfg(min_consistent=-1, depth_tol=0.0), -1, op, None) == MVS_ERR_ARG and err(b"min_consistent")
    assert fused(None, cfg(depth_tol=0.0, normal_cos=2.0), -1, op, None) == MVS_ERR_ARG and err(b"depth_tol")
    assert fused(None, cfg(normal_cos=2.0), -1, op, None) == MVS_ERR_ARG and err(b"normal_cos")
    assert fused(None, cfg(), -1, op, C.byref(n)) == MVS_ERR_ARG and err(b"cap negative or n null")
    assert fused(None, cfg(), 4, op, None) == MVS_ERR_ARG and err(b"cap negative or n null")
    assert fused(None, cfg(), 4, op, C.byref(n)) == MVS_ERR_ARG and err(b"no engine")
    assert fused(None, cfg(), 0, None, C.byref(n)) == MVS_ERR_ARG and err(b"no engine")
    assert n.value == -7 and not out.view(np.uint8).any()


@pytest.mark.parametrize("cap", [16, 32, 64])
def test_existing_struct_sizes_are_unchanged_by_the_maps(cap):
    """mvs_config, mvs_timing, mvs_patch and the seeding structs keep their sizes: the new calls brought their own"""
    build.build_engine(cap=cap)
    lib = engine.load_library(cap=cap)
    assert hasattr(lib, "mvs_engine_render_maps")
    assert (C.sizeof(engine.Config), C.sizeof(engine.Timing), C.sizeof(engine.SeedRandom), C.sizeof(engine.SeedPoints)) == (96, 40, 32, 8)
    assert lib.mvs_patch_bytes() == (192 if cap == 64 else 128)
