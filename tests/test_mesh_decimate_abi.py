"""CPU-side checks of the mesh decimation entry points (include/mvskit_engine.h: mvs_mesh_decimation, mvs_default_mesh_decimation,
mvs_engine_mesh_decimate): every engine library exports them, the struct is 24 bytes with the header's offsets and defaults, and bad
arguments are refused in the header's order before the handle is read or a device is touched, with nothing written through an output
pointer."""
import ctypes as C
import os

import numpy as np
import pytest

from mvskit_amd import build, engine
from mvskit_amd.engine import MVS_ERR_ARG

SYMBOLS = ("mvs_default_mesh_decimation", "mvs_engine_mesh_decimate")
HEADER = os.path.join(build.ROOT, "include", "mvskit_engine.h")


def test_header_declares_them():
    text = open(HEADER).read()
    for name in SYMBOLS + ("mvs_mesh_decimation",):
        assert name + "(" in text or name + ";" in text, name
    # what clustering does not promise, and aliasing, are part of the contract
    assert "WHAT CLUSTERING DOES NOT PROMISE" in text and "need not be manifold" in text and text.count("ALIASES") >= 2


def test_the_new_file_is_a_source_of_the_build():
    assert "mvs_mesh_decimate.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "mvs_mesh_decimate.hip"))


@pytest.mark.parametrize("cap", [16, 32, 64])
def test_symbols_layout_defaults_and_argument_checks(cap):
    build.build_engine(cap=cap)
    lib = engine.load_library(cap=cap)
    for name in SYMBOLS:
        assert hasattr(lib, name), f"libmvskit_engine (cap {cap}) has no {name}"
        assert name in engine.EXPORTS
    D = engine.MeshDecimation
    assert C.sizeof(D) == 24 and [(n, getattr(D, n).offset) for n, _ in D._fields_] == [("origin", 0), ("cell", 12), ("placement", 16), ("pad", 20)]
    d = D((C.c_float * 3)(-5, -5, -5), -5.0, -5, -5)
    lib.mvs_default_mesh_decimation(C.byref(d))
    assert list(d.origin) == [0.0, 0.0, 0.0] and d.cell == 1.0 and d.placement == 0
    lib.mvs_default_mesh_decimation(None)  # ignored

    def err(word):
        return word in lib.mvs_last_error()

    vp = C.c_void_p
    verts = np.full((8, 3), -7, np.float32)
    tris = np.full((8, 3), -7, np.int32)
    out_v = np.full((8, 3), -7, np.float32)
    out_t = np.full((8, 3), -7, np.int32)
    vmap = np.full(8, -7, np.int32)
    nvo, nto = C.c_int64(-7), C.c_int64(-7)
    vtp, trp, ovp, otp, vmp = (a.ctypes.data_as(vp) for a in (verts, tris, out_v, out_t, vmap))
    big = (1 << 30) + 1
    bad_counts = ((-1, 8), (8, -1), (big, 8), (8, big))
    nan, inf = float("nan"), float("inf")

    def dc(cell=1.0, origin=(0.0, 0.0, 0.0), placement=0):
        return C.byref(D((C.c_float * 3)(*origin), cell, placement, 0))

    # d, cell, origin, placement, the counts, verts, tris, the size pointers, the caps, the engine -- each with every later argument bad too
    g = lib.mvs_engine_mesh_decimate
    assert g(None, None, -1, None, -1, None, -1, None, -1, None, None, None, None) == MVS_ERR_ARG and err(b"decimation null")
    for cell in (0.0, -1.0, nan, inf, -inf):
        assert g(None, dc(cell, (nan, nan, nan), 2), -1, None, -1, None, -1, None, -1, None, None, None, None) == MVS_ERR_ARG and err(b"cell"), cell
    for k in range(3):
        for x in (nan, inf, -inf):
            o = [0.0, 0.0, 0.0]
            o[k] = x
            assert g(None, dc(1.0, o, 2), -1, None, -1, None, -1, None, -1, None, None, None, None) == MVS_ERR_ARG and err(b"origin"), (k, x)
    for pl in (2, -1):
        assert g(None, dc(placement=pl), -1, None, -1, None, -1, None, -1, None, None, None, None) == MVS_ERR_ARG and err(b"placement"), pl
    for nv, nt in bad_counts:
        assert g(None, dc(), nv, None, nt, None, -1, None, -1, None, None, None, None) == MVS_ERR_ARG and err(b"count"), (nv, nt)
    assert g(None, dc(), 8, None, 8, None, -1, None, -1, None, None, None, None) == MVS_ERR_ARG and err(b"verts null")
    assert g(None, dc(), 8, vtp, 8, None, -1, None, -1, None, None, None, None) == MVS_ERR_ARG and err(b"tris null")
    assert g(None, dc(), 8, vtp, 8, trp, -1, ovp, -1, otp, vmp, None, C.byref(nto)) == MVS_ERR_ARG and err(b"null")
    assert g(None, dc(), 8, vtp, 8, trp, -1, ovp, -1, otp, vmp, C.byref(nvo), None) == MVS_ERR_ARG and err(b"null")
    assert g(None, dc(), 8, vtp, 8, trp, -1, ovp, 8, otp, vmp, C.byref(nvo), C.byref(nto)) == MVS_ERR_ARG and err(b"negative cap")
    assert g(None, dc(), 8, vtp, 8, trp, 8, ovp, -1, otp, vmp, C.byref(nvo), C.byref(nto)) == MVS_ERR_ARG and err(b"negative cap")
    assert g(None, dc(), 8, vtp, 8, trp, 8, ovp, 8, otp, vmp, C.byref(nvo), C.byref(nto)) == MVS_ERR_ARG and err(b"no engine")
    # the ends of the ranges that are allowed
    assert g(None, dc(1e-30, (-3e38, 3e38, 0.0), 1), 0, None, 0, None, 0, None, 0, None, None, C.byref(nvo), C.byref(nto)) == MVS_ERR_ARG and err(b"no engine")
    assert g(None, dc(3e38), 1 << 30, vtp, 1 << 30, trp, 0, None, 0, None, None, C.byref(nvo), C.byref(nto)) == MVS_ERR_ARG and err(b"no engine")

    # nothing was written on any refused call
    for a in (verts, tris, out_v, out_t, vmap):
        assert (a == -7).all()
    assert (nvo.value, nto.value) == (-7, -7)
