"""CPU-side checks of the hole-filling entry points (include/mvskit_engine.h: mvs_mesh_filling, mvs_default_mesh_filling,
mvs_engine_mesh_boundaries, mvs_engine_mesh_fill): every engine library exports them, the struct is 8 bytes with the header's offsets and
default, and bad arguments are refused in the header's order before the handle is read or a device is touched, with nothing written
through an output pointer."""
import ctypes as C
import os

import numpy as np
import pytest

from mvskit_amd import build, engine
from mvskit_amd.engine import MVS_ERR_ARG

SYMBOLS = ("mvs_default_mesh_filling", "mvs_engine_mesh_boundaries", "mvs_engine_mesh_fill")
HEADER = os.path.join(build.ROOT, "include", "mvskit_engine.h")


def test_header_declares_them():
    text = open(HEADER).read()
    for name in SYMBOLS + ("mvs_mesh_filling",):
        assert name + "(" in text or name + ";" in text, name
    # the terms of the contract, what filling does not do, and aliasing
    for word in ("BOUNDARY", "IRREGULAR", "SIMPLE", "COMPLEX", "LENGTH 3", "LENGTH >= 4", "WHAT FILLING DOES NOT DO", "loop vertex"):
        assert word in text, word
    assert text.count("ALIASES") >= 3


def test_the_new_file_is_a_source_of_the_build():
    assert "mvs_mesh_fill.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "mvs_mesh_fill.hip"))


@pytest.mark.parametrize("cap", [16, 32, 64])
def test_symbols_layout_defaults_and_argument_checks(cap):
    build.build_engine(cap=cap)
    lib = engine.load_library(cap=cap)
    for name in SYMBOLS:
        assert hasattr(lib, name), f"libmvskit_engine (cap {cap}) has no {name}"
        assert name in engine.EXPORTS
    F = engine.MeshFilling
    assert C.sizeof(F) == 8 and [(n, getattr(F, n).offset) for n, _ in F._fields_] == [("max_edges", 0), ("pad", 4)]
    f = F(-5, -5)
    lib.mvs_default_mesh_filling(C.byref(f))
    assert f.max_edges == 64 and f.pad == 0
    lib.mvs_default_mesh_filling(None)  # ignored

    def err(word):
        return word in lib.mvs_last_error()

    vp = C.c_void_p
    verts = np.full((8, 3), -7, np.float32)
    tris = np.full((8, 3), -7, np.int32)
    out_v = np.full((8, 3), -7, np.float32)
    out_t = np.full((8, 3), -7, np.int32)
    loop = np.full(8, -7, np.int32)
    length = np.full(8, -7, np.int32)
    words = [C.c_int64(-7) for _ in range(6)]
    nvo, nto, nfo, nlo, nco, nio = (C.byref(w) for w in words)
    vtp, trp, ovp, otp, lop, lep = (a.ctypes.data_as(vp) for a in (verts, tris, out_v, out_t, loop, length))
    big = (1 << 30) + 1
    bad_counts = ((-1, 8), (8, -1), (big, 8), (8, big))

    def fl(max_edges=64):
        return C.byref(F(max_edges, 0))

    # mvs_engine_mesh_fill: f, max_edges, the counts, verts, tris, the size pointers, the caps, the engine -- each with every later argument bad too
    g = lib.mvs_engine_mesh_fill
    assert g(None, None, -1, None, -1, None, -1, None, -1, None, None, None, None) == MVS_ERR_ARG and err(b"filling null")
    for m in (2, 0, -1, -(1 << 31)):
        assert g(None, fl(m), -1, None, -1, None, -1, None, -1, None, None, None, None) == MVS_ERR_ARG and err(b"max_edges"), m
    for nv, nt in bad_counts:
        assert g(None, fl(), nv, None, nt, None, -1, None, -1, None, None, None, None) == MVS_ERR_ARG and err(b"count"), (nv, nt)
    assert g(None, fl(), 8, None, 8, None, -1, None, -1, None, None, None, None) == MVS_ERR_ARG and err(b"verts null")
    assert g(None, fl(), 8, vtp, 8, None, -1, None, -1, None, None, None, None) == MVS_ERR_ARG and err(b"tris null")
    assert g(None, fl(), 8, vtp, 8, trp, -1, ovp, -1, otp, None, nto, nfo) == MVS_ERR_ARG and err(b"n_v or n_t null")
    assert g(None, fl(), 8, vtp, 8, trp, -1, ovp, -1, otp, nvo, None, nfo) == MVS_ERR_ARG and err(b"n_v or n_t null")
    assert g(None, fl(), 8, vtp, 8, trp, -1, ovp, 8, otp, nvo, nto, nfo) == MVS_ERR_ARG and err(b"negative cap")
    assert g(None, fl(), 8, vtp, 8, trp, 8, ovp, -1, otp, nvo, nto, nfo) == MVS_ERR_ARG and err(b"negative cap")
    assert g(None, fl(), 8, vtp, 8, trp, 8, ovp, 8, otp, nvo, nto, nfo) == MVS_ERR_ARG and err(b"no engine")
    # n_filled may be null; the ends of the ranges that are allowed
    assert g(None, fl(3), 8, vtp, 8, trp, 8, ovp, 8, otp, nvo, nto, None) == MVS_ERR_ARG and err(b"no engine")
    assert g(None, fl((1 << 31) - 1), 0, None, 0, None, 0, None, 0, None, nvo, nto, None) == MVS_ERR_ARG and err(b"no engine")
    assert g(None, fl(), 1 << 30, vtp, 1 << 30, trp, 0, None, 0, None, nvo, nto, nfo) == MVS_ERR_ARG and err(b"no engine")

    # mvs_engine_mesh_boundaries: the counts, tris, the engine
    h = lib.mvs_engine_mesh_boundaries
    for nv, nt in bad_counts:
        assert h(None, nv, nt, None, lop, lep, nlo, nco, nio) == MVS_ERR_ARG and err(b"count"), (nv, nt)
    assert h(None, 8, 8, None, lop, lep, nlo, nco, nio) == MVS_ERR_ARG and err(b"tris null")
    assert h(None, 8, 8, trp, lop, lep, nlo, nco, nio) == MVS_ERR_ARG and err(b"no engine")
    assert h(None, 1 << 30, 0, None, None, None, None, None, None) == MVS_ERR_ARG and err(b"no engine")

    # nothing was written on any refused call
    for a in (verts, tris, out_v, out_t, loop, length):
        assert (a == -7).all()
    assert [w.value for w in words] == [-7] * 6
