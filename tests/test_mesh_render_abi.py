"""CPU-side checks of the mesh render's entry points (include/mvskit_engine.h: mvs_mesh_view_render, mvs_engine_mesh_render,
mvs_engine_mesh_render_lists, mvs_engine_mesh_visibility, mvs_engine_mesh_colours_visible): every engine library exports them, the struct is 16 bytes with the
header's offsets, and bad arguments are refused in the header's order before the handle is read or a device is touched, with nothing
written through an output pointer."""
import ctypes as C
import os

import numpy as np
import pytest

from mvskit_amd import build, engine
from mvskit_amd.engine import MVS_ERR_ARG

SYMBOLS = ("mvs_engine_mesh_render", "mvs_engine_mesh_render_lists", "mvs_engine_mesh_visibility", "mvs_engine_mesh_colours_visible")
HEADER = os.path.join(build.ROOT, "include", "mvskit_engine.h")


def test_header_declares_them():
    text = open(HEADER).read()
    for name in SYMBOLS + ("mvs_mesh_view_render",):
        assert name + "(" in text or name + ";" in text, name
    # the terms of the contract, and what the render does not do
    for word in ("VERTEX", "USABLE", "SKIPPED", "COVERAGE", "top-left", "Z-BUFFER", "NO NEAR-PLANE CLIPPING", "WHAT THE RENDER DOES NOT DO", "culling",
                 "MVS_MRENDER_SMALL"):
        assert word in text, word


def test_the_new_file_is_a_source_of_the_build():
    assert "mvs_mesh_render.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "mvs_mesh_render.hip"))
    assert "mvs_mesh_attr_colours.cuh" in build.DEPS  # the colour kernels' shared body rebuilds the library


def test_the_python_surface():
    for name in ("render_mesh", "mesh_screen", "mesh_render_lists", "mesh_visibility"):
        assert callable(getattr(engine.Engine, name)), name
    import inspect
    assert inspect.signature(engine.Engine.mesh_colours).parameters["visible"].default is None
    assert inspect.signature(engine.Engine.coloured_mesh).parameters["mesh_occlusion"].default is False
    assert inspect.signature(engine.Engine.mesh_visibility).parameters["tol"].default == 0.01


@pytest.mark.parametrize("cap", [16, 32, 64])
def test_symbols_layout_and_argument_checks(cap):
    build.build_engine(cap=cap)
    lib = engine.load_library(cap=cap)
    for name in SYMBOLS:
        assert hasattr(lib, name), f"libmvskit_engine (cap {cap}) has no {name}"
        assert name in engine.EXPORTS
    R = engine.MeshViewRender
    assert C.sizeof(R) == 16 and [(n, getattr(R, n).offset) for n, _ in R._fields_] == [("depth", 0), ("tri", 8)]

    def err(word):
        return word in lib.mvs_last_error()

    vp = C.c_void_p
    verts = np.full((8, 3), -7, np.float32)
    tris = np.full((8, 3), -7, np.int32)
    depth = np.full(64, -7, np.float32)
    tri = np.full(64, -7, np.int32)
    screen = np.full((3, 8, 2), -7, np.int32)
    vdepth = np.full((3, 8), -7, np.float32)
    ncov = np.full(3, -7, np.int64)
    nskip = np.full(3, -7, np.int64)
    visible = np.full(8, 7, np.uint64)
    rgb = np.full((8, 3), 7, np.uint8)
    used = np.full(8, 7, np.uint8)
    vtp, trp, scp, vdp, ncp, nsp, vip, rgp, usp = (a.ctypes.data_as(vp) for a in (verts, tris, screen, vdepth, ncov, nskip, visible, rgb, used))
    slots = (R * 3)()
    for s in slots:
        s.depth, s.tri = depth.ctypes.data, tri.ctypes.data
    big = (1 << 30) + 1
    bad_counts = ((-1, 8), (8, -1), (big, 8), (8, big))

    # mvs_engine_mesh_render: the counts, verts, tris, the engine -- each with every later argument bad too
    g = lib.mvs_engine_mesh_render
    for nv, nt in bad_counts:
        assert g(None, nv, None, nt, None, slots, scp, vdp, ncp, nsp) == MVS_ERR_ARG and err(b"count"), (nv, nt)
    assert g(None, 8, None, 8, None, slots, scp, vdp, ncp, nsp) == MVS_ERR_ARG and err(b"verts null")
    assert g(None, 8, vtp, 8, None, slots, scp, vdp, ncp, nsp) == MVS_ERR_ARG and err(b"tris null")
    assert g(None, 8, vtp, 8, trp, slots, scp, vdp, ncp, nsp) == MVS_ERR_ARG and err(b"no engine")
    # every output may be null; the ends of the ranges that are allowed
    assert g(None, 8, vtp, 8, trp, None, None, None, None, None) == MVS_ERR_ARG and err(b"no engine")
    assert g(None, 0, None, 0, None, slots, scp, vdp, ncp, nsp) == MVS_ERR_ARG and err(b"no engine")
    assert g(None, 1 << 30, vtp, 1 << 30, trp, None, None, None, None, None) == MVS_ERR_ARG and err(b"no engine")

    # mvs_engine_mesh_render_lists: the counts, verts, tris, n_listed, the engine
    q = lib.mvs_engine_mesh_render_lists
    for nv, nt in bad_counts:
        assert q(None, nv, None, nt, None, None) == MVS_ERR_ARG and err(b"count"), (nv, nt)
    assert q(None, 8, None, 8, None, None) == MVS_ERR_ARG and err(b"verts null")
    assert q(None, 8, vtp, 8, None, None) == MVS_ERR_ARG and err(b"tris null")
    assert q(None, 8, vtp, 8, trp, None) == MVS_ERR_ARG and err(b"n_listed null")
    assert q(None, 8, vtp, 8, trp, ncp) == MVS_ERR_ARG and err(b"no engine")
    assert q(None, 0, None, 0, None, ncp) == MVS_ERR_ARG and err(b"no engine")

    # mvs_engine_mesh_visibility: tol, the counts, verts, tris, visible, the engine
    h = lib.mvs_engine_mesh_visibility
    for tol in (-1e-6, -1.0, float("nan"), float("inf"), float("-inf")):
        assert h(None, tol, -1, None, -1, None, None) == MVS_ERR_ARG and err(b"tol"), tol
    for nv, nt in bad_counts:
        assert h(None, 0.0, nv, None, nt, None, None) == MVS_ERR_ARG and err(b"count"), (nv, nt)
    assert h(None, 0.0, 8, None, 8, None, None) == MVS_ERR_ARG and err(b"verts null")
    assert h(None, 0.0, 8, vtp, 8, None, None) == MVS_ERR_ARG and err(b"tris null")
    assert h(None, 0.0, 8, vtp, 8, trp, None) == MVS_ERR_ARG and err(b"visible null")
    assert h(None, 0.0, 8, vtp, 8, trp, vip) == MVS_ERR_ARG and err(b"no engine")
    assert h(None, 0.01, 0, None, 0, None, None) == MVS_ERR_ARG and err(b"no engine")
    assert h(None, 3.0e38, 8, vtp, 0, None, vip) == MVS_ERR_ARG and err(b"no engine")

    # mvs_engine_mesh_colours_visible: the checks of mvs_engine_mesh_colours, under its own name, whether or not there is a visibility
    k = lib.mvs_engine_mesh_colours_visible
    c = engine.MapsConfig()
    lib.mvs_default_maps_config(C.byref(c))
    m = engine.MeshColouring(0.01, 0.1)
    for vis in (None, vip):
        assert k(None, None, C.byref(m), 8, vtp, None, vis, rgp, usp) == MVS_ERR_ARG and err(b"mvs_engine_mesh_colours_visible")
        assert k(None, C.byref(c), None, 8, vtp, None, vis, rgp, usp) == MVS_ERR_ARG and err(b"colouring null")
        assert k(None, C.byref(c), C.byref(engine.MeshColouring(0.0, 0.1)), 8, vtp, None, vis, rgp, usp) == MVS_ERR_ARG and err(b"occl_tol")
        assert k(None, C.byref(c), C.byref(m), -1, vtp, None, vis, rgp, usp) == MVS_ERR_ARG and err(b"n_v")
        assert k(None, C.byref(c), C.byref(m), 8, None, None, vis, rgp, usp) == MVS_ERR_ARG and err(b"verts or rgb null")
        assert k(None, C.byref(c), C.byref(m), 8, vtp, None, vis, rgp, usp) == MVS_ERR_ARG and err(b"no engine")

    # nothing was written on any refused call
    for a in (verts, tris, depth, tri, screen, vdepth, ncov, nskip):
        assert (a == -7).all()
    for a in (visible, rgb, used):
        assert (a == 7).all()
