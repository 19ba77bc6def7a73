"""CPU-side checks of the seam entry points (include/mvskit_seams.h: mvs_mesh_seams, mvs_default_mesh_seams, mvs_engine_mesh_adjacency,
mvs_engine_mesh_face_quality, mvs_engine_mesh_smooth_labels, mvs_engine_mesh_seam_levels, mvs_engine_mesh_texture_levelled): the header
against the binding's table as tests/test_mesh_texture_abi.py holds mvskit_texture.h, every engine library exports them, the struct is 16
bytes with the header's offsets and defaults, bad arguments are refused in the header's order before the handle is read or a device is
touched, with nothing written through an output pointer; the Python surface."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from mvskit_amd import abi, build, engine
from mvskit_amd.engine import MVS_ERR_ARG
from test_device_headers import PATCH_SIDE, _closure

SYMBOLS = ("mvs_default_mesh_seams", "mvs_engine_mesh_adjacency", "mvs_engine_mesh_face_quality", "mvs_engine_mesh_smooth_labels",
           "mvs_engine_mesh_seam_levels", "mvs_engine_mesh_texture_levelled")
HEADER = os.path.join(build.ROOT, "include", "mvskit_seams.h")


def _header():
    """the header without its comments"""
    return re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)


def test_header_declares_them_and_the_older_lists_point_here():
    text = open(HEADER).read()
    for name in SYMBOLS:
        assert name + "(" in text, name
    for word in ("ADMISSIBLE", "PROPOSAL", "MOVERS", "SEAM EDGE", "OFFSETS", "LIMITS", "WHAT THESE CALLS DO NOT DO", "graph cuts", "Poisson", "chart packing",
                 "masks", "sharded", '#include "mvskit_texture.h"'):
        assert word in text, word
    texture = open(os.path.join(build.ROOT, "include", "mvskit_texture.h")).read().split("WHAT THE TEXTURING DOES NOT DO")[1]
    assert "seam-aware" in texture and "levelling" in texture and texture.count("(since f-14: mvskit_seams.h)") == 2
    design = open(os.path.join(build.ROOT, "DESIGN.md")).read()
    assert "f-14" in design and "mvskit_seams.h" in design


def test_binding_table_matches_the_header():
    assert re.findall(r"\b(mvs_[a-z_]+)\s*\(", open(HEADER).read().split("#ifndef MVSKIT_SEAMS_H")[1]) == list(abi.SEAM_SIGNATURES) == list(SYMBOLS)
    protos = re.findall(r"\b(int|void)\s+(mvs_\w+)\s*\(([^()]*)\)\s*;", _header())
    assert [name for _, name, _ in protos] == list(abi.SEAM_SIGNATURES)
    assert not set(abi.SEAM_SIGNATURES) & (set(abi.SIGNATURES) | set(abi.TEXTURE_SIGNATURES))
    scalars = {"int": C.c_int, "int64_t": C.c_int64, "float": C.c_float}
    pointees = {**scalars, **abi.TEXTURE_STRUCTS, **abi.SEAM_STRUCTS, "mvs_engine*": C.c_void_p}
    for ret, name, params in protos:
        restype, argtypes = abi.SEAM_SIGNATURES[name]
        assert restype is {"int": C.c_int, "void": None}[ret], name
        params = [" ".join(p.split()) for p in params.split(",")]
        assert len(params) == len(argtypes), name
        for k, (p, t) in enumerate(zip(params, argtypes)):
            where = f"{name}, parameter {k} ({p})"
            if "*" in p:
                if isinstance(t, type) and issubclass(t, C._Pointer):
                    pointee = p.replace("const ", "")
                    pointee = pointee[:pointee.rindex("*")].strip()
                    assert pointee in pointees and t._type_ is pointees[pointee], where
                else:
                    assert t is C.c_void_p, where
            else:
                ctype, _ = p.rsplit(" ", 1)
                assert ctype in scalars and t is scalars[ctype], where
    structs = re.findall(r"typedef\s+struct\s+(mvs_\w+)\s*\{(.*?)\}\s*\1\s*;", _header(), re.S)
    assert [n for n, _ in structs] == list(abi.SEAM_STRUCTS)
    fields = [d.split()[-1] for d in structs[0][1].split(";") if d.strip()]
    assert fields == [n for n, _ in engine.MeshSeams._fields_] == ["keep", "iterations", "max_shift", "samples"]
    assert all(d.split()[0] == "int32_t" for d in structs[0][1].split(";") if d.strip())


def test_the_new_file_is_a_source_of_the_build_and_stays_off_the_patch_side():
    assert "mvs_mesh_seams.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "mvs_mesh_seams.hip"))
    assert HEADER in build.DEPS
    reached = _closure("mvs_mesh_seams.hip")
    assert not reached & PATCH_SIDE, sorted(reached & PATCH_SIDE)
    assert reached <= {"mvs_mesh_common.cuh", "mvs_common.cuh", "mvs_wave.cuh", "mvs_camera.cuh", "mvs_math.cuh", "mvs_kernels.h", "mvs_types.h"}, sorted(reached)


def test_the_python_surface():
    E = engine.Engine
    p = inspect.signature(E.mesh_adjacency).parameters
    assert list(p) == ["self", "n_v", "tris"]
    p = inspect.signature(E.mesh_face_quality).parameters
    assert list(p) == ["self", "verts", "tris", "visible", "front_only"] and p["visible"].default is None and p["front_only"].default is True
    p = inspect.signature(E.smooth_face_views).parameters
    assert list(p) == ["self", "tris", "quality", "label", "keep", "iterations"] and (p["keep"].default, p["iterations"].default) == (192, 64)
    p = inspect.signature(E.seam_levels).parameters
    assert list(p) == ["self", "verts", "tris", "label", "max_shift", "samples"] and (p["max_shift"].default, p["samples"].default) == (32, 4)
    p = inspect.signature(E.texture_mesh_levelled).parameters
    assert list(p) == ["self", "verts", "tris", "label", "offset", "res", "width"] and (p["res"].default, p["width"].default) == (8, 4096)
    p = inspect.signature(E.textured_mesh).parameters
    assert p["seam_keep"].default == 0 and p["level_colours"].default is False


@pytest.mark.parametrize("cap", [16, 32, 64])
def test_symbols_layout_defaults_and_argument_checks(cap):
    build.build_engine(cap=cap)
    lib = engine.load_library(cap=cap)
    for name in SYMBOLS:
        assert hasattr(lib, name), f"libmvskit_engine (cap {cap}) has no {name}"
        fn = getattr(lib, name)
        assert (fn.restype, fn.argtypes) == abi.SEAM_SIGNATURES[name]
    S, X = engine.MeshSeams, engine.MeshTexturing
    assert C.sizeof(S) == 16 and [(n, getattr(S, n).offset) for n, _ in S._fields_] == [("keep", 0), ("iterations", 4), ("max_shift", 8), ("samples", 12)]
    s = S(-7, -7, -7, -7)
    lib.mvs_default_mesh_seams(C.byref(s))
    assert (s.keep, s.iterations, s.max_shift, s.samples) == (192, 64, 32, 4)
    lib.mvs_default_mesh_seams(None)

    def err(word):
        return word in lib.mvs_last_error()

    vp = C.c_void_p
    verts = np.full((8, 3), -7, np.float32)
    tris = np.full((8, 3), -7, np.int32)
    label = np.full(8, -7, np.int32)
    out = np.full(8, -7, np.int32)
    nbr = np.full((8, 3), -7, np.int32)
    quality = np.full((8, 3), 7, np.uint8)
    stats = np.full(4, -7, np.int64)
    offset = np.full((3, 3), -7, np.int32)
    pairs = np.full((3, 3, 4), -7, np.int64)
    visible = np.full(8, 7, np.uint64)
    rgb = np.full((64, 64, 3), 7, np.uint8)
    uv = np.full((8, 3, 2), -7, np.int32)
    nirr, nedges, height, ntex = C.c_int64(-7), C.c_int64(-7), C.c_int64(-7), C.c_int64(-7)
    vtp, trp, lbp, oup, nbp, qup, stp, ofp, pap, vip, rgp, uvp = (a.ctypes.data_as(vp) for a in (verts, tris, label, out, nbr, quality, stats, offset, pairs, visible,
                                                                                                 rgb, uv))
    big = (1 << 30) + 1
    ok, sk = C.byref(X(8, 64, 1, 0)), C.byref(S(192, 64, 32, 4))
    adj, qual, smooth, levels, tex = (lib.mvs_engine_mesh_adjacency, lib.mvs_engine_mesh_face_quality, lib.mvs_engine_mesh_smooth_labels,
                                      lib.mvs_engine_mesh_seam_levels, lib.mvs_engine_mesh_texture_levelled)

    # adjacency: counts, tris, nbr, engine
    for nv, nt in ((-1, 8), (8, -1), (big, 8), (8, big)):
        assert adj(None, nv, nt, None, None, None) == MVS_ERR_ARG and err(b"count"), (nv, nt)
    assert adj(None, 8, 8, None, None, None) == MVS_ERR_ARG and err(b"tris null")
    assert adj(None, 8, 8, trp, None, C.byref(nirr)) == MVS_ERR_ARG and err(b"nbr null")
    assert adj(None, 8, 8, trp, nbp, C.byref(nirr)) == MVS_ERR_ARG and err(b"no engine")
    assert adj(None, 0, 0, None, None, None) == MVS_ERR_ARG and err(b"no engine")

    # face_quality: the texturing struct as in mvskit_texture.h, counts, verts, tris, quality, engine
    assert qual(None, None, -1, None, -1, None, None, None) == MVS_ERR_ARG and err(b"texturing null")
    assert qual(None, C.byref(X(0, 1, 1, 0)), -1, None, -1, None, None, None) == MVS_ERR_ARG and err(b"res outside")
    assert qual(None, C.byref(X(8, 10, 1, 0)), -1, None, -1, None, None, None) == MVS_ERR_ARG and err(b"width outside")
    assert qual(None, ok, -1, None, 8, None, None, None) == MVS_ERR_ARG and err(b"count")
    assert qual(None, ok, 8, None, 8, None, None, None) == MVS_ERR_ARG and err(b"verts null")
    assert qual(None, ok, 8, vtp, 8, None, None, None) == MVS_ERR_ARG and err(b"tris null")
    assert qual(None, ok, 8, vtp, 8, trp, vip, None) == MVS_ERR_ARG and err(b"quality null")
    assert qual(None, ok, 8, vtp, 8, trp, vip, qup) == MVS_ERR_ARG and err(b"no engine")
    assert qual(None, ok, 0, None, 0, None, None, None) == MVS_ERR_ARG and err(b"no engine")

    # smooth_labels: the struct and its four ranges, counts, tris, nviews_q, quality, label_in, label_out, stats, engine
    assert smooth(None, None, -1, -1, None, 0, None, None, None, None) == MVS_ERR_ARG and err(b"seams null")
    for bad, word in (((0, 64, 32, 4), b"keep outside"), ((256, 64, 32, 4), b"keep outside"), ((192, -1, 32, 4), b"iterations outside"),
                      ((192, 4097, 32, 4), b"iterations outside"), ((192, 64, -1, 4), b"max_shift outside"), ((192, 64, 256, 4), b"max_shift outside"),
                      ((192, 64, 32, 0), b"samples outside"), ((192, 64, 32, 17), b"samples outside")):
        assert smooth(None, C.byref(S(*bad)), -1, -1, None, 0, None, None, None, None) == MVS_ERR_ARG and err(word), bad
        assert levels(None, C.byref(S(*bad)), C.byref(X(0, 1, 1, 0)), -1, None, -1, None, None, None, None, None) == MVS_ERR_ARG and err(word), bad
    for nv, nt in ((-1, 8), (8, -1), (big, 8), (8, big)):
        assert smooth(None, sk, nv, nt, None, 0, None, None, None, None) == MVS_ERR_ARG and err(b"count"), (nv, nt)
    assert smooth(None, sk, 8, 8, None, 0, None, None, None, None) == MVS_ERR_ARG and err(b"tris null")
    for nq in (0, -1, 65):
        assert smooth(None, sk, 8, 8, trp, nq, None, None, None, None) == MVS_ERR_ARG and err(b"nviews_q outside"), nq
    assert smooth(None, sk, 8, 8, trp, 3, None, None, None, None) == MVS_ERR_ARG and err(b"quality null")
    assert smooth(None, sk, 8, 8, trp, 3, qup, None, oup, stp) == MVS_ERR_ARG and err(b"label_in null")
    assert smooth(None, sk, 8, 8, trp, 3, qup, lbp, None, stp) == MVS_ERR_ARG and err(b"label_out null")
    assert smooth(None, sk, 8, 8, trp, 3, qup, lbp, oup, None) == MVS_ERR_ARG and err(b"stats null")
    assert smooth(None, sk, 8, 8, trp, 3, qup, lbp, oup, stp) == MVS_ERR_ARG and err(b"no engine")
    for ends in ((1, 0, 0, 1), (255, 4096, 255, 16)):
        assert smooth(None, C.byref(S(*ends)), 1 << 30, 1 << 30, trp, 64, qup, lbp, oup, stp) == MVS_ERR_ARG and err(b"no engine"), ends

    # seam_levels: seams, texturing, the ranges of both, the mesh, label, offset, pairs, engine
    assert levels(None, None, None, -1, None, -1, None, None, None, None, None) == MVS_ERR_ARG and err(b"seams null")
    assert levels(None, sk, None, -1, None, -1, None, None, None, None, None) == MVS_ERR_ARG and err(b"texturing null")
    assert levels(None, sk, C.byref(X(0, 1, 1, 0)), -1, None, -1, None, None, None, None, None) == MVS_ERR_ARG and err(b"res outside")
    assert levels(None, sk, C.byref(X(8, 10, 1, 0)), -1, None, -1, None, None, None, None, None) == MVS_ERR_ARG and err(b"width outside")
    assert levels(None, sk, ok, 8, None, big, None, None, None, None, None) == MVS_ERR_ARG and err(b"count")
    assert levels(None, sk, ok, 8, None, 8, None, None, None, None, None) == MVS_ERR_ARG and err(b"verts null")
    assert levels(None, sk, ok, 8, vtp, 8, None, None, None, None, None) == MVS_ERR_ARG and err(b"tris null")
    assert levels(None, sk, ok, 8, vtp, 8, trp, None, None, None, None) == MVS_ERR_ARG and err(b"label null")
    assert levels(None, sk, ok, 8, vtp, 8, trp, lbp, None, pap, C.byref(nedges)) == MVS_ERR_ARG and err(b"offset null")
    assert levels(None, sk, ok, 8, vtp, 8, trp, lbp, ofp, None, C.byref(nedges)) == MVS_ERR_ARG and err(b"pairs null")
    assert levels(None, sk, ok, 8, vtp, 8, trp, lbp, ofp, pap, C.byref(nedges)) == MVS_ERR_ARG and err(b"no engine")
    assert levels(None, sk, ok, 0, None, 0, None, None, ofp, pap, None) == MVS_ERR_ARG and err(b"no engine")

    # texture_levelled: mvs_engine_mesh_texture's order, offset optional
    hp, np_ = C.byref(height), C.byref(ntex)
    assert tex(None, None, -1, None, -1, None, None, None, -1, None, None, None, None) == MVS_ERR_ARG and err(b"texturing null")
    assert tex(None, C.byref(X(257, 1, 1, 0)), -1, None, -1, None, None, None, -1, None, None, None, None) == MVS_ERR_ARG and err(b"res outside")
    assert tex(None, C.byref(X(8, 32769, 1, 0)), -1, None, -1, None, None, None, -1, None, None, None, None) == MVS_ERR_ARG and err(b"width outside")
    assert tex(None, ok, 8, None, -1, None, None, None, -1, None, None, None, None) == MVS_ERR_ARG and err(b"count")
    assert tex(None, ok, 8, None, 8, None, None, None, -1, None, None, None, None) == MVS_ERR_ARG and err(b"verts null")
    assert tex(None, ok, 8, vtp, 8, None, None, None, -1, None, None, None, None) == MVS_ERR_ARG and err(b"tris null")
    assert tex(None, ok, 8, vtp, 8, trp, None, ofp, -1, rgp, uvp, None, None) == MVS_ERR_ARG and err(b"label null")
    assert tex(None, ok, 8, vtp, 8, trp, lbp, ofp, -1, rgp, uvp, None, np_) == MVS_ERR_ARG and err(b"height or n_textured null")
    assert tex(None, ok, 8, vtp, 8, trp, lbp, ofp, -1, rgp, uvp, hp, None) == MVS_ERR_ARG and err(b"height or n_textured null")
    assert tex(None, ok, 8, vtp, 8, trp, lbp, ofp, -1, rgp, uvp, hp, np_) == MVS_ERR_ARG and err(b"negative cap_h")
    assert tex(None, ok, 8, vtp, 8, trp, lbp, ofp, 64, rgp, uvp, hp, np_) == MVS_ERR_ARG and err(b"no engine")
    assert tex(None, ok, 8, vtp, 8, trp, lbp, None, 64, rgp, uvp, hp, np_) == MVS_ERR_ARG and err(b"no engine")
    for name in (b"mvs_engine_mesh_texture_levelled",):
        assert name in lib.mvs_last_error()

    # nothing was written on any refused call
    for a in (verts, tris, label, out, nbr, stats, offset, pairs, uv):
        assert (a == -7).all()
    assert (quality == 7).all() and (visible == 7).all() and (rgb == 7).all()
    assert (nirr.value, nedges.value, height.value, ntex.value) == (-7, -7, -7, -7)
