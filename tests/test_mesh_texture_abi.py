"""CPU-side checks of the textured-mesh entry points (include/mvskit_texture.h: mvs_mesh_texturing, mvs_default_mesh_texturing,
mvs_engine_mesh_face_views, mvs_engine_mesh_texture): the header against the binding's table as tests/test_abi.py holds
mvskit_engine.h, every engine library exports them, the struct is 16 bytes with the header's offsets, bad arguments are refused in the
header's order before the handle is read or a device is touched, with nothing written through an output pointer; the Python surface;
and write_mesh_obj's OBJ, MTL and PNG read back."""
import ctypes as C
import inspect
import os
import re
import struct
import zlib

import numpy as np
import pytest

from mvskit_amd import abi, build, engine
from mvskit_amd.engine import MVS_ERR_ARG
from test_device_headers import PATCH_SIDE, _closure

SYMBOLS = ("mvs_default_mesh_texturing", "mvs_engine_mesh_face_views", "mvs_engine_mesh_texture")
HEADER = os.path.join(build.ROOT, "include", "mvskit_texture.h")


def _header():
    """the header without its comments"""
    return re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)


def test_header_declares_them_and_says_what_it_does_not_do():
    text = open(HEADER).read()
    for name in SYMBOLS:
        assert name + "(" in text, name
    for word in ("CANDIDATE", "HONOURED", "UNTEXTURED", "LAYOUT", "SIZE CALL", "OWNERSHIP", "TEXEL", "f_v = -sign(det M)", "WHAT THE TEXTURING DOES NOT DO",
                 "seam-aware", "levelling", "chart packing", "level-0 texels", "masks", "per-pixel occlusion", "sharded"):
        assert word in text, word
    # the render's list points here, and keeps its own words
    render = open(os.path.join(build.ROOT, "include", "mvskit_engine.h")).read()
    assert "mvskit_texture.h" in render and "WHAT THE RENDER DOES NOT DO" in render and "texture" in render.split("WHAT THE RENDER DOES NOT DO")[1][:400]


def test_binding_table_matches_the_header():
    """tests/test_abi.py's check of SIGNATURES, on this header and TEXTURE_SIGNATURES: the same names in the same order, at every
    position the ctypes class of the C type"""
    assert re.findall(r"\b(mvs_[a-z_]+)\s*\(", open(HEADER).read().split("#ifndef MVSKIT_TEXTURE_H")[1]) == list(abi.TEXTURE_SIGNATURES) == list(SYMBOLS)
    protos = re.findall(r"\b(int|void)\s+(mvs_\w+)\s*\(([^()]*)\)\s*;", _header())
    assert [name for _, name, _ in protos] == list(abi.TEXTURE_SIGNATURES)
    assert not set(abi.TEXTURE_SIGNATURES) & set(abi.SIGNATURES)
    scalars = {"int": C.c_int, "int64_t": C.c_int64, "float": C.c_float}
    pointees = {**scalars, **abi.TEXTURE_STRUCTS, "mvs_engine*": C.c_void_p}
    for ret, name, params in protos:
        restype, argtypes = abi.TEXTURE_SIGNATURES[name]
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
    assert [n for n, _ in structs] == list(abi.TEXTURE_STRUCTS)
    fields = [d.split()[-1] for d in structs[0][1].split(";") if d.strip()]
    assert fields == [n for n, _ in engine.MeshTexturing._fields_] == ["res", "width", "front_only", "pad"]
    assert all(d.split()[0] == "int32_t" for d in structs[0][1].split(";") if d.strip())


def test_the_new_file_is_a_source_of_the_build_and_stays_off_the_patch_side():
    assert "mvs_mesh_texture.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "mvs_mesh_texture.hip"))
    assert HEADER in build.DEPS
    reached = _closure("mvs_mesh_texture.hip")
    assert not reached & PATCH_SIDE, sorted(reached & PATCH_SIDE)
    assert reached <= {"mvs_mesh_common.cuh", "mvs_common.cuh", "mvs_wave.cuh", "mvs_camera.cuh", "mvs_math.cuh", "mvs_kernels.h", "mvs_types.h"}, sorted(reached)


def test_the_python_surface():
    E = engine.Engine
    for name in ("mesh_face_views", "texture_mesh", "textured_mesh"):
        assert callable(getattr(E, name)), name
    p = inspect.signature(E.mesh_face_views).parameters
    assert list(p) == ["self", "verts", "tris", "visible", "front_only"] and p["visible"].default is None and p["front_only"].default is True
    p = inspect.signature(E.texture_mesh).parameters
    assert list(p) == ["self", "verts", "tris", "label", "res", "width"] and p["res"].default == 8 and p["width"].default == 4096
    p = inspect.signature(E.textured_mesh).parameters
    assert (p["res"].default, p["atlas_width"].default, p["front_only"].default, p["visibility_tol"].default) == (8, 4096, True, 0.01)
    # coloured_mesh's mesh and clean-up arguments, with its defaults
    c = inspect.signature(E.coloured_mesh).parameters
    for name in ("volume", "source", "min_consistent", "depth_tol", "normal_cos", "cap_v", "cap_t", "min_triangles", "largest_only", "smooth_iterations",
                 "decimate_cell", "decimate_placement", "fill_max_edges"):
        assert p[name].default == c[name].default, name
    assert list(inspect.signature(engine.write_mesh_obj).parameters) == ["path", "verts", "tris", "atlas", "uv", "normals"]
    assert inspect.signature(engine.write_mesh_obj).parameters["normals"].default is None


@pytest.mark.parametrize("cap", [16, 32, 64])
def test_symbols_layout_defaults_and_argument_checks(cap):
    build.build_engine(cap=cap)
    lib = engine.load_library(cap=cap)
    for name in SYMBOLS:
        assert hasattr(lib, name), f"libmvskit_engine (cap {cap}) has no {name}"
        fn = getattr(lib, name)
        assert (fn.restype, fn.argtypes) == abi.TEXTURE_SIGNATURES[name]
    X = engine.MeshTexturing
    assert C.sizeof(X) == 16 and [(n, getattr(X, n).offset) for n, _ in X._fields_] == [("res", 0), ("width", 4), ("front_only", 8), ("pad", 12)]
    x = X(-7, -7, -7, -7)
    lib.mvs_default_mesh_texturing(C.byref(x))
    assert (x.res, x.width, x.front_only, x.pad) == (8, 4096, 1, 0)
    lib.mvs_default_mesh_texturing(None)

    def err(word):
        return word in lib.mvs_last_error()

    vp = C.c_void_p
    verts = np.full((8, 3), -7, np.float32)
    tris = np.full((8, 3), -7, np.int32)
    label = np.full(8, -7, np.int32)
    area = np.full(8, -7, np.int64)
    faces = np.full(3, -7, np.int64)
    visible = np.full(8, 7, np.uint64)
    rgb = np.full((64, 64, 3), 7, np.uint8)
    uv = np.full((8, 3, 2), -7, np.int32)
    height, ntex = C.c_int64(-7), C.c_int64(-7)
    vtp, trp, lbp, arp, fcp, vip, rgp, uvp = (a.ctypes.data_as(vp) for a in (verts, tris, label, area, faces, visible, rgb, uv))
    hp, np_ = C.byref(height), C.byref(ntex)
    big = (1 << 30) + 1
    ok = C.byref(X(8, 64, 1, 0))

    f = lib.mvs_engine_mesh_face_views
    g = lib.mvs_engine_mesh_texture
    # 1 the struct, with every later argument bad too
    assert f(None, None, -1, None, -1, None, None, None, None, None) == MVS_ERR_ARG and err(b"texturing null")
    assert g(None, None, -1, None, -1, None, None, -1, None, None, None, None) == MVS_ERR_ARG and err(b"texturing null")
    # 2 res, 3 width
    for res in (0, -1, 257):
        assert f(None, C.byref(X(res, 1, 1, 0)), -1, None, -1, None, None, None, None, None) == MVS_ERR_ARG and err(b"res outside"), res
        assert g(None, C.byref(X(res, 1, 1, 0)), -1, None, -1, None, None, -1, None, None, None, None) == MVS_ERR_ARG and err(b"res outside"), res
    for res, width in ((8, 10), (1, 3), (256, 258), (8, 32769), (8, -1)):
        assert f(None, C.byref(X(res, width, 1, 0)), -1, None, -1, None, None, None, None, None) == MVS_ERR_ARG and err(b"width outside"), (res, width)
        assert g(None, C.byref(X(res, width, 1, 0)), -1, None, -1, None, None, -1, None, None, None, None) == MVS_ERR_ARG and err(b"width outside"), (res, width)
    # 4 the counts
    for nv, nt in ((-1, 8), (8, -1), (big, 8), (8, big)):
        assert f(None, ok, nv, None, nt, None, None, None, None, None) == MVS_ERR_ARG and err(b"count"), (nv, nt)
        assert g(None, ok, nv, None, nt, None, None, -1, None, None, None, None) == MVS_ERR_ARG and err(b"count"), (nv, nt)
    # 5 verts, 6 tris, 7 label
    assert f(None, ok, 8, None, 8, None, None, None, None, None) == MVS_ERR_ARG and err(b"verts null")
    assert g(None, ok, 8, None, 8, None, None, -1, None, None, None, None) == MVS_ERR_ARG and err(b"verts null")
    assert f(None, ok, 8, vtp, 8, None, None, None, None, None) == MVS_ERR_ARG and err(b"tris null")
    assert g(None, ok, 8, vtp, 8, None, None, -1, None, None, None, None) == MVS_ERR_ARG and err(b"tris null")
    assert f(None, ok, 8, vtp, 8, trp, vip, None, arp, fcp) == MVS_ERR_ARG and err(b"label null")
    assert g(None, ok, 8, vtp, 8, trp, None, -1, rgp, uvp, None, None) == MVS_ERR_ARG and err(b"label null")
    # 8 mvs_engine_mesh_texture: height, n_textured, cap_h
    assert g(None, ok, 8, vtp, 8, trp, lbp, -1, rgp, uvp, None, np_) == MVS_ERR_ARG and err(b"height or n_textured null")
    assert g(None, ok, 8, vtp, 8, trp, lbp, -1, rgp, uvp, hp, None) == MVS_ERR_ARG and err(b"height or n_textured null")
    assert g(None, ok, 8, vtp, 8, trp, lbp, -1, rgp, uvp, hp, np_) == MVS_ERR_ARG and err(b"negative cap_h")
    # 9 the engine; every optional output may be null, the ends of the allowed ranges
    assert f(None, ok, 8, vtp, 8, trp, vip, lbp, arp, fcp) == MVS_ERR_ARG and err(b"no engine")
    assert f(None, ok, 8, vtp, 8, trp, None, lbp, None, None) == MVS_ERR_ARG and err(b"no engine")
    assert f(None, ok, 0, None, 0, None, None, None, None, None) == MVS_ERR_ARG and err(b"no engine")
    assert g(None, ok, 8, vtp, 8, trp, lbp, 64, rgp, uvp, hp, np_) == MVS_ERR_ARG and err(b"no engine")
    assert g(None, ok, 0, None, 0, None, None, 0, None, None, hp, np_) == MVS_ERR_ARG and err(b"no engine")
    for res, width in ((1, 4), (256, 259), (256, 32768)):
        assert f(None, C.byref(X(res, width, 0, 0)), 1 << 30, vtp, 1 << 30, trp, None, lbp, None, None) == MVS_ERR_ARG and err(b"no engine")
        assert g(None, C.byref(X(res, width, 0, 0)), 1 << 30, vtp, 1 << 30, trp, lbp, 0, None, None, hp, np_) == MVS_ERR_ARG and err(b"no engine")

    # nothing was written on any refused call
    for a in (verts, tris, label, area, faces, uv):
        assert (a == -7).all()
    assert (visible == 7).all() and (rgb == 7).all() and height.value == -7 and ntex.value == -7


def _decode_png(data):
    """-> [H, W, 3] uint8 of an 8-bit RGB PNG whose rows all carry filter 0; every chunk's CRC checked"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(kind + body) & 0xFFFFFFFF, kind
        chunks.append((kind, body))
        pos += 12 + n
    assert chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    w, h, depth, colour, comp, filt, interlace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, filt, interlace) == (8, 2, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(b"".join(b for k, b in chunks if k == b"IDAT")), np.uint8).reshape(h, 1 + 3 * w)
    assert (raw[:, 0] == 0).all()
    return raw[:, 1:].reshape(h, w, 3)


@pytest.mark.parametrize("with_normals", [False, True])
def test_write_mesh_obj_round_trip(tmp_path, with_normals):
    rng = np.random.RandomState(4)
    verts = rng.uniform(-3, 3, (7, 3)).astype(np.float32)
    tris = np.int32([[0, 1, 2], [2, 1, 3], [4, 5, 6], [6, 0, 3]])
    normals = rng.uniform(-1, 1, (7, 3)).astype(np.float32) if with_normals else None
    Hh, Ww = 22, 37
    atlas = rng.randint(0, 256, (Hh, Ww, 3)).astype(np.uint8)
    uv = np.stack([rng.randint(0, Ww, (4, 3)), rng.randint(0, Hh, (4, 3))], axis=-1).astype(np.int32)
    uv[0] = [[0, 0], [Ww - 1, 0], [0, Hh - 1]]
    path = str(tmp_path / "mesh.obj")
    engine.write_mesh_obj(path, verts, tris, atlas, uv, normals=normals)
    assert sorted(os.listdir(tmp_path)) == ["mesh.mtl", "mesh.obj", "mesh.png"]
    assert _decode_png(open(tmp_path / "mesh.png", "rb").read()).tobytes() == atlas.tobytes()
    mtl = open(tmp_path / "mesh.mtl").read().split("\n")
    assert "newmtl mesh" in mtl and "map_Kd mesh.png" in mtl
    v, vt, vn, faces, other = [], [], [], [], []
    for line in open(path).read().splitlines():
        key, *rest = line.split()
        {"v": v, "vt": vt, "vn": vn, "f": faces}.get(key, other).append(rest)
    assert other == [["mesh.mtl"], ["mesh"]]  # mtllib, usemtl
    assert np.array(v, dtype=np.float32).tobytes() == verts.tobytes()  # %.9g holds a float32
    if with_normals:
        assert np.array(vn, dtype=np.float32).tobytes() == normals.tobytes()
    else:
        assert vn == []
    vt = np.array(vt, dtype=np.float64)
    assert vt.shape == (12, 2) and len(faces) == 4
    for t, corners in enumerate(faces):
        for k, corner in enumerate(corners):
            ids = [int(x) for x in corner.split("/")]
            assert len(ids) == (3 if with_normals else 2) and ids[0] == tris[t, k] + 1 and ids[1] == 3 * t + k + 1
            if with_normals:
                assert ids[2] == ids[0]
            u, w = vt[ids[1] - 1]
            # vt maps back to the uv texel: the centre of (column, row), v upwards
            assert int(np.floor(u * Ww)) == uv[t, k, 0] and int(np.floor((1.0 - w) * Hh)) == uv[t, k, 1]
            assert abs(u * Ww - (uv[t, k, 0] + 0.5)) < 1e-9 and abs((1.0 - w) * Hh - (uv[t, k, 1] + 0.5)) < 1e-9
    with pytest.raises(ValueError):
        engine.write_mesh_obj(path, verts, tris, atlas, uv[:3])
