"""CPU-side checks of the mesh attribute entry points (include/mvskit_engine.h: mvs_mesh_colouring, mvs_engine_mesh_normals,
mvs_engine_mesh_colours): every engine library exports them, the struct is 8 bytes, bad arguments are refused in the header's order
before the handle is read or a device is touched, with nothing written through an output pointer; and write_mesh_ply's two new
arguments."""
import ctypes as C
import os

import numpy as np
import pytest

from mvskit_amd import build, engine
from mvskit_amd.engine import MVS_ERR_ARG

SYMBOLS = ("mvs_default_mesh_colouring", "mvs_engine_mesh_normals", "mvs_engine_mesh_colours")
HEADER = os.path.join(build.ROOT, "include", "mvskit_engine.h")


def test_header_declares_them():
    text = open(HEADER).read()
    for name in SYMBOLS + ("mvs_mesh_colouring",):
        assert name + "(" in text or name + ";" in text, name
    assert "VANISHES" in text  # the vanishing rule is part of the normals contract


@pytest.mark.parametrize("cap", [16, 32, 64])
def test_symbols_layout_defaults_and_argument_checks(cap):
    build.build_engine(cap=cap)
    lib = engine.load_library(cap=cap)
    for name in SYMBOLS:
        assert hasattr(lib, name), f"libmvskit_engine (cap {cap}) has no {name}"
        assert name in engine.EXPORTS
    M = engine.MeshColouring
    assert C.sizeof(M) == 8 and [(n, getattr(M, n).offset) for n, _ in M._fields_] == [("occl_tol", 0), ("min_cos", 4)]
    d = M(-1.0, -1.0)
    lib.mvs_default_mesh_colouring(C.byref(d))
    assert d.occl_tol == np.float32(0.01) and d.min_cos == np.float32(0.1)
    lib.mvs_default_mesh_colouring(None)  # ignored

    def err(word):
        return word in lib.mvs_last_error()

    vp = C.c_void_p
    verts = np.full((8, 3), -7, np.float32)
    tris = np.full((8, 3), -7, np.int32)
    normals = np.full((8, 3), -7, np.float32)
    rgb = np.full((8, 3), 249, np.uint8)
    used = np.full(8, 249, np.uint8)
    vtp, trp, nmp, rgp, usp = (a.ctypes.data_as(vp) for a in (verts, tris, normals, rgb, used))

    # mvs_engine_mesh_normals: the counts, verts, tris, normals, the engine
    f = lib.mvs_engine_mesh_normals
    big = (1 << 30) + 1
    for nv, nt in ((-1, 8), (8, -1), (big, 8), (8, big)):
        assert f(None, nv, None, nt, None, None) == MVS_ERR_ARG and err(b"count"), (nv, nt)
    assert f(None, 8, None, 8, None, None) == MVS_ERR_ARG and err(b"verts null")
    assert f(None, 8, vtp, 8, None, None) == MVS_ERR_ARG and err(b"tris null")
    assert f(None, 8, vtp, 8, trp, None) == MVS_ERR_ARG and err(b"normals null")
    assert f(None, 8, vtp, 8, trp, nmp) == MVS_ERR_ARG and err(b"no engine")
    assert f(None, 0, None, 0, None, None) == MVS_ERR_ARG and err(b"no engine")  # null pointers are fine with zero counts
    assert f(None, 8, vtp, 0, None, nmp) == MVS_ERR_ARG and err(b"no engine")
    assert f(None, 1 << 30, vtp, 1 << 30, trp, nmp) == MVS_ERR_ARG and err(b"no engine")  # the limit itself is allowed

    def cfg(**kw):
        c = engine.MapsConfig()
        lib.mvs_default_maps_config(C.byref(c))
        for k, v in kw.items():
            setattr(c, k, v)
        return C.byref(c)

    def col(occl_tol=0.01, min_cos=0.1):
        return C.byref(M(occl_tol, min_cos))

    # mvs_engine_mesh_colours: the maps ladder, the colouring, n_v, verts / rgb, the engine -- each with every later argument bad too
    g = lib.mvs_engine_mesh_colours
    nan, inf = float("nan"), float("inf")
    assert g(None, None, None, -1, None, None, None, None) == MVS_ERR_ARG and err(b"config null")
    assert g(None, cfg(source=2, min_consistent=-1), None, -1, None, None, None, None) == MVS_ERR_ARG and err(b"source")
    assert g(None, cfg(min_consistent=-1, depth_tol=0.0), None, -1, None, None, None, None) == MVS_ERR_ARG and err(b"min_consistent")
    assert g(None, cfg(depth_tol=0.0, normal_cos=2.0), None, -1, None, None, None, None) == MVS_ERR_ARG and err(b"depth_tol")
    assert g(None, cfg(normal_cos=2.0), None, -1, None, None, None, None) == MVS_ERR_ARG and err(b"normal_cos")
    assert g(None, cfg(), None, -1, None, None, None, None) == MVS_ERR_ARG and err(b"colouring null")
    for x in (0.0, -1.0, nan, inf):
        assert g(None, cfg(), col(occl_tol=x, min_cos=nan), -1, None, None, None, None) == MVS_ERR_ARG and err(b"occl_tol"), x
    for x in (nan, inf, -1.5, 1.5):
        assert g(None, cfg(), col(min_cos=x), -1, None, None, None, None) == MVS_ERR_ARG and err(b"min_cos"), x
    for n in (-1, big):
        assert g(None, cfg(), col(), n, None, None, None, None) == MVS_ERR_ARG and err(b"n_v"), n
    assert g(None, cfg(), col(), 8, None, nmp, rgp, usp) == MVS_ERR_ARG and err(b"verts or rgb null")
    assert g(None, cfg(), col(), 8, vtp, nmp, None, usp) == MVS_ERR_ARG and err(b"verts or rgb null")
    assert g(None, cfg(), col(), 8, vtp, nmp, rgp, usp) == MVS_ERR_ARG and err(b"no engine")
    assert g(None, cfg(), col(min_cos=-1.0), 8, vtp, None, rgp, None) == MVS_ERR_ARG and err(b"no engine")  # normals and used may be null
    assert g(None, cfg(), col(min_cos=1.0), 0, None, None, None, None) == MVS_ERR_ARG and err(b"no engine")

    # nothing was written on any refused call
    assert (verts == -7).all() and (tris == -7).all() and (normals == -7).all() and (rgb == 249).all() and (used == 249).all()


def _parse_mesh_ply(data):
    """a small PLY reader: -> (format, {element: (count, [(type, name)])}, offset of the body)"""
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").split("\n")
    assert head[0] == "ply" and head[-2] == "end_header"
    elems, cur = {}, None
    for ln in head[2:-2]:
        w = ln.split()
        if w[0] == "element":
            cur = w[1]
            elems[cur] = (int(w[2]), [])
        else:
            assert w[0] == "property"
            elems[cur][1].append((" ".join(w[1:-1]), w[-1]))
    return head[1], elems, end


def _read_back(path):
    data = open(path, "rb").read()
    fmt, elems, end = _parse_mesh_ply(data)
    assert list(elems) == ["vertex", "face"] and elems["face"][1] == [("list uchar int", "vertex_indices")]
    nv, props = elems["vertex"]
    nf = elems["face"][0]
    np_type = {"float": "<f4", "uchar": "u1"}
    names = [n for _, n in props]
    if fmt == "format binary_little_endian 1.0":
        dt = np.dtype([(n, np_type[t]) for t, n in props])
        rows = np.frombuffer(data, dt, count=nv, offset=end)
        faces = np.frombuffer(data, np.dtype([("n", "u1"), ("v", "<i4", (3,))]), count=nf, offset=end + dt.itemsize * nv)
        assert end + dt.itemsize * nv + 13 * nf == len(data) and (faces["n"] == 3).all()
        cols = {n: rows[n] for n in names}
        tris = faces["v"]
    else:
        assert fmt == "format ascii 1.0"
        lines = data[end:].decode("ascii").split("\n")
        assert lines[-1] == "" and len(lines) == nv + nf + 1
        cells = [ln.split() for ln in lines[:nv]]
        assert all(len(c) == len(props) for c in cells)
        cols = {n: np.array([np.float32(c[k]) if t == "float" else int(c[k]) for c in cells], np_type[t]) for k, (t, n) in enumerate(props)}
        f = np.array([[int(x) for x in ln.split()] for ln in lines[nv:nv + nf]], np.int64).reshape(nf, 4)
        assert (f[:, 0] == 3).all()
        tris = f[:, 1:].astype(np.int32)
    return props, cols, tris


@pytest.mark.parametrize("binary", [True, False])
def test_write_mesh_ply_with_normals_and_colours(tmp_path, binary):
    rng = np.random.default_rng(11)
    verts = rng.normal(size=(29, 3)).astype(np.float32) * np.float32(1e3)
    tris = rng.integers(0, 29, size=(40, 3)).astype(np.int32)
    normals = rng.normal(size=(29, 3)).astype(np.float32)
    colours = rng.integers(0, 256, size=(29, 3)).astype(np.uint8)
    p = tmp_path / "m.ply"
    # without the new arguments: the bytes of the file as it was before they existed
    engine.write_mesh_ply(p, verts, tris, binary=binary)
    head = (f"ply\nformat {'binary_little_endian' if binary else 'ascii'} 1.0\nelement vertex 29\nproperty float x\nproperty float y\n"
            f"property float z\nelement face 40\nproperty list uchar int vertex_indices\nend_header\n").encode("ascii")
    if binary:
        faces = np.zeros(40, dtype=np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
        faces["n"], faces["v"] = 3, tris
        body = verts.tobytes() + faces.tobytes()
    else:
        body = ("".join(f"{x:.9g} {y:.9g} {z:.9g}\n" for x, y, z in verts.tolist()) + "".join(f"3 {a} {b} {c}\n" for a, b, c in tris.tolist())).encode("ascii")
    assert open(p, "rb").read() == head + body
    xyz, nrm, rgbn = [("float", n) for n in "xyz"], [("float", n) for n in ("nx", "ny", "nz")], [("uchar", n) for n in ("red", "green", "blue")]
    for kw, want_props, stride in ((dict(normals=normals), xyz + nrm, 24), (dict(colours=colours), xyz + rgbn, 15),
                                   (dict(normals=normals, colours=colours), xyz + nrm + rgbn, 27)):
        engine.write_mesh_ply(p, verts, tris, binary=binary, **kw)
        props, cols, t = _read_back(p)
        assert props == want_props and t.tobytes() == tris.tobytes()
        assert np.stack([cols[n] for n in "xyz"], 1).tobytes() == verts.tobytes()
        if "normals" in kw:
            assert np.stack([cols[n] for n in ("nx", "ny", "nz")], 1).tobytes() == normals.tobytes()
        if "colours" in kw:
            assert np.stack([cols[n] for n in ("red", "green", "blue")], 1).tobytes() == colours.tobytes()
        if binary:
            size = os.path.getsize(p)
            assert (size - 13 * 40 - open(p, "rb").read().index(b"end_header\n") - 11) == stride * 29
    with pytest.raises(ValueError):
        engine.write_mesh_ply(p, verts, tris, normals=normals[:5])
    engine.write_mesh_ply(p, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), binary=binary, normals=np.zeros((0, 3)), colours=np.zeros((0, 3)))
    props, cols, t = _read_back(p)
    assert props == xyz + nrm + rgbn and t.shape == (0, 3) and cols["x"].shape == (0,)
