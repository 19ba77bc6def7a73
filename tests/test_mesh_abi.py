"""CPU-side checks of the mesh entry points (include/mvskit_engine.h: mvs_volume, mvs_engine_tsdf, mvs_engine_extract_mesh,
mvs_engine_mesh): every engine library exports them, mvs_volume is 40 bytes with the declared layout, bad arguments are refused in the
header's order before the handle is read or a device is touched, with nothing written through an output pointer; and the two helpers
that need no device, volume_around and write_mesh_ply."""
import ctypes as C

import numpy as np
import pytest

from mvskit_amd import build, engine
from mvskit_amd.engine import MVS_ERR_ARG

SYMBOLS = ("mvs_engine_tsdf", "mvs_engine_extract_mesh", "mvs_engine_mesh")


@pytest.mark.parametrize("cap", [16, 32, 64])
def test_mesh_symbols_layout_and_argument_checks(cap):
    build.build_engine(cap=cap)
    lib = engine.load_library(cap=cap)
    for name in SYMBOLS:
        assert hasattr(lib, name), f"libmvskit_engine (cap {cap}) has no {name}"
        assert name in engine.EXPORTS
    V = engine.Volume
    assert C.sizeof(V) == 40 and C.sizeof(engine.MapsConfig) == 24
    assert [(n, getattr(V, n).offset) for n, _ in V._fields_] == [("origin", 0), ("voxel", 12), ("dims", 16), ("trunc", 28), ("min_count", 32), ("pad", 36)]

    def err(word):
        return word in lib.mvs_last_error()

    def cfg(**kw):
        c = engine.MapsConfig()
        lib.mvs_default_maps_config(C.byref(c))
        for k, v in kw.items():
            setattr(c, k, v)
        return C.byref(c)

    def vol(voxel=0.5, dims=(4, 3, 2), trunc=2.0, min_count=1):
        return C.byref(engine.make_volume((0.0, 0.0, 0.0), voxel, dims, trunc, min_count))

    nan, inf = float("nan"), float("inf")
    vp = C.c_void_p
    tsdf = np.full(24, -7, np.float32)
    count = np.full(24, -7, np.int32)
    verts = np.full((8, 3), -7, np.float32)
    tris = np.full((8, 3), -7, np.int32)
    tp, cp, vtp, trp = (a.ctypes.data_as(vp) for a in (tsdf, count, verts, tris))
    nv, nt = C.c_int64(-7), C.c_int64(-7)
    pnv, pnt = C.byref(nv), C.byref(nt)

    # the volume's own ladder, through a call that takes (volume, rest...) with every later argument bad too
    def volume_ladder(call):
        assert call(None) == MVS_ERR_ARG and err(b"volume null")
        for x in (0.0, -1.0, nan, inf):
            assert call(vol(voxel=x, trunc=nan, dims=(1, 1, 1), min_count=0)) == MVS_ERR_ARG and err(b"voxel"), x
        for x in (0.0, -1.0, nan, inf):
            assert call(vol(trunc=x, dims=(1, 1, 1), min_count=0)) == MVS_ERR_ARG and err(b"trunc"), x
        for d in ((1, 4, 4), (4, 1025, 4), (4, 4, 0), (-3, 4, 4)):
            assert call(vol(dims=d, min_count=0)) == MVS_ERR_ARG and err(b"dimension"), d
        assert call(vol(dims=(1024, 1024, 257), min_count=0)) == MVS_ERR_ARG and err(b"2^28")
        for m in (0, -1):
            assert call(vol(min_count=m)) == MVS_ERR_ARG and err(b"min_count"), m

    # mvs_engine_tsdf: the maps ladder, the volume, the outputs, the engine
    f = lib.mvs_engine_tsdf
    assert f(None, None, None, None, None) == MVS_ERR_ARG and err(b"config null")
    assert f(None, cfg(source=2, min_consistent=-1), None, None, None) == MVS_ERR_ARG and err(b"source")
    assert f(None, cfg(min_consistent=-1, depth_tol=0.0), None, None, None) == MVS_ERR_ARG and err(b"min_consistent")
    assert f(None, cfg(depth_tol=0.0, normal_cos=2.0), None, None, None) == MVS_ERR_ARG and err(b"depth_tol")
    assert f(None, cfg(normal_cos=2.0), None, None, None) == MVS_ERR_ARG and err(b"normal_cos")
    volume_ladder(lambda v: f(None, cfg(), v, None, None))
    assert f(None, cfg(), vol(), None, cp) == MVS_ERR_ARG and err(b"tsdf or count null")
    assert f(None, cfg(), vol(), tp, None) == MVS_ERR_ARG and err(b"tsdf or count null")
    assert f(None, cfg(), vol(), tp, cp) == MVS_ERR_ARG and err(b"no engine")

    # mvs_engine_extract_mesh: the volume, tsdf, n_v / n_t, the caps, the engine
    g = lib.mvs_engine_extract_mesh
    volume_ladder(lambda v: g(None, v, None, None, -1, vtp, -1, trp, None, None))
    assert g(None, vol(), None, cp, -1, vtp, -1, trp, None, None) == MVS_ERR_ARG and err(b"tsdf null")
    assert g(None, vol(), tp, cp, -1, vtp, -1, trp, None, pnt) == MVS_ERR_ARG and err(b"n_v or n_t null")
    assert g(None, vol(), tp, cp, -1, vtp, -1, trp, pnv, None) == MVS_ERR_ARG and err(b"n_v or n_t null")
    assert g(None, vol(), tp, cp, -1, vtp, 8, trp, pnv, pnt) == MVS_ERR_ARG and err(b"negative cap")
    assert g(None, vol(), tp, cp, 8, vtp, -1, trp, pnv, pnt) == MVS_ERR_ARG and err(b"negative cap")
    assert g(None, vol(), tp, cp, 8, vtp, 8, trp, pnv, pnt) == MVS_ERR_ARG and err(b"no engine")
    assert g(None, vol(), tp, None, 0, None, 0, None, pnv, pnt) == MVS_ERR_ARG and err(b"no engine")

    # mvs_engine_mesh: the maps ladder, the volume, n_v / n_t, the caps, the engine
    h = lib.mvs_engine_mesh
    assert h(None, None, None, -1, vtp, -1, trp, None, None) == MVS_ERR_ARG and err(b"config null")
    assert h(None, cfg(normal_cos=2.0), None, -1, vtp, -1, trp, None, None) == MVS_ERR_ARG and err(b"normal_cos")
    volume_ladder(lambda v: h(None, cfg(), v, -1, vtp, -1, trp, None, None))
    assert h(None, cfg(), vol(), -1, vtp, -1, trp, None, pnt) == MVS_ERR_ARG and err(b"n_v or n_t null")
    assert h(None, cfg(), vol(), -1, vtp, 8, trp, pnv, pnt) == MVS_ERR_ARG and err(b"negative cap")
    assert h(None, cfg(), vol(), 8, vtp, 8, trp, pnv, pnt) == MVS_ERR_ARG and err(b"no engine")

    # nothing was written on any refused call
    assert (tsdf == -7).all() and (count == -7).all() and (verts == -7).all() and (tris == -7).all() and nv.value == -7 and nt.value == -7


def test_volume_around():
    rng = np.random.default_rng(5)
    xyz = rng.uniform([-1.0, 0.5, 2.0], [1.5, 0.9, 2.1], size=(200, 3))
    v = engine.volume_around(xyz, 0.1)
    o, d = np.array(v.origin[:], np.float64), np.array(v.dims[:])
    assert C.sizeof(v) == 40 and v.shape == (d[2], d[1], d[0])
    assert v.voxel == np.float32(0.1) and v.trunc == np.float32(0.4) and v.min_count == 1
    top = o + (d - 1) * 0.1
    # two voxels of padding on every side, and no more than one voxel beyond that
    assert (o <= xyz.min(0) - 0.2 + 1e-6).all() and (o >= xyz.min(0) - 0.2 - 1e-6).all()
    assert (top >= xyz.max(0) + 0.2 - 1e-6).all() and (top <= xyz.max(0) + 0.3 + 1e-6).all()
    w = engine.volume_around(xyz, 0.1, trunc_voxels=3, pad_voxels=0, min_count=2)
    assert w.trunc == np.float32(0.3) and w.min_count == 2 and (np.array(w.dims[:]) == d - 4).all()
    for bad in (np.zeros((0, 3)), np.array([[0.0, np.nan, 0.0]])):
        with pytest.raises(ValueError):
            engine.volume_around(bad, 0.1)
    with pytest.raises(ValueError):
        engine.volume_around(xyz, 1e-4)  # more than 1024 lattice points along x
    with pytest.raises(ValueError):
        engine.volume_around(xyz, 0.0)


def _read_mesh_ply(path):
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").split("\n")
    assert head[0] == "ply" and head[-2] == "end_header"
    fmt = head[1]
    elems = [ln for ln in head if ln.startswith("element ")]
    assert [e.split()[1] for e in elems] == ["vertex", "face"]
    nv, nf = (int(e.split()[2]) for e in elems)
    props = [ln for ln in head if ln.startswith("property ")]
    assert props == ["property float x", "property float y", "property float z", "property list uchar int vertex_indices"]
    if fmt == "format binary_little_endian 1.0":
        verts = np.frombuffer(data, "<f4", count=3 * nv, offset=end).reshape(nv, 3)
        faces = np.frombuffer(data, np.dtype([("n", "u1"), ("v", "<i4", (3,))]), count=nf, offset=end + 12 * nv)
        assert end + 12 * nv + 13 * nf == len(data) and (faces["n"] == 3).all()
        return verts, faces["v"]
    assert fmt == "format ascii 1.0"
    rows = data[end:].decode("ascii").split("\n")
    assert rows[-1] == "" and len(rows) == nv + nf + 1
    verts = np.array([[np.float32(x) for x in r.split()] for r in rows[:nv]], np.float32).reshape(nv, 3)
    faces = np.array([[int(x) for x in r.split()] for r in rows[nv:nv + nf]], np.int64).reshape(nf, 4)
    assert (faces[:, 0] == 3).all()
    return verts, faces[:, 1:].astype(np.int32)


@pytest.mark.parametrize("binary", [True, False])
def test_write_mesh_ply_round_trip(tmp_path, binary):
    rng = np.random.default_rng(9)
    verts = rng.normal(size=(37, 3)).astype(np.float32) * np.float32(1e3)
    verts[0] = [0.0, -0.0, 1e-20]
    tris = rng.integers(0, 37, size=(51, 3)).astype(np.int32)
    p = tmp_path / "m.ply"
    engine.write_mesh_ply(p, verts, tris, binary=binary)
    v, t = _read_mesh_ply(p)
    assert v.tobytes() == verts.tobytes() and t.tobytes() == tris.tobytes()
    engine.write_mesh_ply(p, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), binary=binary)
    v, t = _read_mesh_ply(p)
    assert v.shape == (0, 3) and t.shape == (0, 3)
