"""mvs_engine_export_ply / Engine.export_ply / Engine.points, and the host mirror's PatchManager::writePly on top of them, against a
numpy restatement of the file the mirror wrote before the device path existed (patch_manager.cpp:542-633): the same header, one
"%g"-formatted line per alive patch, the colour as the mean over m_images of a bilinear sample of the level-`level` pyramid computed in
float32 in the mirror's order of operations (P of the level: rows 0-1 halved per level; a view the point lies behind or projects
outside [0, W-1) x [0, H-1) counts but adds nothing; 128 for an empty list)."""
import ctypes as C

import numpy as np
import pytest

import camera_scenes as cs
from mvskit_amd import build, engine, synth
from ply_support import level_inputs, parse_ascii, restate_ply


@pytest.fixture(scope="module")
def host():
    build.build_engine()
    engine.load_library()
    L = C.CDLL(build.build_host())
    L.mvshost_set_ply_output.argtypes = [C.c_char_p]
    L.mvshost_set_ply_output.restype = None
    L.mvshost_run.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_uint,
                              C.c_int, C.c_longlong, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


@pytest.mark.gpu
@pytest.mark.parametrize("level", [0, 1])
def test_mirror_writeply_is_the_restatement(host, small_plane_scene, tmp_path, level):
    """PatchManager::writePly of the host mirror (now mvs_engine_export_ply) writes, byte for byte, the file of the restatement."""
    _mirror_writeply(host, small_plane_scene, tmp_path, level)


@pytest.mark.gpu
def test_mirror_writeply_on_mixed_cameras(host, tmp_path):
    """the same at level 0 on the `mixed` family of camera_scenes.py, 3 views of 160 x 120 of the plane: k_ply_colour's projection and
    image indexed by views whose intrinsics, roll and distance differ, around (12, -8, 16)"""
    _mirror_writeply(host, cs.family_scene("mixed", 3, 160, 120, 30.0, "plane"), tmp_path, 0)


def _mirror_writeply(host, sc, tmp_path, level):
    seeds = synth.make_seeds(sc, level=level, stride=4, seed=21)
    out = np.zeros(200000, dtype=engine.PATCH_DTYPE)
    nout, ptot = C.c_longlong(), C.c_longlong()
    P = np.ascontiguousarray(sc.P, dtype=np.float32)
    img = np.ascontiguousarray(sc.images)
    sd = np.ascontiguousarray(seeds)
    ply = tmp_path / "out.ply"
    host.mvshost_set_ply_output(str(ply).encode())
    r = host.mvshost_run(sc.nviews, sc.W, sc.H, P.ctypes.data, img.ctypes.data, level, 2, 7, 2, C.c_float(0.7), 9, 2, sd.shape[0], sd.ctypes.data,
                         out.shape[0], out.ctypes.data, C.byref(nout), C.byref(ptot))
    host.mvshost_set_ply_output(b"")
    assert r == 0 and 0 < nout.value < out.shape[0]
    recs = out[: nout.value]
    e = engine.Engine(sc.nviews, level=level, minImageNum=2)
    e.set_scene(sc)
    Pl, pyr = level_inputs(e, sc, level)
    e.close()
    got = ply.read_bytes()
    want = restate_ply(recs, Pl, pyr)
    assert got == want
    # the colours are not all the grey of an empty list
    assert len({tuple(r[6:9]) for r in parse_ascii(got)}) > 10


@pytest.fixture(scope="module")
def swept(small_plane_scene):
    sc = small_plane_scene
    e = engine.Engine(sc.nviews, level=0, minImageNum=2, enable_check=1, seed=5)
    e.set_scene(sc)
    e.upload_patches(synth.make_seeds(sc, stride=4, seed=3))
    e.propagate(0)
    yield e
    e.close()


@pytest.mark.gpu
def test_binary_and_points_carry_the_ascii_numbers(swept, small_plane_scene):
    e = swept
    text, binary = e.export_ply(), e.export_ply(binary=True)
    pe = e.patches()
    P, pyr = level_inputs(e, small_plane_scene, 0)
    assert text == restate_ply(pe, P, pyr)
    assert binary == restate_ply(pe, P, pyr, binary=True)
    assert binary.startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % pe.shape[0])
    pts = e.points()
    assert pts.dtype.itemsize == 27 and pts.shape[0] == pe.shape[0] > 0
    np.testing.assert_array_equal(pts["xyz"], pe["coord"][:, :3])
    np.testing.assert_array_equal(pts["normal"], pe["normal"][:, :3])
    rows = parse_ascii(text)
    assert len(rows) == pts.shape[0]
    for i in range(0, pts.shape[0], max(1, pts.shape[0] // 500)):
        assert rows[i][:6] == ["%g" % v for v in (*pts["xyz"][i], *pts["normal"][i])]
        assert [int(t) for t in rows[i][6:]] == list(pts["rgb"][i])


def _raw_export(e, fmt, cap, buf):
    n = C.c_int64(-1)
    r = e.L.mvs_engine_export_ply(e.h, fmt, cap, buf, C.byref(n))
    return r, n.value


@pytest.mark.gpu
def test_capacity_and_size_query(swept):
    e = swept
    for fmt, binary in ((engine.PLY_ASCII, False), (engine.PLY_BINARY_LE, True)):
        r, n = _raw_export(e, fmt, 0, None)
        assert r == 0 and n == len(e.export_ply(binary=binary))
        buf = C.create_string_buffer(b"\x5a" * n, n)
        r, n2 = _raw_export(e, fmt, n - 1, buf)
        assert r == -4 and n2 == n  # MVS_ERR_CAPACITY, *nbytes = the exact size
        assert buf.raw == b"\x5a" * n  # nothing written
        r, n3 = _raw_export(e, fmt, n, buf)
        assert r == 0 and n3 == n and buf.raw == e.export_ply(binary=binary)
    assert _raw_export(e, 2, 0, None)[0] == -1


@pytest.mark.gpu
def test_empty_pool_and_views_outside(small_plane_scene):
    sc = small_plane_scene
    e = engine.Engine(sc.nviews, level=0, minImageNum=2)
    e.set_scene(sc)
    for binary in (False, True):
        data = e.export_ply(binary=binary)
        assert data == restate_ply(np.zeros(0, e.dtype), [], [], binary=binary) and b"element vertex 0\n" in data and data.endswith(b"end_header\n")
    # patches at the border of the scene: each seed as it is, then moved so far sideways that some or all of its listed views see it
    # outside the image or behind the camera
    seeds = synth.make_seeds(sc, stride=8, seed=4)
    seeds = seeds[seeds["nimages"] == sc.nviews][:50]
    assert seeds.shape[0] > 10
    far = seeds.copy()
    far["coord"][:, 0] += 40.0  # outside every image
    behind = seeds.copy()
    mid = np.asarray(sc.centers, np.float64).mean(axis=0)
    behind["coord"][:, :3] = (2 * mid - seeds["coord"][:, :3].astype(np.float64)).astype(np.float32)  # mirrored through the cameras
    recs = np.concatenate([seeds, far, behind])
    e.upload_patches(recs)
    pe = e.patches()
    P, pyr = level_inputs(e, sc, 0)
    text = e.export_ply()
    assert text == restate_ply(pe, P, pyr)
    assert e.export_ply(binary=True) == restate_ply(pe, P, pyr, binary=True)
    pts = e.points()
    k = seeds.shape[0]
    assert (pts["rgb"][k:2 * k] == 0).all()  # every listed view counts, none adds a sample: 0, not the 128 of an empty list
    for i in range(k, 3 * k):
        P0 = [np.asarray(sc.P[v], np.float64) @ pe["coord"][i].astype(np.float64) for v in range(sc.nviews)]
        assert all(p[2] <= 0 or not (0 <= p[0] / p[2] < sc.W - 1 and 0 <= p[1] / p[2] < sc.H - 1) for p in P0)
    assert (pts["rgb"][2 * k:3 * k] == 0).all()
    e.close()


@pytest.mark.gpu
def test_export_only_reads(small_plane_scene):
    """propagate after an export gives the pool of a run without it."""
    sc = small_plane_scene
    seeds = synth.make_seeds(sc, stride=4, seed=8)
    pools, counts = [], []
    for export in (False, True):
        e = engine.Engine(sc.nviews, level=0, minImageNum=2, enable_check=1, seed=11)
        e.set_scene(sc)
        e.upload_patches(seeds)
        c = [e.propagate(0)]
        if export:
            t0 = e.thresholds()
            e.export_ply()
            e.export_ply(binary=True)
            e.points()
            assert e.thresholds() == t0
        e.filter()
        e.update_threshold()
        c.append(e.propagate(1))
        pools.append(e.patches())
        counts.append(c)
        e.close()
    assert counts[0] == counts[1]
    assert pools[0].tobytes() == pools[1].tobytes()


@pytest.mark.gpu
def test_cap64_lists_longer_than_32():
    """The 64-view library (192-byte records): lists of 40 views, byte for byte."""
    nv = 40
    sc = synth.make_scene(nviews=nv, W=128, H=96, arc_deg=20.0, radius=4.0, kind="plane")
    seeds = synth.make_seeds(sc, level=1, stride=2, seed=6, views=[0, nv // 2])
    e = engine.Engine(nv, level=1, minImageNum=2)
    assert e.list_cap == 64
    recs = synth.convert_records(seeds, e.dtype)
    # every view listed (the reference first): 40 entries, some of them views that see the point outside their image
    for i in range(recs.shape[0]):
        ref = int(recs["images"][i, 0])
        recs["images"][i, :nv] = [ref] + [u for u in range(nv) if u != ref]
    recs["nimages"] = nv
    long_ = recs["nimages"] > 32
    assert long_.sum() > 20
    e.set_scene(sc)
    e.upload_patches(recs)
    pe = e.patches()
    assert (pe["nimages"] > 32).sum() == long_.sum()
    P, pyr = level_inputs(e, sc, 1)
    assert e.export_ply() == restate_ply(pe, P, pyr)
    assert e.export_ply(binary=True) == restate_ply(pe, P, pyr, binary=True)
    e.close()
