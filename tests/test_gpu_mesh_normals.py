"""mvs_engine_mesh_normals on the GPU against normals_exact of tests/mesh_attr_reading.py: the reading restates the contract operation by
operation and the sum is an integer sum, so the yardstick is equality of bytes -- whatever order the hardware met the triangles in.  No
scene: the engine has a device and no views."""
import ctypes as C

import numpy as np
import pytest

import mesh_attr_reading as ar
import mesh_reading as mr
from mvskit_amd import engine
from mvskit_amd.engine import MVS_ERR_ARG
from scene_support import grid_mesh

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(2)
    yield e
    e.close()


def _same(e, verts, tris):
    got = e.mesh_normals(verts, tris)
    want = ar.normals_exact(verts, tris)
    assert got.dtype == np.float32 and got.shape == want.shape
    assert got.tobytes() == want.tobytes(), f"{int((got.view(np.uint32) != want.view(np.uint32)).any(axis=1).sum())} normals differ from the reading"
    assert e.mesh_normals(verts, tris).tobytes() == got.tobytes(), "two calls give different bytes"
    return got


def test_one_triangle(eng):
    n = _same(eng, np.array([[0, 0, 0], [2, 0, 0], [0, 3, 0]], np.float32), np.array([[0, 1, 2]], np.int32))
    assert (n == np.array([0, 0, 1], np.float32)).all()
    rng = np.random.default_rng(1)
    _same(eng, rng.normal(size=(3, 3)).astype(np.float32), np.array([[2, 0, 1]], np.int32))


def test_fan_of_20000_triangles_in_shuffled_order(eng):
    """valence 20 000 at vertex 0: 60 000 atomic adds meet on its three words"""
    rng = np.random.default_rng(2)
    k = 20000
    a = 2 * np.pi * np.arange(k) / k
    ring = np.stack([np.cos(a), np.sin(a), 0.05 * rng.normal(size=k)], 1)
    verts = np.concatenate([[[0.0, 0.0, 0.3]], ring]).astype(np.float32)
    i = np.arange(k)
    tris = np.stack([np.zeros(k, np.int64), 1 + i, 1 + (i + 1) % k], 1).astype(np.int32)
    tris = tris[rng.permutation(k)]
    n = _same(eng, verts, tris)
    assert n[0, 2] > 0.9
    # listed in another order: the same bytes
    assert eng.mesh_normals(verts, tris[rng.permutation(k)]).tobytes() == n.tobytes()


def test_grid_with_jittered_heights(eng):
    """70 x 70: 4900 vertices in 20 blocks, 9522 triangles in 38"""
    z = 0.3 * np.random.default_rng(3).normal(size=(70, 70))
    verts, tris = grid_mesh(70, 70, z)
    n = _same(eng, verts, tris)
    assert (n[:, 2] > 0).all()


def test_sphere_from_extract_mesh(eng):
    dims, origin, voxel = (11, 10, 10), (1.0, 2.0, 3.0), 0.5
    centre = np.array([1.0 + 0.5 * 5.2, 2.0 + 0.5 * 4.4, 3.0 + 0.5 * 4.6])
    F = mr.sphere_volume(dims, [centre], 0.5 * 3.3, origin=origin, voxel=voxel)
    verts, tris = eng.extract_mesh(engine.make_volume(origin, voxel, dims, 1.0), F)
    assert verts.shape[0] == 604
    n = _same(eng, verts, tris).astype(np.float64)
    radial = verts.astype(np.float64) - centre
    radial /= np.linalg.norm(radial, axis=1, keepdims=True)
    assert ((n * radial).sum(1) > 0.9).all(), "a normal does not point outward"


def test_face_areas_over_a_factor_of_2_to_the_40(eng):
    """three separate triangles of areas 1, 2^-20 and 2^-40, and a vertex shared by a large and a vanishing face: below 2^-31 of the largest
    component a face adds nothing; and the same mesh scaled by 2^60 and 2^-60 (the scale follows the largest component)"""
    s, t = 2.0 ** -10, 2.0 ** -20
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0],
                      [5, 5, 0], [5 + s, 5, 0], [5, 5, s],
                      [9, 9, 0], [9 + t, 9, 0], [9, 9 + t, t],
                      [0, 0, t]], np.float32)
    tris = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8], [0, 9, 2], [1, 0, 9]], np.int32)
    n = _same(eng, verts, tris)
    assert (n[6:9] == 0).all() and (n[3:6] == np.array([0, -1, 0], np.float32)).all() and n[0, 2] > 0.99
    for scale in (2.0 ** 60, 2.0 ** -60):
        moved = (verts.astype(np.float64) * scale).astype(np.float32)
        _same(eng, moved, tris)
    # the largest component overflows: that face is non-finite and adds nothing, the others set the scale
    huge = verts.copy()
    huge[3:6] *= np.float32(2.0 ** 80)
    n = _same(eng, huge, tris)
    assert (n[3:6] == 0).all() and n[0, 2] > 0.99


def test_a_triangle_with_a_nan_vertex(eng):
    verts, tris = grid_mesh(6, 5, np.random.default_rng(5).normal(size=(5, 6)))
    clean = _same(eng, verts, tris)
    bad = np.concatenate([verts, [[np.nan, 0, 0], [np.inf, 1, 1]]]).astype(np.float32)
    more = np.concatenate([tris, [[0, 7, 30], [31, 8, 9], [30, 31, 3]]]).astype(np.int32)
    n = _same(eng, bad, more)
    assert n[:30].tobytes() == clean.tobytes() and (n[30:] == 0).all()


def test_degenerate_and_empty(eng):
    verts = np.random.default_rng(6).normal(size=(300, 3)).astype(np.float32)
    line = np.stack([np.arange(298), np.arange(298), np.arange(298) + 1], 1).astype(np.int32)  # no area anywhere
    assert (_same(eng, verts, line) == 0).all()
    assert (_same(eng, verts, np.zeros((0, 3), np.int32)) == 0).all()
    assert _same(eng, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)).shape == (0, 3)


def test_an_index_out_of_range_is_refused_and_nothing_written(eng):
    verts, tris = grid_mesh(20, 20)
    out = np.full((400, 3), -7, np.float32)
    f = eng.L.mvs_engine_mesh_normals
    for where, value in ((0, 400), (tris.shape[0] - 1, -1), (300, 1 << 30), (17, -(1 << 31))):
        t = tris.copy()
        t[where, 1] = value
        assert f(eng.h, 400, verts.ctypes.data_as(C.c_void_p), t.shape[0], t.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) == MVS_ERR_ARG
        assert b"index" in eng.L.mvs_last_error() and (out == -7).all(), (where, value)
    # no vertices at all: every index is out of range
    t = np.zeros((1, 3), np.int32)
    assert f(eng.h, 0, None, 1, t.ctypes.data_as(C.c_void_p), None) == MVS_ERR_ARG and b"index" in eng.L.mvs_last_error()
    assert f(eng.h, 400, verts.ctypes.data_as(C.c_void_p), tris.shape[0], tris.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) == 0
    assert out.tobytes() == ar.normals_exact(verts, tris).tobytes()


def test_device_tensors(eng):
    """the mesh and the normals as torch device tensors: the same bytes as through host pointers"""
    import torch

    verts, tris = grid_mesh(33, 17, np.random.default_rng(7).normal(size=(17, 33)))
    want = _same(eng, verts, tris)
    dev = torch.device("cuda", eng.cfg.device)
    dV, dT = torch.from_numpy(verts).to(dev), torch.from_numpy(tris).to(dev)
    dN = torch.zeros((verts.shape[0], 3), dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    eng._check(eng.L.mvs_engine_mesh_normals(eng.h, verts.shape[0], C.c_void_p(dV.data_ptr()), tris.shape[0], C.c_void_p(dT.data_ptr()), C.c_void_p(dN.data_ptr())))
    assert dN.cpu().numpy().tobytes() == want.tobytes()
