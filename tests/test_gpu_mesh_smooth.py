"""mvs_engine_mesh_smooth on the GPU against smooth_exact of tests/mesh_clean_reading.py: the reading restates the contract operation by
operation and the sums are integer sums, so the yardstick is equality of bytes -- whatever order the hardware met the triangles in.  No
scene: the engine has a device and no views."""
import ctypes as C

import numpy as np
import pytest

import mesh_clean_reading as cr
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


def _same(e, verts, tris, **kw):
    got = e.smooth_mesh(verts, tris, **kw)
    want = cr.smooth_exact(verts, tris, **kw)
    assert got.dtype == np.float32 and got.shape == want.shape
    assert got.tobytes() == want.tobytes(), f"{int((got.view(np.uint32) != want.view(np.uint32)).any(axis=1).sum())} positions differ from the reading"
    assert e.smooth_mesh(verts, tris, **kw).tobytes() == got.tobytes(), "two calls give different bytes"
    return got


def _interior_rms(verts, n):
    z = verts[:, 2].astype(np.float64).reshape(n, n)[1:-1, 1:-1]
    return float(np.sqrt((z * z).mean()))


def test_one_triangle(eng):
    tri = np.array([[0, 0, 0], [4, 0, 0], [0, 8, 0]], np.float32)
    out = _same(eng, tri, np.array([[0, 1, 2]], np.int32), iterations=1, lam=0.5, mu=0.0)
    assert (out == np.array([[1, 2, 0], [2, 2, 0], [1, 4, 0]], np.float32)).all()
    rng = np.random.default_rng(51)
    _same(eng, rng.normal(size=(3, 3)).astype(np.float32), np.array([[2, 0, 1]], np.int32))


def test_fan_of_20000_triangles_in_two_orders(eng):
    """valence 20 000 at vertex 0: 60 000 atomic adds and 20 000 counts meet on its words, every step"""
    rng = np.random.default_rng(52)
    k = 20000
    a = 2 * np.pi * np.arange(k) / k
    ring = np.stack([np.cos(a), np.sin(a), 0.05 * rng.normal(size=k)], 1)
    verts = np.concatenate([[[0.0, 0.0, 0.3]], ring]).astype(np.float32)
    i = np.arange(k)
    tris = np.stack([np.zeros(k, np.int64), 1 + i, 1 + (i + 1) % k], 1).astype(np.int32)
    out = _same(eng, verts, tris[rng.permutation(k)], iterations=3)
    assert eng.smooth_mesh(verts, tris[rng.permutation(k)], iterations=3).tobytes() == out.tobytes()


def test_jittered_grid_gets_flatter(eng):
    """70 x 70: 4900 vertices in 20 blocks, 9522 triangles in 38; the rms height of the interior falls as on the CPU (0.3008 -> 0.1151)"""
    verts, tris = grid_mesh(70, 70, 0.3 * np.random.default_rng(3).normal(size=(70, 70)))
    out = _same(eng, verts, tris)
    assert _interior_rms(out, 70) < _interior_rms(verts, 70)


def test_sphere_from_extract_mesh(eng):
    dims, origin, voxel = (11, 10, 10), (1.0, 2.0, 3.0), 0.5
    centre = np.array([1.0 + 0.5 * 5.2, 2.0 + 0.5 * 4.4, 3.0 + 0.5 * 4.6])
    F = mr.sphere_volume(dims, [centre], 0.5 * 3.3, origin=origin, voxel=voxel)
    verts, tris = eng.extract_mesh(engine.make_volume(origin, voxel, dims, 1.0), F)
    assert verts.shape[0] == 604
    taubin, laplace = _same(eng, verts, tris), _same(eng, verts, tris, mu=0.0)

    def volume(v):
        v = v.astype(np.float64) - centre
        return float(abs((v[tris[:, 0]] * np.cross(v[tris[:, 1]], v[tris[:, 2]])).sum()) / 6.0)

    # as on the CPU (17.953: 18.103 after Taubin, 14.372 after Laplacian): the second step keeps the volume
    assert abs(volume(taubin) - volume(verts)) < abs(volume(laplace) - volume(verts))


def test_zero_iterations_copy_and_mu_zero(eng):
    verts, tris = grid_mesh(12, 12, np.random.default_rng(53).normal(size=(12, 12)))
    assert _same(eng, verts, tris, iterations=0).tobytes() == verts.tobytes()
    lap = _same(eng, verts, tris, iterations=4, mu=0.0)
    assert lap.tobytes() != _same(eng, verts, tris, iterations=4).tobytes()
    _same(eng, verts, tris, iterations=1, lam=0.9, mu=-0.95)


def test_translated_grid(eng):
    """the grid far from the origin: the terms, not the positions, set the scale"""
    verts, tris = grid_mesh(70, 70, 0.3 * np.random.default_rng(3).normal(size=(70, 70)))
    moved = verts + np.array([1e4, -1e4, 1e4], np.float32)
    out = _same(eng, moved, tris, iterations=3)
    assert np.abs(out - moved).max() < 2.0


def test_a_vertex_with_a_nan(eng):
    verts, tris = grid_mesh(6, 5, np.random.default_rng(55).normal(size=(5, 6)))
    bad = verts.copy()
    bad[14, 1] = np.nan   # an interior vertex
    bad[3, 0] = np.inf    # one on the rim
    out = _same(eng, bad, tris, iterations=2)
    assert out[14].tobytes() == bad[14].tobytes() and out[3].tobytes() == bad[3].tobytes()
    others = np.delete(np.arange(30), [14, 3])
    assert np.isfinite(out[others]).all()
    # a vertex whose every term is dropped keeps its bytes: the corner of a triangle with two bad neighbours
    lone = np.array([[0, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [1, 1, 1], [2, 1, 1], [1, 2, 1]], np.float32)
    out = _same(eng, lone, np.array([[0, 1, 2], [3, 4, 5]], np.int32), iterations=1)
    assert out[:3].tobytes() == lone[:3].tobytes() and (out[3:] != lone[3:]).any()


def test_unused_vertices_and_coincident_vertices(eng):
    verts, tris = grid_mesh(9, 9, np.random.default_rng(56).normal(size=(9, 9)))
    more = np.concatenate([[[np.nan, -0.0, 5.0]], verts, [[1e30, -1e-40, 3.0]]]).astype(np.float32)
    out = _same(eng, more, tris + 1, iterations=2)
    assert out[0].tobytes() == more[0].tobytes() and out[-1].tobytes() == more[-1].tobytes()
    same = np.tile(np.float32([-0.0, 2.5, -1.0]), (81, 1))  # M == 0: every step leaves the bytes, the sign of a zero too
    assert _same(eng, same, tris, iterations=2).tobytes() == same.tobytes()
    assert _same(eng, verts, np.zeros((0, 3), np.int32)).tobytes() == verts.tobytes()
    assert _same(eng, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)).shape == (0, 3)
    # repeated ids: their zero terms count
    _same(eng, verts, np.array([[0, 0, 1], [5, 5, 5], [7, 8, 7], [1, 2, 10]], np.int32), iterations=2)


def test_a_bad_id_is_refused_and_nothing_written(eng):
    verts, tris = grid_mesh(20, 20)
    out = np.full((400, 3), -7, np.float32)
    vp = C.c_void_p
    f = eng.L.mvs_engine_mesh_smooth
    for iterations in (2, 0):
        s = engine.MeshSmoothing(iterations, 0.5, -0.53, 0)
        for where, value in ((0, 400), (tris.shape[0] - 1, -1), (300, 1 << 30)):
            t = tris.copy()
            t[where, 0] = value
            assert f(eng.h, C.byref(s), 400, verts.ctypes.data_as(vp), t.shape[0], t.ctypes.data_as(vp), out.ctypes.data_as(vp)) == MVS_ERR_ARG
            assert b"index" in eng.L.mvs_last_error() and (out == -7).all(), (where, value)


def test_device_tensors(eng):
    import torch

    verts, tris = grid_mesh(33, 17, np.random.default_rng(57).normal(size=(17, 33)))
    want = _same(eng, verts, tris, iterations=3)
    dev = torch.device("cuda", eng.cfg.device)
    dV, dT = torch.from_numpy(verts).to(dev), torch.from_numpy(tris).to(dev)
    dO = torch.zeros((verts.shape[0], 3), dtype=torch.float32, device=dev)
    s = engine.MeshSmoothing(3, 0.5, -0.53, 0)
    torch.cuda.synchronize(dev)
    eng._check(eng.L.mvs_engine_mesh_smooth(eng.h, C.byref(s), verts.shape[0], C.c_void_p(dV.data_ptr()), tris.shape[0], C.c_void_p(dT.data_ptr()),
                                            C.c_void_p(dO.data_ptr())))
    assert dO.cpu().numpy().tobytes() == want.tobytes()
