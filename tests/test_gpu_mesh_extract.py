"""mvs_engine_extract_mesh on the GPU against tests/mesh_reading.py: the reading restates the extraction in numpy float32 in the stated
operation order, so the yardstick is equality -- the vertex count, order and bits, and the triangle list.  No scene: the engine has a
device and no views."""
import ctypes as C

import numpy as np
import pytest

import mesh_reading as mr
from mvskit_amd import engine
from mvskit_amd.engine import MVS_ERR_CAPACITY

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(2)
    yield e
    e.close()


def _same(e, origin, voxel, dims, F, count=None, min_count=1):
    vol = engine.make_volume(origin, voxel, dims, 1.0, min_count)
    verts, tris = e.extract_mesh(vol, F, count)
    want_v, want_t = mr.extract(origin, voxel, dims, F, count, min_count)
    assert verts.shape == want_v.shape and tris.shape == want_t.shape, (verts.shape, want_v.shape, tris.shape, want_t.shape)
    assert verts.tobytes() == want_v.tobytes(), "vertex bits differ from the reading"
    assert tris.tobytes() == want_t.tobytes(), "the triangle list differs from the reading"
    return verts, tris


def test_the_256_patterns_of_one_cube(eng):
    rng = np.random.default_rng(1)
    total = 0
    for m in range(256):
        mag = rng.uniform(0.1, 2.0, 8).astype(np.float32)
        F = np.where([(m >> c) & 1 for c in range(8)], -mag, mag).astype(np.float32).reshape(2, 2, 2)
        _, tris = _same(eng, (0.25, -1.5, 3.0), 0.37, (2, 2, 2), F)
        total += tris.shape[0]
    assert total == 1920


def test_random_volume_with_unobserved_points(eng):
    """5 x 4 x 3 random values, about a quarter of the points unobserved: NaN, or a count below min_count; and through count = None"""
    rng = np.random.default_rng(2)
    dims = (5, 4, 3)
    for trial in range(4):
        F = rng.normal(size=(3, 4, 5)).astype(np.float32)
        F[rng.random(F.shape) < 0.12] = np.nan
        count = np.where(rng.random(F.shape) < 0.14, 1, rng.integers(2, 5, F.shape)).astype(np.int32)
        unobs = np.isnan(F) | (count < 2)
        assert 0.1 < unobs.mean() < 0.45
        verts, tris = _same(eng, (-0.3, 0.1, 7.0), 0.05, dims, F, count, min_count=2)
        assert verts.shape[0] > 0
        all_v, all_t = _same(eng, (-0.3, 0.1, 7.0), 0.05, dims, F, None, min_count=2)
        assert all_v.shape[0] >= verts.shape[0]
        _same(eng, (-0.3, 0.1, 7.0), 0.05, dims, F, count, min_count=1)  # every count passes


def test_sphere_over_more_than_one_scan_block(eng):
    """11 x 10 x 10 = 1100 points: the scans take more than one block; 604 vertices and 1204 triangles, closed, Euler characteristic 2"""
    dims = (11, 10, 10)
    F = mr.sphere_volume(dims, [(1.0 + 0.5 * 5.2, 2.0 + 0.5 * 4.4, 3.0 + 0.5 * 4.6)], 0.5 * 3.3, origin=(1.0, 2.0, 3.0), voxel=0.5)
    verts, tris = _same(eng, (1.0, 2.0, 3.0), 0.5, dims, F)
    assert (verts.shape[0], tris.shape[0]) == (604, 1204) and mr.closed_and_oriented(tris) and mr.euler(verts, tris) == 2


@pytest.mark.parametrize("dims", [(2, 2, 33), (33, 2, 2), (2, 33, 2)])
def test_slabs(eng, dims):
    rng = np.random.default_rng(dims[0] * 100 + dims[2])
    F = rng.normal(size=dims[::-1]).astype(np.float32)
    verts, tris = _same(eng, (0.0, 0.0, 0.0), 1.0, dims, F)
    assert tris.shape[0] > 30


def test_exact_zeros_are_outside(eng):
    """tsdf == 0 (and -0) is not inside: a crossing lies on the zero point itself (t = 0 or 1), and zeros among positives cut nothing"""
    dims = (4, 4, 3)
    rng = np.random.default_rng(6)
    F = rng.normal(size=(3, 4, 4)).astype(np.float32)
    F[rng.random(F.shape) < 0.3] = 0.0
    F[0, 0, 0], F[1, 1, 1] = -0.0, 0.0
    _same(eng, (0.0, 0.0, 0.0), 1.0, dims, F)
    G = np.abs(F)
    verts, tris = _same(eng, (0.0, 0.0, 0.0), 1.0, dims, G)
    assert verts.shape[0] == 0 and tris.shape[0] == 0
    H = np.where(F == 0, np.float32(0), np.float32(-1)).astype(np.float32)
    verts, _ = _same(eng, (2.0, 2.0, 2.0), 0.5, dims, H)
    lattice = mr.lattice_positions((2.0, 2.0, 2.0), 0.5, dims).reshape(-1, 3)
    assert verts.shape[0] > 0 and all((lattice == v).all(1).any() for v in verts), "a crossing next to an exact zero is not the zero's lattice point"


def test_sizes_caps_and_repeat(eng):
    dims = (6, 5, 4)
    F = np.random.default_rng(8).normal(size=(4, 5, 6)).astype(np.float32)
    vol = engine.make_volume((0.0, 0.0, 0.0), 1.0, dims, 1.0)
    want_v, want_t = mr.extract((0.0, 0.0, 0.0), 1.0, dims, F)
    nv0, nt0 = want_v.shape[0], want_t.shape[0]
    assert nv0 > 10 and nt0 > 10
    L, fp = eng.L, F.ctypes.data_as(C.c_void_p)
    nv, nt = C.c_int64(-1), C.c_int64(-1)

    def call(cap_v, verts, cap_t, tris):
        nv.value = nt.value = -1
        return L.mvs_engine_extract_mesh(eng.h, C.byref(vol), fp, None, cap_v, None if verts is None else verts.ctypes.data_as(C.c_void_p), cap_t,
                                         None if tris is None else tris.ctypes.data_as(C.c_void_p), C.byref(nv), C.byref(nt))

    verts, tris = np.full((nv0, 3), -7, np.float32), np.full((nt0, 3), -7, np.int32)
    # size calls: no output, one output, zero caps with outputs
    assert call(0, None, 0, None) == 0 and (nv.value, nt.value) == (nv0, nt0)
    assert call(nv0, verts, 0, None) == 0 and (nv.value, nt.value) == (nv0, nt0)
    assert call(0, None, nt0, tris) == 0 and (nv.value, nt.value) == (nv0, nt0)
    # a cap one too small: MVS_ERR_CAPACITY, the exact counts, outputs untouched
    assert call(nv0 - 1, verts, nt0, tris) == MVS_ERR_CAPACITY and (nv.value, nt.value) == (nv0, nt0)
    assert call(nv0, verts, nt0 - 1, tris) == MVS_ERR_CAPACITY and (nv.value, nt.value) == (nv0, nt0)
    assert call(0, verts, 0, tris) == MVS_ERR_CAPACITY and (nv.value, nt.value) == (nv0, nt0)
    assert (verts == -7).all() and (tris == -7).all()
    # exact caps, and larger ones: the rows behind the mesh stay
    assert call(nv0, verts, nt0, tris) == 0 and (nv.value, nt.value) == (nv0, nt0)
    assert verts.tobytes() == want_v.tobytes() and tris.tobytes() == want_t.tobytes()
    big_v, big_t = np.full((nv0 + 3, 3), -7, np.float32), np.full((nt0 + 3, 3), -7, np.int32)
    assert call(nv0 + 3, big_v, nt0 + 3, big_t) == 0
    assert big_v[:nv0].tobytes() == want_v.tobytes() and big_t[:nt0].tobytes() == want_t.tobytes() and (big_v[nv0:] == -7).all() and (big_t[nt0:] == -7).all()
    # two calls give the same bytes
    again_v, again_t = eng.extract_mesh(vol, F)
    assert again_v.tobytes() == verts.tobytes() and again_t.tobytes() == tris.tobytes()


def test_device_tensors(eng):
    """the volume and the mesh as torch device tensors: the same bytes as through host pointers"""
    import torch

    dims = (7, 6, 5)
    rng = np.random.default_rng(4)
    F = rng.normal(size=(5, 6, 7)).astype(np.float32)
    count = rng.integers(0, 3, F.shape).astype(np.int32)
    vol = engine.make_volume((0.5, 0.5, 0.5), 0.1, dims, 1.0, 1)
    want_v, want_t = _same(eng, (0.5, 0.5, 0.5), 0.1, dims, F, count)
    dev = torch.device("cuda", eng.cfg.device)
    dF, dC = torch.from_numpy(F).to(dev), torch.from_numpy(count).to(dev)
    dV = torch.zeros((want_v.shape[0], 3), dtype=torch.float32, device=dev)
    dT = torch.zeros((want_t.shape[0], 3), dtype=torch.int32, device=dev)
    nv, nt = C.c_int64(), C.c_int64()
    torch.cuda.synchronize(dev)
    eng._check(eng.L.mvs_engine_extract_mesh(eng.h, C.byref(vol), C.c_void_p(dF.data_ptr()), C.c_void_p(dC.data_ptr()), dV.shape[0], C.c_void_p(dV.data_ptr()),
                                             dT.shape[0], C.c_void_p(dT.data_ptr()), C.byref(nv), C.byref(nt)))
    assert (nv.value, nt.value) == (want_v.shape[0], want_t.shape[0]) and nv.value > 0
    assert dV.cpu().numpy().tobytes() == want_v.tobytes() and dT.cpu().numpy().tobytes() == want_t.tobytes()
