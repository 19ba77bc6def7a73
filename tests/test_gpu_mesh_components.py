"""mvs_engine_mesh_components on the GPU against components() of tests/mesh_clean_reading.py: labels are the smallest id of a component
and the counts are integer sums, so the yardstick is equality of bytes -- whatever order the triangles are listed in and the hardware
met them in.  No scene: the engine has a device and no views."""
import ctypes as C

import numpy as np
import pytest

import mesh_clean_reading as cr
from mvskit_amd import engine
from mvskit_amd.engine import MVS_ERR_ARG
from scene_support import grid_mesh

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(2)
    yield e
    e.close()


def _same(e, n_v, tris):
    label, ntris, n = e.mesh_components(n_v, tris)
    wl, wn, wc = cr.components(n_v, tris)
    assert label.dtype == np.int32 and ntris.dtype == np.int32
    assert label.tobytes() == wl.tobytes(), f"{int((label != wl).sum())} labels differ from the reading"
    assert ntris.tobytes() == wn.tobytes(), f"{int((ntris != wn).sum())} counts differ from the reading"
    assert n == wc
    again = e.mesh_components(n_v, tris)
    assert again[0].tobytes() == label.tobytes() and again[1].tobytes() == ntris.tobytes() and again[2] == n, "two calls differ"
    return label, ntris, n


def test_one_triangle_and_empty_meshes(eng):
    label, ntris, n = _same(eng, 3, np.array([[2, 0, 1]], np.int32))
    assert label.tolist() == [0, 0, 0] and ntris.tolist() == [1, 1, 1] and n == 1
    assert _same(eng, 0, np.zeros((0, 3), np.int32))[2] == 0
    label, ntris, n = _same(eng, 700, np.zeros((0, 3), np.int32))
    assert (label == np.arange(700)).all() and (ntris == 0).all() and n == 0


def test_strip_of_5000_triangles_in_shuffled_order(eng):
    """long parent chains over 20 blocks"""
    rng = np.random.default_rng(31)
    k = 5000
    strip = np.stack([np.arange(k), np.arange(k) + 1, np.arange(k) + 2], 1).astype(np.int32)
    label, ntris, n = _same(eng, k + 2, strip[rng.permutation(k)])
    assert (label == 0).all() and (ntris == k).all() and n == 1
    other = eng.mesh_components(k + 2, strip[rng.permutation(k)])
    assert other[0].tobytes() == label.tobytes() and other[1].tobytes() == ntris.tobytes()


def test_fan_of_20000_triangles(eng):
    """one component: every wave's count meets one word"""
    rng = np.random.default_rng(32)
    k = 20000
    i = np.arange(k)
    tris = np.stack([np.zeros(k, np.int64), 1 + i, 1 + (i + 1) % k], 1).astype(np.int32)
    label, ntris, n = _same(eng, k + 1, tris[rng.permutation(k)])
    assert (label == 0).all() and (ntris == k).all() and n == 1


def test_two_grids_apart_and_sharing_one_vertex(eng):
    _, g = grid_mesh(70, 70)
    two = np.concatenate([g, g + 4900]).astype(np.int32)
    rng = np.random.default_rng(33)
    label, ntris, n = _same(eng, 9800, two[rng.permutation(two.shape[0])])
    assert n == 2 and (label[:4900] == 0).all() and (label[4900:] == 4900).all() and (ntris == g.shape[0]).all()
    # the second grid's first vertex becomes the first grid's last: vertex 4900 is unused, the rest is one component
    joined = np.where(two == 4900, 4899, two).astype(np.int32)
    label, ntris, n = _same(eng, 9800, joined[rng.permutation(two.shape[0])])
    assert n == 1 and label[4900] == 4900 and ntris[4900] == 0 and (np.delete(label, 4900) == 0).all() and ntris[0] == 2 * g.shape[0]


def test_smallest_id_only_in_the_last_triangle(eng):
    k = 3000
    chain = np.stack([np.arange(k) + 10, np.arange(k) + 11, np.arange(k) + 12], 1)
    tris = np.concatenate([chain, [[k + 11, 4, 10]]]).astype(np.int32)
    label, ntris, n = _same(eng, k + 20, tris)
    assert (label[10:k + 12] == 4).all() and label[4] == 4 and ntris[4] == k + 1 and n == 1 and label[5] == 5


def test_repeated_ids(eng):
    tris = np.array([[0, 0, 0], [3, 3, 4], [4, 5, 4], [7, 8, 7], [8, 7, 7], [9, 9, 9], [9, 9, 9], [2, 2, 5]], np.int32)
    label, ntris, n = _same(eng, 11, tris)
    assert label.tolist() == [0, 1, 2, 2, 2, 2, 6, 7, 7, 9, 10] and ntris.tolist() == [1, 0, 3, 3, 3, 3, 0, 2, 2, 2, 0] and n == 4


def test_300_single_triangles_among_unused_vertices(eng):
    rng = np.random.default_rng(34)
    ids = rng.permutation(1900)[:900].reshape(300, 3).astype(np.int32)
    label, ntris, n = _same(eng, 1900, ids)
    assert n == 300 and int((ntris == 0).sum()) == 1000 and (label[ids] == ids.min(axis=1, keepdims=True)).all()


def test_an_id_out_of_range_is_refused_and_nothing_written(eng):
    _, tris = grid_mesh(20, 20)
    label, ntris = np.full(400, -7, np.int32), np.full(400, -7, np.int32)
    n = C.c_int64(-7)
    f = eng.L.mvs_engine_mesh_components
    vp = C.c_void_p
    for where, value in ((0, 400), (tris.shape[0] - 1, -1), (300, 1 << 30)):
        t = tris.copy()
        t[where, 1] = value
        assert f(eng.h, 400, t.shape[0], t.ctypes.data_as(vp), label.ctypes.data_as(vp), ntris.ctypes.data_as(vp), C.byref(n)) == MVS_ERR_ARG
        assert b"index" in eng.L.mvs_last_error() and (label == -7).all() and (ntris == -7).all() and n.value == -7, (where, value)
    t = np.zeros((1, 3), np.int32)  # no vertices at all: every id is out of range
    assert f(eng.h, 0, 1, t.ctypes.data_as(vp), None, None, C.byref(n)) == MVS_ERR_ARG and n.value == -7
    assert f(eng.h, 400, tris.shape[0], tris.ctypes.data_as(vp), label.ctypes.data_as(vp), None, None) == 0  # outputs may be null
    assert label.tobytes() == cr.components(400, tris)[0].tobytes() and (ntris == -7).all()


def test_device_tensors(eng):
    import torch

    _, tris = grid_mesh(33, 17)
    tris = np.concatenate([tris, tris[:40] + 600]).astype(np.int32)
    want = _same(eng, 1300, tris)
    dev = torch.device("cuda", eng.cfg.device)
    dT = torch.from_numpy(tris).to(dev)
    dL, dN = torch.zeros(1300, dtype=torch.int32, device=dev), torch.zeros(1300, dtype=torch.int32, device=dev)
    n = C.c_int64()
    torch.cuda.synchronize(dev)
    eng._check(eng.L.mvs_engine_mesh_components(eng.h, 1300, tris.shape[0], C.c_void_p(dT.data_ptr()), C.c_void_p(dL.data_ptr()), C.c_void_p(dN.data_ptr()),
                                                C.byref(n)))
    assert dL.cpu().numpy().tobytes() == want[0].tobytes() and dN.cpu().numpy().tobytes() == want[1].tobytes() and n.value == want[2]
