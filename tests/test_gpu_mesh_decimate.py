"""mvs_engine_mesh_decimate on the GPU against decimate() of tests/mesh_decimate_reading.py: clusters, kept triangles and the vertex map
are integers, the mean is an integer sum and the member placement copies bytes, so the yardstick is equality of bytes, and two calls give
the same bytes.  No scene: the engine has a device and no views."""
import ctypes as C

import numpy as np
import pytest

import mesh_decimate_reading as dr
import mesh_reading as mr
from mvskit_amd import engine
from mvskit_amd.engine import MVS_ERR_ARG, MVS_ERR_CAPACITY
from scene_support import grid_mesh

pytestmark = pytest.mark.gpu
PLACEMENTS = ("mean", "member")


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(2)
    yield e
    e.close()


@pytest.fixture(scope="module")
def sphere():
    """the sphere of the prune test alone: 2146 vertices, 4288 triangles, closed"""
    dims = (24, 20, 20)
    return mr.extract((0.0, 0.0, 0.0), 1.0, dims, mr.sphere_volume(dims, [(8.3, 9.6, 10.2)], 6.2))


def _same(e, verts, tris, cell, origin=(0.0, 0.0, 0.0), placement="mean"):
    got = e.decimate_mesh(verts, tris, cell, origin, placement)
    want = dr.decimate(verts, tris, cell, origin, placement)
    for g, w, name in zip(got, want, ("verts", "tris", "vmap")):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), f"{name} differ from the reading"
    again = e.decimate_mesh(verts, tris, cell, origin, placement)
    assert all(a.tobytes() == g.tobytes() for a, g in zip(again, got)), "two calls give different bytes"
    return got


def _both(e, verts, tris, cell, origin=(0.0, 0.0, 0.0)):
    return [_same(e, verts, tris, cell, origin, p) for p in PLACEMENTS]


def _decimation(cell, origin=(0.0, 0.0, 0.0), placement=0):
    return engine.MeshDecimation((C.c_float * 3)(*origin), cell, placement, 0)


def _raw(e, d, verts, tris, cap_v, out_v, cap_t, out_t, vmap, nv, nt):
    vp = C.c_void_p
    p = lambda a: None if a is None else a.ctypes.data_as(vp)  # noqa: E731
    return e.L.mvs_engine_mesh_decimate(e.h, C.byref(d), verts.shape[0], p(verts), tris.shape[0], p(tris), cap_v, p(out_v), cap_t, p(out_t), p(vmap),
                                        C.byref(nv), C.byref(nt))


def _refused(e, verts, tris, cell, word, status=MVS_ERR_ARG):
    out_v, out_t, vmap = np.full((verts.shape[0], 3), -7, np.float32), np.full(tris.shape, -7, np.int32), np.full(verts.shape[0], -7, np.int32)
    nv, nt = C.c_int64(-7), C.c_int64(-7)
    for placement in (0, 1):
        assert _raw(e, _decimation(cell, placement=placement), verts, tris, verts.shape[0], out_v, tris.shape[0], out_t, vmap, nv, nt) == status
        assert word in e.L.mvs_last_error(), e.L.mvs_last_error()
        assert (out_v == -7).all() and (out_t == -7).all() and (vmap == -7).all() and (nv.value, nt.value) == (-7, -7)
    with pytest.raises(dr.Refused):
        dr.decimate(verts, tris, cell)


TRIANGLE = np.array([[0.5, 0.5, 0.0], [1.5, 0.5, 0.0], [0.5, 1.5, 0.0]], np.float32)
ONE = np.array([[0, 1, 2]], np.int32)


# ---- basic shapes
def test_one_triangle_in_three_cells_and_in_one(eng):
    for v, t, vmap in _both(eng, TRIANGLE, ONE, 1.0):
        assert v.tobytes() == TRIANGLE.tobytes() and t.tolist() == [[0, 1, 2]] and vmap.tolist() == [0, 1, 2]
    for v, t, vmap in _both(eng, TRIANGLE, ONE, 10.0):
        assert v.shape == (0, 3) and t.shape == (0, 3) and vmap.tolist() == [-1, -1, -1]


def test_no_triangles_and_no_vertices(eng):
    verts = np.random.default_rng(61).normal(size=(700, 3)).astype(np.float32)
    for v, t, vmap in _both(eng, verts, np.zeros((0, 3), np.int32), 0.5):
        assert v.shape == (0, 3) and t.shape == (0, 3) and vmap.shape == (700,) and (vmap == -1).all()
    for v, t, vmap in _both(eng, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), 0.5):
        assert v.shape == (0, 3) and t.shape == (0, 3) and vmap.shape == (0,)


# ---- the sphere
@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("cell,n_v,n_t", [(2.0, 184, 364), (3.0, 84, 164), (1.5, 285, 569), (0.01, 2138, 4272)])
def test_sphere(eng, sphere, cell, n_v, n_t, placement):
    v, t, vmap = _same(eng, *sphere, cell, placement=placement)
    assert (v.shape[0], t.shape[0]) == (n_v, n_t)
    assert mr.closed_and_oriented(t) == (cell != 1.5)


@pytest.mark.parametrize("cell", [1.5, 2.0])
def test_sphere_shuffled(eng, sphere, cell):
    verts, tris = sphere
    shuffled = tris[np.random.default_rng(62).permutation(tris.shape[0])]
    for placement in PLACEMENTS:
        a = _same(eng, verts, tris, cell, placement=placement)
        b = _same(eng, verts, shuffled, cell, placement=placement)  # the reading's bytes for that order
        assert a[0].tobytes() == b[0].tobytes() and a[2].tobytes() == b[2].tobytes() and a[1].shape == b[1].shape


# ---- grid addressing
def test_grid_with_negative_indices_and_far_from_the_origin(eng):
    rng = np.random.default_rng(63)
    verts, tris = grid_mesh(70, 70, rng.normal(size=(70, 70)))
    origin = (-0.7, 0.4, 0.0)
    g = dr.cells(verts, origin, 3.3)
    assert g[:, 0].min() == 0 and g[:, 1].min() == -1 and g[:, 2].min() < 0 < g[:, 2].max()
    near = _both(eng, verts, tris, 3.3, origin)
    assert 300 < near[0][0].shape[0] < 4900
    moved = verts + np.array([1e4, -1e4, 1e4], np.float32)
    far = _both(eng, moved, tris, 3.3, origin)
    assert dr.cells(moved, origin, 3.3)[:, 1].max() < -3000 and 300 < far[0][0].shape[0] < 4900


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_cells_that_differ_in_one_axis_are_two_clusters(eng, axis):
    for base in ((0.5, 0.5, 0.5), (-3.5, 2.5, 1000.5), (1047.5, -1048.5, 2047.5)):
        verts = np.array([base, base, (5.5, 7.5, 9.5)], np.float32)
        verts[1, axis] += 1.0
        for v, t, vmap in _both(eng, verts, ONE, 1.0):
            assert v.tobytes() == verts.tobytes() and t.tolist() == [[0, 1, 2]]


def test_the_ends_of_the_grid(eng):
    lo, hi = np.float32(-(1 << 20)) + np.float32(0.5), np.float32((1 << 20) - 1) + np.float32(0.5)
    verts = np.array([[lo, 0.5, 0.5], [0.5, hi, 0.5], [0.5, 0.5, lo], [hi, hi, hi], [lo, lo, lo], [hi, lo, 0.5]], np.float32)
    tris = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    g = dr.cells(verts, (0, 0, 0), 1.0)
    assert g.min() == -(1 << 20) and g.max() == (1 << 20) - 1
    for v, t, vmap in _both(eng, verts, tris, 1.0):
        assert v.tobytes() == verts.tobytes() and t.tobytes() == tris.tobytes()
    # one cell beyond either end, a NaN and an infinity on a member: refused, nothing written
    for k, value in ((0, lo - 1), (4, hi + 1), (8, np.nan), (10, np.inf), (17, -np.inf)):
        w = verts.copy()
        w.reshape(-1)[k] = value
        _refused(eng, w, tris, 1.0, b"member")
    # the same on a vertex no triangle names: ignored
    for value in (np.nan, np.inf, lo - 1):
        w = np.concatenate([verts, [[0.5, value, 0.5]]]).astype(np.float32)
        for v, t, vmap in _both(eng, w, tris, 1.0):
            assert v.tobytes() == verts.tobytes() and vmap.tolist() == [0, 1, 2, 3, 4, 5, -1]


def test_an_unused_vertex_does_not_move_the_mean(eng):
    verts, tris = grid_mesh(12, 9, np.random.default_rng(64).normal(size=(9, 12)))
    more = np.concatenate([verts[:50], [[9.9, 6.9, 3.9]], verts[50:]]).astype(np.float32)  # in a corner of the cell that holds most members
    tris2 = np.where(tris >= 50, tris + 1, tris).astype(np.int32)
    origin = (-50.0, -5.0, -50.0)
    g = dr.cells(more, origin, 6.0)
    assert int((g == g[50]).all(axis=1).sum()) > 20
    for a, b in zip(_both(eng, verts, tris, 6.0, origin), _both(eng, more, tris2, 6.0, origin)):
        assert a[0].shape[0] > 3 and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and b[2][50] == -1


# ---- contention
def _fan(n=20000):
    """a fan around vertex 0 whose rim wobbles between radius 0.7 and 1.3"""
    a = np.linspace(0.0, 2 * np.pi, n - 1, endpoint=False)
    r = 1.0 + 0.3 * np.sin(7 * a)
    rim = np.stack([r * np.cos(a), r * np.sin(a), 0.05 * np.cos(3 * a)], 1)
    verts = np.concatenate([[[0.0, 0.0, 0.0]], rim]).astype(np.float32)
    i = np.arange(1, n)
    tris = np.stack([np.zeros(n - 1, np.int64), i, np.where(i + 1 < n, i + 1, 1)], 1).astype(np.int32)
    return verts, tris


def test_a_fan_in_one_cell_collapses(eng):
    verts, tris = _fan()
    for v, t, vmap in _both(eng, verts, tris, 10.0, (-5.0, -5.0, -5.0)):
        assert v.shape == (0, 3) and t.shape == (0, 3) and (vmap == -1).all()


def test_a_fan_in_about_a_hundred_cells(eng):
    verts, tris = _fan()
    st = {}
    dr.decimate(verts, tris, 0.1, (-5.0, -5.0, -5.0), stats=st)
    assert 60 <= st["clusters"] <= 160 and st["collapsed"] > 19000
    for v, t, vmap in _both(eng, verts, tris, 0.1, (-5.0, -5.0, -5.0)):
        assert 60 <= v.shape[0] <= 160 and t.shape[0] > 0


# ---- triangle rules
def test_repeated_ids_collapse(eng):
    verts, tris = grid_mesh(9, 7)
    more = np.concatenate([[[3, 3, 5]], tris[:40], [[1, 1, 1], [8, 2, 8]], tris[40:], [[60, 61, 61]]]).astype(np.int32)
    for v, t, vmap in _both(eng, verts, more, 0.5, (-0.25, -0.25, -0.25)):
        assert v.tobytes() == verts.tobytes() and t.tobytes() == tris.tobytes()


def test_of_two_triangles_over_the_same_cells_the_earlier_stays(eng):
    verts = np.concatenate([TRIANGLE, TRIANGLE + np.float32(0.25)])
    for tris, kept in (([[0, 1, 2], [5, 4, 3]], [0, 1, 2]), ([[5, 4, 3], [0, 1, 2]], [2, 1, 0]), ([[3, 4, 5], [1, 2, 0], [2, 1, 0]], [0, 1, 2])):
        for v, t, vmap in _both(eng, verts, np.array(tris, np.int32), 1.0):
            assert t.tolist() == [kept] and vmap.tolist() == [0, 1, 2, 0, 1, 2]
    # more of them than a wave holds, and two that share only two clusters
    many = np.array([[0, 1, 2], [3, 4, 5], [2, 4, 0]] * 100 + [[0, 1, 6], [6, 4, 3]], np.int32)
    verts7 = np.concatenate([verts, [[3.5, 3.5, 0.0]]]).astype(np.float32)
    for v, t, vmap in _both(eng, verts7, many, 1.0):
        assert t.tolist() == [[0, 1, 2], [0, 1, 3]]


# ---- placement
def test_member_placement_tie_takes_the_smaller_id(eng):
    # every cell holds two members at the same distance from their mean
    verts = np.array([[0.75, 0.5, 0.5], [1.25, 0.5, 0.5], [0.5, 1.25, 0.5], [0.25, 0.5, 0.5], [1.75, 0.5, 0.5], [0.5, 1.75, 0.5]], np.float32)
    tris = np.array([[5, 4, 3], [0, 1, 2]], np.int32)
    mean = _same(eng, verts, tris, 1.0)
    assert mean[0].tolist() == [[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5]]
    member = _same(eng, verts, tris, 1.0, placement="member")
    assert member[0].tobytes() == verts[:3].tobytes() and member[1].tolist() == [[2, 1, 0]]


def test_a_cluster_of_one_keeps_its_bytes(eng):
    sub = np.float32(1e-40)
    verts = np.array([[-0.0, sub, 0.5], [1.5, -0.0, -sub], [0.3, 1.7, -0.0], [0.1, 0.2, 0.3]], np.float32)
    assert np.signbit(verts[0, 0]) and verts[0, 1] != 0
    for v, t, vmap in _both(eng, verts, ONE, 1.0):
        assert v.tobytes() == verts[:3].tobytes() and vmap.tolist() == [0, 1, 2, -1]
    # all members zeros of either sign (M == 0): they share a cell, whatever the grid
    zeros = np.array([[0.0, -0.0, 0.0], [-0.0, -0.0, -0.0], [0.0, 0.0, 0.0]], np.float32)
    for v, t, vmap in _both(eng, zeros, ONE, 1.0):
        assert v.shape == (0, 3)


# ---- sizes and buffers
def test_size_call_and_caps_one_too_small(eng, sphere):
    verts, tris = sphere
    for placement in (0, 1):
        want_v, want_t, want_map = dr.decimate(verts, tris, 2.0, placement=PLACEMENTS[placement])
        nv0, nt0 = want_v.shape[0], want_t.shape[0]
        d = _decimation(2.0, placement=placement)
        out_v, out_t = np.full((nv0, 3), -7, np.float32), np.full((nt0, 3), -7, np.int32)
        vmap = np.full(verts.shape[0], -7, np.int32)
        nv, nt = C.c_int64(-7), C.c_int64(-7)
        # the size call in its three forms: the exact counts and nothing else
        for ov, ot in ((None, None), (out_v, None), (None, out_t)):
            nv.value = nt.value = -7
            assert _raw(eng, d, verts, tris, nv0, ov, nt0, ot, vmap, nv, nt) == 0
            assert (nv.value, nt.value) == (nv0, nt0) and (out_v == -7).all() and (out_t == -7).all() and (vmap == -7).all()
        for cap_v, cap_t in ((nv0 - 1, nt0), (nv0, nt0 - 1), (0, 0)):
            nv.value = nt.value = -7
            assert _raw(eng, d, verts, tris, cap_v, out_v, cap_t, out_t, vmap, nv, nt) == MVS_ERR_CAPACITY and b"cap" in eng.L.mvs_last_error()
            assert (nv.value, nt.value) == (nv0, nt0) and (out_v == -7).all() and (out_t == -7).all() and (vmap == -7).all()
        assert _raw(eng, d, verts, tris, nv0, out_v, nt0, out_t, None, nv, nt) == 0  # without a vertex map
        assert out_v.tobytes() == want_v.tobytes() and out_t.tobytes() == want_t.tobytes()
        assert _raw(eng, d, verts, tris, nv0, out_v, nt0, out_t, vmap, nv, nt) == 0
        assert out_v.tobytes() == want_v.tobytes() and out_t.tobytes() == want_t.tobytes() and vmap.tobytes() == want_map.tobytes()


def test_a_bad_id_is_refused_and_nothing_written(eng):
    verts, tris = grid_mesh(20, 20)
    for where, value in ((0, 400), (tris.shape[0] - 1, -1), (300, 1 << 30)):
        t = tris.copy()
        t[where, 2] = value
        _refused(eng, verts, t, 2.0, b"index")
    # a bad id is reported before a bad member
    w = verts.copy()
    w[5, 1] = np.nan
    t = tris.copy()
    t[7, 0] = 400
    _refused(eng, w, t, 2.0, b"index")


def test_device_tensors(eng):
    import torch

    rng = np.random.default_rng(65)
    verts, tris = grid_mesh(33, 17, rng.normal(size=(17, 33)))
    dev = torch.device("cuda", eng.cfg.device)
    dV, dT = torch.from_numpy(verts).to(dev), torch.from_numpy(tris).to(dev)
    vp = C.c_void_p
    for placement in (0, 1):
        want = _same(eng, verts, tris, 2.5, (0.3, 0.3, 0.3), PLACEMENTS[placement])
        oV = torch.zeros(want[0].shape, dtype=torch.float32, device=dev)
        oT = torch.zeros(want[1].shape, dtype=torch.int32, device=dev)
        oM = torch.zeros(verts.shape[0], dtype=torch.int32, device=dev)
        nv, nt = C.c_int64(), C.c_int64()
        d = _decimation(2.5, (0.3, 0.3, 0.3), placement)
        torch.cuda.synchronize(dev)
        eng._check(eng.L.mvs_engine_mesh_decimate(eng.h, C.byref(d), verts.shape[0], vp(dV.data_ptr()), tris.shape[0], vp(dT.data_ptr()), oV.shape[0],
                                                  vp(oV.data_ptr()), oT.shape[0], vp(oT.data_ptr()), vp(oM.data_ptr()), C.byref(nv), C.byref(nt)))
        assert (nv.value, nt.value) == (want[0].shape[0], want[1].shape[0])
        assert oV.cpu().numpy().tobytes() == want[0].tobytes() and oT.cpu().numpy().tobytes() == want[1].tobytes() and oM.cpu().numpy().tobytes() == want[2].tobytes()


# ---- with the other mesh calls
def test_normals_and_components_accept_the_output(eng, sphere):
    v, t, vmap = eng.decimate_mesh(*sphere, 2.0)
    normals = eng.mesh_normals(v, t)
    assert np.allclose(np.linalg.norm(normals, axis=1), 1.0, atol=1e-6)
    # a closed, outward-oriented sphere: the normals point away from its centre
    assert (np.einsum("ij,ij->i", normals, v - np.array([8.3, 9.6, 10.2], np.float32)) > 0).all()
    label, ntris, n = eng.mesh_components(v.shape[0], t)
    assert n == 1 and (label == 0).all() and (ntris == t.shape[0]).all()


def test_a_tiny_cell_is_a_prune_where_nothing_merged(eng, sphere):
    verts, tris = sphere
    pv, pt, pmap = eng.prune_mesh(verts, tris, min_triangles=1)
    dv, dt, dmap = _same(eng, verts, tris, 0.01)
    assert (pmap >= 0).all() and (dmap >= 0).all()
    rows, counts = np.unique(dmap, return_counts=True)
    alone = np.isin(dmap, rows[counts == 1])  # per input vertex: its cluster has no other member
    assert int((~alone).sum()) == int(counts[counts > 1].sum()) > 0
    assert dv[dmap[alone]].tobytes() == pv[pmap[alone]].tobytes()
    whole = alone[tris].all(axis=1)  # per input triangle: none of its corners merged
    row_alone = counts == 1
    assert dt[row_alone[dt].all(axis=1)].tobytes() == dmap[tris[whole]].tobytes()
    assert pt[whole].tobytes() == pmap[tris[whole]].tobytes()
