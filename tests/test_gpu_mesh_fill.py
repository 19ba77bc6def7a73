"""mvs_engine_mesh_boundaries and mvs_engine_mesh_fill on the GPU against boundaries() and fill() of tests/mesh_fill_reading.py: labels,
lengths, counts and the new triangles are integers, the centroid is an integer sum and everything else a copy of input bytes, so the
yardstick is equality of bytes, and two calls give the same bytes.  No scene: the engine has a device and no views."""
import ctypes as C

import numpy as np
import pytest

import mesh_fill_cases as mc
import mesh_fill_reading as fr
import mesh_reading as mr
from mvskit_amd import engine
from mvskit_amd.engine import MVS_ERR_ARG, MVS_ERR_CAPACITY
from scene_support import grid_mesh

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(2)
    yield e
    e.close()


def _same_boundaries(e, n_v, tris):
    got = e.mesh_boundaries(n_v, tris)
    want = fr.boundaries(n_v, tris)
    for g, w, name in zip(got, want, ("loop", "length", "n_loops", "n_complex", "n_irregular")):
        if isinstance(w, np.ndarray):
            assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), f"{name} differ from the reading"
        else:
            assert g == w, (name, g, w)
    again = e.mesh_boundaries(n_v, tris)
    assert all(np.array_equal(a, g) for a, g in zip(again, got)), "two calls give different results"
    return got


def _same(e, verts, tris, max_edges=64):
    """both calls against the reading, each twice; the boundaries of the filled mesh too"""
    before = _same_boundaries(e, verts.shape[0], tris)
    got = e.fill_holes(verts, tris, max_edges)
    want = fr.fill(verts, tris, max_edges)
    for g, w, name in zip(got[:2], want[:2], ("verts", "tris")):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), f"{name} differ from the reading"
    assert got[2] == want[2]
    again = e.fill_holes(verts, tris, max_edges)
    assert again[0].tobytes() == got[0].tobytes() and again[1].tobytes() == got[1].tobytes() and again[2] == got[2], "two calls give different bytes"
    # exactly the loops that were left, with their labels and lengths
    n_v = verts.shape[0]
    loop, length, n_loops, n_complex, n_irregular = before
    after = _same_boundaries(e, got[0].shape[0], got[1])
    gone = (length >= 3) & (length <= max_edges)
    assert after[2:] == (n_loops - got[2], n_complex, n_irregular)
    assert (after[0][:n_v] == np.where(gone, -1, loop)).all() and (after[1][:n_v] == np.where(gone, 0, length)).all() and (after[0][n_v:] == -1).all()
    return got


def _filling(max_edges=64):
    return engine.MeshFilling(max_edges, 0)


def _raw(e, f, verts, tris, cap_v, out_v, cap_t, out_t, nv, nt, nf):
    vp = C.c_void_p
    p = lambda a: None if a is None else a.ctypes.data_as(vp)  # noqa: E731
    return e.L.mvs_engine_mesh_fill(e.h, C.byref(f), verts.shape[0], p(verts), tris.shape[0], p(tris), cap_v, p(out_v), cap_t, p(out_t), C.byref(nv), C.byref(nt),
                                    None if nf is None else C.byref(nf))


def _refused(e, verts, tris, word, max_edges=64):
    out_v, out_t = np.full((verts.shape[0] + 8, 3), -7, np.float32), np.full((tris.shape[0] + 64, 3), -7, np.int32)
    nv, nt, nf = C.c_int64(-7), C.c_int64(-7), C.c_int64(-7)
    for ov, ot in ((out_v, out_t), (None, None)):  # the size call is refused too
        assert _raw(e, _filling(max_edges), verts, tris, out_v.shape[0], ov, out_t.shape[0], ot, nv, nt, nf) == MVS_ERR_ARG
        assert word in e.L.mvs_last_error(), e.L.mvs_last_error()
        assert (out_v == -7).all() and (out_t == -7).all() and (nv.value, nt.value, nf.value) == (-7, -7, -7)
    with pytest.raises(fr.Refused):
        fr.fill(verts, tris, max_edges)


# ---- the cases of the reading's test
@pytest.mark.parametrize("name", list(mc.cases()))
def test_cases_of_the_reading(eng, name):
    verts, tris, counts, lengths, max_edges, (new_v, new_t, n_filled) = mc.cases()[name]
    v, t, nf = _same(eng, verts, tris, max_edges)
    assert (v.shape[0] - verts.shape[0], t.shape[0] - tris.shape[0], nf) == (new_v, new_t, n_filled)
    loop, length, *got = eng.mesh_boundaries(verts.shape[0], tris)
    assert tuple(got) == counts and mc.component_lengths(loop, length) == lengths
    if name in ("one_triangle_out", "two_rings_out", "two_adjacent_rings_out"):
        assert mr.closed_and_oriented(t) and eng.mesh_boundaries(v.shape[0], t)[2:] == (0, 0, 0)
    if name == "grid_rim_filled":
        assert v[-1].tolist() == [34.5, 34.5, 0.0]


@pytest.mark.parametrize("name", ["one_triangle_out", "two_rings_out", "two_adjacent_rings_out", "two_holes_meet_in_a_vertex", "first_triangle_twice", "fin"])
def test_sphere_shuffled(eng, name):
    verts, tris, _, _, max_edges, _ = mc.cases()[name]
    shuffled = tris[np.random.default_rng(72).permutation(tris.shape[0])]
    a, b = _same(eng, verts, tris, max_edges), _same(eng, verts, shuffled, max_edges)
    n_t = tris.shape[0]
    assert a[0].tobytes() == b[0].tobytes() and a[1][n_t:].tobytes() == b[1][n_t:].tobytes() and a[2] == b[2]
    for x, y in zip(eng.mesh_boundaries(verts.shape[0], tris), eng.mesh_boundaries(verts.shape[0], shuffled)):
        assert np.array_equal(x, y)


# ---- basic shapes
def test_no_triangles_and_no_vertices(eng):
    verts = np.random.default_rng(73).normal(size=(700, 3)).astype(np.float32)
    none = np.zeros((0, 3), np.int32)
    v, t, nf = _same(eng, verts, none)
    assert v.tobytes() == verts.tobytes() and t.shape == (0, 3) and nf == 0
    loop, length, *counts = eng.mesh_boundaries(700, none)
    assert (loop == -1).all() and (length == 0).all() and counts == [0, 0, 0]
    v, t, nf = _same(eng, np.zeros((0, 3), np.float32), none)
    assert v.shape == (0, 3) and t.shape == (0, 3) and nf == 0


def test_one_triangle_gets_its_mirror_image(eng):
    verts = np.array([[0.5, 0.5, 0.0], [1.5, 0.5, 0.0], [0.5, 1.5, 0.0]], np.float32)
    for tri, mirror in (([0, 1, 2], [1, 0, 2]), ([2, 1, 0], [2, 0, 1]), ([1, 2, 0], [1, 0, 2])):
        v, t, nf = _same(eng, verts, np.array([tri], np.int32))
        assert nf == 1 and v.tobytes() == verts.tobytes() and t.tolist() == [tri, mirror] and mr.closed_and_oriented(t)


def test_repeated_ids_change_nothing(eng):
    verts, tris = grid_mesh(9, 7, np.random.default_rng(74).normal(size=(7, 9)))
    more = np.concatenate([[[3, 3, 5]], tris[:40], [[1, 1, 1], [8, 2, 8]], tris[40:], [[60, 61, 61]]]).astype(np.int32)
    a, b = _same(eng, verts, tris), _same(eng, verts, more)
    assert a[2] == b[2] == 1 and a[0].tobytes() == b[0].tobytes() and b[1][:more.shape[0]].tobytes() == more.tobytes()
    assert a[1][tris.shape[0]:].tobytes() == b[1][more.shape[0]:].tobytes()
    for x, y in zip(eng.mesh_boundaries(63, tris), eng.mesh_boundaries(63, more)):
        assert np.array_equal(x, y)


# ---- contention
def test_the_fan_of_the_decimation_test(eng):
    """19 999 sums on one row and one root"""
    verts, tris = mc.fan()
    loop, length, *counts = _same_boundaries(eng, verts.shape[0], tris)
    assert counts == [1, 0, 0] and loop[0] == -1 and (loop[1:] == 1).all() and (length[1:] == 19999).all()
    v, t, nf = _same(eng, verts, tris, 64)
    assert nf == 0 and v.tobytes() == verts.tobytes() and t.tobytes() == tris.tobytes()
    v, t, nf = _same(eng, verts, tris, 1 << 30)
    assert nf == 1 and v.shape[0] == 20001 and t.shape[0] == 2 * 19999 and mr.closed_and_oriented(t)


# ---- positions
def test_non_finite_positions(eng):
    verts, tris, *_ = mc.cases()["two_rings_out"]
    loop, length, *_ = fr.boundaries(verts.shape[0], tris)
    on_loop, interior = int(np.flatnonzero(loop >= 0)[3]), int(np.flatnonzero(loop < 0)[0])
    want = fr.fill(verts, tris)
    for k, bad in enumerate((np.nan, np.inf, -np.inf)):
        w = verts.copy()
        w[on_loop, k] = bad
        _refused(eng, w, tris, b"loop vertex")
        assert _same(eng, w, tris, 5)[2] == 0  # a loop too long to fill
        w = verts.copy()
        w[[500, interior], k] = bad  # an unused vertex and an interior one
        got = _same(eng, w, tris)
        assert got[0][verts.shape[0]:].tobytes() == want[0][verts.shape[0]:].tobytes() and got[1].tobytes() == want[1].tobytes()
    # on a loop of 3 that gets its triangle back: refused all the same
    verts, tris, *_ = mc.cases()["one_triangle_out"]
    w = verts.copy()
    w[mc.sphere()[1][100][2], 0] = np.nan
    _refused(eng, w, tris, b"loop vertex")


def test_zeros_of_either_sign_give_plus_zero(eng):
    verts = np.array([[0.0, -0.0, 0.0], [-0.0, -0.0, -0.0], [0.0, 0.0, 0.0], [-0.0, 0.0, -0.0], [5.0, 5.0, 5.0]], np.float32)
    tris = np.array([[0, 1, 4], [1, 2, 4], [2, 3, 4], [3, 0, 4]], np.int32)
    v, t, nf = _same(eng, verts, tris)
    assert nf == 1 and v[5].tobytes() == np.zeros(3, np.float32).tobytes() and mr.closed_and_oriented(t)
    # beside a loop that is not at the origin: M > 0, the sums of this one are 0
    both_v = np.concatenate([verts, verts + np.float32(3.0)]).astype(np.float32)
    both_v[9] = (-50.0, 0.0, 0.0)
    v, t, nf = _same(eng, both_v, np.concatenate([tris, tris + 5]).astype(np.int32))
    assert nf == 2 and v[10].tobytes() == np.zeros(3, np.float32).tobytes() and v[11].tolist() == [3.0, 3.0, 3.0]


def test_a_bad_id_is_refused_before_a_bad_loop_vertex(eng):
    verts, tris, *_ = mc.cases()["two_rings_out"]
    on_loop = int(np.flatnonzero(fr.boundaries(verts.shape[0], tris)[0] >= 0)[0])
    for where, value in ((0, verts.shape[0]), (tris.shape[0] - 1, -1), (300, 1 << 30)):
        t = tris.copy()
        t[where, 2] = value
        _refused(eng, verts, t, b"index")
        w = verts.copy()
        w[on_loop, 1] = np.nan
        _refused(eng, w, t, b"index")
        loop, length = np.full(verts.shape[0], -7, np.int32), np.full(verts.shape[0], -7, np.int32)
        words = [C.c_int64(-7) for _ in range(3)]
        vp = C.c_void_p
        assert eng.L.mvs_engine_mesh_boundaries(eng.h, verts.shape[0], t.shape[0], t.ctypes.data_as(vp), loop.ctypes.data_as(vp), length.ctypes.data_as(vp),
                                                *(C.byref(x) for x in words)) == MVS_ERR_ARG and b"index" in eng.L.mvs_last_error()
        assert (loop == -7).all() and (length == -7).all() and [x.value for x in words] == [-7] * 3


# ---- sizes and buffers
def test_size_call_and_caps_one_too_small(eng):
    verts, tris, *_ = mc.cases()["two_rings_out"]
    want_v, want_t, want_f = fr.fill(verts, tris)
    nv0, nt0 = want_v.shape[0], want_t.shape[0]
    f = _filling()
    out_v, out_t = np.full((nv0, 3), -7, np.float32), np.full((nt0, 3), -7, np.int32)
    nv, nt, nf = C.c_int64(-7), C.c_int64(-7), C.c_int64(-7)
    # the size call in its three forms: the exact counts and nothing else
    for ov, ot in ((None, None), (out_v, None), (None, out_t)):
        nv.value = nt.value = nf.value = -7
        assert _raw(eng, f, verts, tris, nv0, ov, nt0, ot, nv, nt, nf) == 0
        assert (nv.value, nt.value, nf.value) == (nv0, nt0, want_f) and (out_v == -7).all() and (out_t == -7).all()
    for cap_v, cap_t in ((nv0 - 1, nt0), (nv0, nt0 - 1), (0, 0)):
        nv.value = nt.value = nf.value = -7
        assert _raw(eng, f, verts, tris, cap_v, out_v, cap_t, out_t, nv, nt, nf) == MVS_ERR_CAPACITY and b"cap" in eng.L.mvs_last_error()
        assert (nv.value, nt.value, nf.value) == (nv0, nt0, want_f) and (out_v == -7).all() and (out_t == -7).all()
    assert _raw(eng, f, verts, tris, nv0, out_v, nt0, out_t, nv, nt, None) == 0  # without n_filled
    assert out_v.tobytes() == want_v.tobytes() and out_t.tobytes() == want_t.tobytes()
    # caps larger than the mesh: the rows beyond it stay
    big_v, big_t = np.full((nv0 + 3, 3), -7, np.float32), np.full((nt0 + 3, 3), -7, np.int32)
    assert _raw(eng, f, verts, tris, nv0 + 3, big_v, nt0 + 3, big_t, nv, nt, nf) == 0
    assert big_v[:nv0].tobytes() == want_v.tobytes() and big_t[:nt0].tobytes() == want_t.tobytes() and (big_v[nv0:] == -7).all() and (big_t[nt0:] == -7).all()
    # every output of mvs_engine_mesh_boundaries may be null
    vp = C.c_void_p
    assert eng.L.mvs_engine_mesh_boundaries(eng.h, verts.shape[0], tris.shape[0], tris.ctypes.data_as(vp), None, None, None, None, None) == 0
    n = C.c_int64(-7)
    assert eng.L.mvs_engine_mesh_boundaries(eng.h, verts.shape[0], tris.shape[0], tris.ctypes.data_as(vp), None, None, C.byref(n), None, None) == 0 and n.value == 2


def test_device_tensors(eng):
    import torch

    verts, tris, *_ = mc.cases()["two_adjacent_rings_out"]
    verts, tris = np.ascontiguousarray(verts), np.ascontiguousarray(tris)
    want = _same(eng, verts, tris)
    wl = fr.boundaries(verts.shape[0], tris)
    dev = torch.device("cuda", eng.cfg.device)
    dV, dT = torch.from_numpy(verts.copy()).to(dev), torch.from_numpy(tris.copy()).to(dev)
    oV = torch.zeros(want[0].shape, dtype=torch.float32, device=dev)
    oT = torch.zeros(want[1].shape, dtype=torch.int32, device=dev)
    oL = torch.zeros(verts.shape[0], dtype=torch.int32, device=dev)
    oN = torch.zeros(verts.shape[0], dtype=torch.int32, device=dev)
    nv, nt, nf = C.c_int64(), C.c_int64(), C.c_int64()
    f = _filling()
    vp = C.c_void_p
    torch.cuda.synchronize(dev)
    eng._check(eng.L.mvs_engine_mesh_fill(eng.h, C.byref(f), verts.shape[0], vp(dV.data_ptr()), tris.shape[0], vp(dT.data_ptr()), oV.shape[0], vp(oV.data_ptr()),
                                          oT.shape[0], vp(oT.data_ptr()), C.byref(nv), C.byref(nt), C.byref(nf)))
    assert (nv.value, nt.value, nf.value) == (want[0].shape[0], want[1].shape[0], want[2])
    assert oV.cpu().numpy().tobytes() == want[0].tobytes() and oT.cpu().numpy().tobytes() == want[1].tobytes()
    eng._check(eng.L.mvs_engine_mesh_boundaries(eng.h, verts.shape[0], tris.shape[0], vp(dT.data_ptr()), vp(oL.data_ptr()), vp(oN.data_ptr()), None, None, None))
    assert oL.cpu().numpy().tobytes() == wl[0].tobytes() and oN.cpu().numpy().tobytes() == wl[1].tobytes()


# ---- with the other mesh calls
def test_the_other_mesh_calls_accept_the_output(eng):
    verts, tris, *_ = mc.cases()["two_rings_out"]
    v, t, nf = eng.fill_holes(verts, tris)
    normals = eng.mesh_normals(v, t)
    used = np.zeros(v.shape[0], bool)
    used[t.reshape(-1)] = True
    assert used[verts.shape[0]:].all() and np.allclose(np.linalg.norm(normals[used], axis=1), 1.0, atol=1e-6)
    # a closed, outward-oriented sphere: the normals point away from its centre, at the new vertices too
    assert (np.einsum("ij,ij->i", normals[used], v[used] - mc.CENTRE) > 0).all()
    label, ntris, n = eng.mesh_components(v.shape[0], t)
    assert n == 1 and (label[used] == 0).all() and (ntris[used] == t.shape[0]).all()
    s = eng.smooth_mesh(v, t, 2)
    assert s.shape == v.shape and np.isfinite(s[used]).all() and s[~used].tobytes() == v[~used].tobytes()
    dv, dt, dmap = eng.decimate_mesh(v, t, 2.0)
    assert 0 < dv.shape[0] < v.shape[0] and 0 < dt.shape[0] < t.shape[0] and (dmap[~used] == -1).all()
