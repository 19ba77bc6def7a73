"""mvs_engine_mesh_prune on the GPU against prune() of tests/mesh_clean_reading.py: what stays keeps its order and its bytes, the new ids
come from scans, so the yardstick is equality of bytes.  No scene: the engine has a device and no views."""
import ctypes as C

import numpy as np
import pytest

import mesh_clean_reading as cr
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


@pytest.fixture(scope="module")
def spheres(eng):
    """one large and two small spheres in a 24 x 20 x 20 lattice, apart from each other: (verts, tris, label, ntris)"""
    dims = (24, 20, 20)
    F = np.minimum(mr.sphere_volume(dims, [(8.3, 9.6, 10.2)], 6.2), mr.sphere_volume(dims, [(19.4, 5.3, 5.6), (19.6, 14.2, 14.4)], 2.3))
    verts, tris = eng.extract_mesh(engine.make_volume((0.0, 0.0, 0.0), 1.0, dims, 1.0), F)
    label, ntris, n = eng.mesh_components(verts.shape[0], tris)
    assert n == 3
    return verts, tris, label, ntris


def _same(e, verts, tris, **kw):
    got = e.prune_mesh(verts, tris, **kw)
    want = cr.prune(verts, tris, **kw)
    for g, w, name in zip(got, want, ("verts", "tris", "vmap")):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert g.tobytes() == w.tobytes(), f"{name} differ from the reading"
    again = e.prune_mesh(verts, tris, **kw)
    assert all(a.tobytes() == g.tobytes() for a, g in zip(again, got)), "two calls give different bytes"
    return got


def test_small_spheres_go(eng, spheres):
    verts, tris, label, ntris = spheres
    sizes = np.unique(ntris[ntris > 0])
    small, large = int(sizes[:-1].max()), int(sizes[-1])
    assert sizes.shape[0] in (2, 3) and small < large
    pv, pt, vmap = _same(eng, verts, tris, min_triangles=small + 1)
    assert pt.shape[0] == large and mr.closed_and_oriented(pt) and mr.euler(pv, pt) == 2
    big = label[np.argmax(ntris)]
    assert ((vmap >= 0) == (label == big)).all()
    lv, lt, lmap = _same(eng, verts, tris, largest_only=True)
    assert lv.tobytes() == pv.tobytes() and lt.tobytes() == pt.tobytes() and lmap.tobytes() == vmap.tobytes()
    # nothing to drop any more
    qv, qt, qmap = _same(eng, pv, pt, min_triangles=large)
    assert qv.tobytes() == pv.tobytes() and qt.tobytes() == pt.tobytes() and (qmap == np.arange(pv.shape[0])).all()


def test_min_triangles_1_removes_exactly_the_unused_vertices(eng, spheres):
    verts, tris, label, ntris = spheres
    loose = np.random.default_rng(41).normal(size=(5, 3)).astype(np.float32)
    more = np.concatenate([loose[:2], verts, loose[2:]])
    pv, pt, vmap = _same(eng, more, tris + 2, min_triangles=1)
    used = np.zeros(more.shape[0], bool)
    used[np.unique(tris + 2)] = True
    assert ((vmap >= 0) == used).all() and pt.shape[0] == tris.shape[0] and pv.shape[0] == int(used.sum()) <= verts.shape[0]


def test_threshold_above_everything_gives_an_empty_mesh(eng, spheres):
    verts, tris, label, ntris = spheres
    for kw in (dict(min_triangles=int(ntris.max()) + 1), dict(min_triangles=1 << 40, largest_only=True)):
        pv, pt, vmap = _same(eng, verts, tris, **kw)
        assert pv.shape == (0, 3) and pt.shape == (0, 3) and (vmap == -1).all()
    pv, pt, vmap = _same(eng, verts, np.zeros((0, 3), np.int32), largest_only=True)
    assert pv.shape == (0, 3) and pt.shape == (0, 3) and (vmap == -1).all()
    pv, pt, vmap = _same(eng, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    assert pv.shape == (0, 3) and vmap.shape == (0,)


def test_a_tie_keeps_the_smaller_label(eng):
    """two equal 70 x 70 grids, the second listed first; in 20 and 38 blocks"""
    rng = np.random.default_rng(42)
    v, g = grid_mesh(70, 70, rng.normal(size=(70, 70)))
    verts = np.concatenate([v, v + np.float32(100)])
    tris = np.concatenate([g + 4900, g]).astype(np.int32)
    tris = tris[rng.permutation(tris.shape[0])]
    pv, pt, vmap = _same(eng, verts, tris, largest_only=True)
    assert pv.tobytes() == v.tobytes() and (vmap[:4900] == np.arange(4900)).all() and (vmap[4900:] == -1).all()
    assert pt.tobytes() == tris[tris[:, 0] < 4900].tobytes()
    # one triangle more on the second: it wins
    verts2 = np.concatenate([verts, [[0, 0, 0]]]).astype(np.float32)
    tris2 = np.concatenate([tris, [[9799, 9800, 9798]]]).astype(np.int32)
    pv, pt, vmap = _same(eng, verts2, tris2, largest_only=True)
    assert (vmap[:4900] == -1).all() and (vmap[4900:] == np.arange(4901)).all()


def test_size_call_and_caps_one_too_small(eng, spheres):
    verts, tris, label, ntris = spheres
    want_v, want_t, want_map = cr.prune(verts, tris, 1, True)
    nv0, nt0 = want_v.shape[0], want_t.shape[0]
    p = engine.MeshPruning(1, 1, 0)
    vp = C.c_void_p
    out_v, out_t = np.full((nv0, 3), -7, np.float32), np.full((nt0, 3), -7, np.int32)
    vmap = np.full(verts.shape[0], -7, np.int32)
    nv, nt = C.c_int64(-7), C.c_int64(-7)

    def call(cap_v, ov, cap_t, ot):
        return eng.L.mvs_engine_mesh_prune(eng.h, C.byref(p), verts.shape[0], verts.ctypes.data_as(vp), tris.shape[0], tris.ctypes.data_as(vp), cap_v,
                                           None if ov is None else ov.ctypes.data_as(vp), cap_t, None if ot is None else ot.ctypes.data_as(vp),
                                           vmap.ctypes.data_as(vp), C.byref(nv), C.byref(nt))

    # the size call in its three forms: the exact counts and nothing else
    for ov, ot in ((None, None), (out_v, None), (None, out_t)):
        nv.value = nt.value = -7
        assert call(nv0, ov, nt0, ot) == 0
        assert (nv.value, nt.value) == (nv0, nt0) and (out_v == -7).all() and (out_t == -7).all() and (vmap == -7).all()
    for cap_v, cap_t in ((nv0 - 1, nt0), (nv0, nt0 - 1), (0, 0)):
        nv.value = nt.value = -7
        assert call(cap_v, out_v, cap_t, out_t) == MVS_ERR_CAPACITY and b"cap" in eng.L.mvs_last_error()
        assert (nv.value, nt.value) == (nv0, nt0) and (out_v == -7).all() and (out_t == -7).all() and (vmap == -7).all()
    assert call(nv0, out_v, nt0, out_t) == 0
    assert out_v.tobytes() == want_v.tobytes() and out_t.tobytes() == want_t.tobytes() and vmap.tobytes() == want_map.tobytes()


def test_normals_of_the_pruned_mesh_are_the_kept_rows(eng, spheres):
    verts, tris, label, ntris = spheres
    full = eng.mesh_normals(verts, tris)
    small = int(np.unique(ntris[ntris > 0])[0])
    for kw in (dict(min_triangles=1), dict(min_triangles=small + 1), dict(largest_only=True)):
        pv, pt, vmap = eng.prune_mesh(verts, tris, **kw)
        assert eng.mesh_normals(pv, pt).tobytes() == full[vmap >= 0].tobytes(), kw


def test_a_bad_id_is_refused_and_nothing_written(eng):
    verts, tris = grid_mesh(20, 20)
    out_v, out_t, vmap = np.full((400, 3), -7, np.float32), np.full(tris.shape, -7, np.int32), np.full(400, -7, np.int32)
    nv, nt = C.c_int64(-7), C.c_int64(-7)
    p = engine.MeshPruning(1, 0, 0)
    vp = C.c_void_p
    for where, value in ((0, 400), (tris.shape[0] - 1, -1), (300, 1 << 30)):
        t = tris.copy()
        t[where, 2] = value
        assert eng.L.mvs_engine_mesh_prune(eng.h, C.byref(p), 400, verts.ctypes.data_as(vp), t.shape[0], t.ctypes.data_as(vp), 400, out_v.ctypes.data_as(vp),
                                           t.shape[0], out_t.ctypes.data_as(vp), vmap.ctypes.data_as(vp), C.byref(nv), C.byref(nt)) == MVS_ERR_ARG
        assert b"index" in eng.L.mvs_last_error(), (where, value)
        assert (out_v == -7).all() and (out_t == -7).all() and (vmap == -7).all() and (nv.value, nt.value) == (-7, -7)


def test_device_tensors(eng):
    import torch

    rng = np.random.default_rng(43)
    v, g = grid_mesh(33, 17, rng.normal(size=(17, 33)))
    verts = np.concatenate([v, v[:100] + np.float32(50)])
    tris = np.concatenate([g, g[:30] + 561]).astype(np.int32)
    want = _same(eng, verts, tris, min_triangles=31)
    dev = torch.device("cuda", eng.cfg.device)
    dV, dT = torch.from_numpy(verts).to(dev), torch.from_numpy(tris).to(dev)
    oV = torch.zeros(want[0].shape, dtype=torch.float32, device=dev)
    oT = torch.zeros(want[1].shape, dtype=torch.int32, device=dev)
    oM = torch.zeros(verts.shape[0], dtype=torch.int32, device=dev)
    nv, nt = C.c_int64(), C.c_int64()
    p = engine.MeshPruning(31, 0, 0)
    torch.cuda.synchronize(dev)
    vp = C.c_void_p
    eng._check(eng.L.mvs_engine_mesh_prune(eng.h, C.byref(p), verts.shape[0], vp(dV.data_ptr()), tris.shape[0], vp(dT.data_ptr()), oV.shape[0], vp(oV.data_ptr()),
                                           oT.shape[0], vp(oT.data_ptr()), vp(oM.data_ptr()), C.byref(nv), C.byref(nt)))
    assert (nv.value, nt.value) == (want[0].shape[0], want[1].shape[0])
    assert oV.cpu().numpy().tobytes() == want[0].tobytes() and oT.cpu().numpy().tobytes() == want[1].tobytes() and oM.cpu().numpy().tobytes() == want[2].tobytes()
