"""Engine.coloured_mesh with the clean-up switched on, on the smallest plane scene of tests/test_gpu_mesh_tsdf.py (3 views of 96 x 64 on
the textured plane, csize 2): the chain mesh -> prune -> smooth -> normals -> colours equals the five calls made by hand, the defaults
give the bytes of the chain without clean-up, and nothing of the engine's state moves."""
import numpy as np
import pytest

import mesh_clean_reading as cr
from maps_reading import DEPTH_TOL, NORMAL_COS
from mvskit_amd import synth
from scene_support import PLAIN, cached_scene, engine_with_pool, lattice

pytestmark = pytest.mark.gpu
KW = dict(min_consistent=1, depth_tol=DEPTH_TOL, normal_cos=NORMAL_COS)
CKW = dict(occl_tol=DEPTH_TOL, min_cos=0.1, **KW)


def _bytes(arrays):
    return [a.tobytes() for a in arrays]


def test_coloured_mesh_with_clean_up():
    sc = cached_scene(3, 96, 64, 30.0)
    sizes = [(sc.W, sc.H)] * sc.nviews
    seeds = synth.make_seeds(sc, PLAIN["level"], PLAIN["csize"], stride=1)
    e = engine_with_pool(sc, PLAIN, None, sizes, None, seeds)
    alive, thr = e.patches(), e.thresholds()
    vol = lattice(sc, PLAIN["level"])

    # today's chain, and the defaults
    verts, tris = e.mesh(vol, **KW)
    normals = e.mesh_normals(verts, tris)
    rgb, used = e.mesh_colours(verts, normals, **CKW)
    assert verts.shape[0] > 256 and tris.shape[0] > 256
    assert _bytes(e.coloured_mesh(vol, **CKW)) == _bytes((verts, tris, normals, rgb, used))
    assert _bytes(e.coloured_mesh(vol, min_triangles=0, largest_only=False, smooth_iterations=0, **CKW)) == _bytes((verts, tris, normals, rgb, used))

    # the five calls by hand; k drops everything but the components of at least half the largest one's size
    label, ntris, n = e.mesh_components(verts.shape[0], tris)
    assert n >= 1 and label.tobytes() == cr.components(verts.shape[0], tris)[0].tobytes()
    k = max(2, int(ntris.max()) // 2)
    pv, pt, vmap = e.prune_mesh(verts, tris, min_triangles=k)
    assert 0 < pt.shape[0] <= tris.shape[0] and pv.shape[0] <= verts.shape[0]
    assert _bytes((pv, pt, vmap)) == _bytes(cr.prune(verts, tris, k))
    sv = e.smooth_mesh(pv, pt, 2)
    assert sv.tobytes() == cr.smooth_exact(pv, pt, 2).tobytes() and sv.tobytes() != pv.tobytes()
    sn = e.mesh_normals(sv, pt)
    srgb, sused = e.mesh_colours(sv, sn, **CKW)
    assert _bytes(e.coloured_mesh(vol, min_triangles=k, smooth_iterations=2, **CKW)) == _bytes((sv, pt, sn, srgb, sused))
    # each switch alone
    assert _bytes(e.coloured_mesh(vol, largest_only=True, **CKW)[:2]) == _bytes(e.prune_mesh(verts, tris, largest_only=True)[:2])
    assert e.coloured_mesh(vol, smooth_iterations=1, **CKW)[0].tobytes() == e.smooth_mesh(verts, tris, 1).tobytes()

    # nothing of the engine's state moved
    assert e.patches().tobytes() == alive.tobytes() and e.thresholds() == thr
    t = engine_with_pool(sc, PLAIN, None, sizes, None, seeds)
    assert t.patches().tobytes() == alive.tobytes()
    assert e.propagate(1) == t.propagate(1)
    assert e.patches().tobytes() == t.patches().tobytes()
    t.close()
    e.close()
