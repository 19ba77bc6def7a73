"""Engine.coloured_mesh with decimation switched on, on the smallest plane scene of tests/test_gpu_mesh_tsdf.py (3 views of 96 x 64 on the
textured plane, csize 2): the chain mesh -> prune -> smooth -> decimate -> normals -> colours equals the calls made by hand, the defaults
give the bytes of the chain without decimation, and nothing of the engine's state moves."""
import numpy as np
import pytest

import mesh_decimate_reading as dr
from maps_reading import DEPTH_TOL, NORMAL_COS
from mvskit_amd import engine, synth
from scene_support import PLAIN, cached_scene, engine_with_pool, lattice

pytestmark = pytest.mark.gpu
KW = dict(min_consistent=1, depth_tol=DEPTH_TOL, normal_cos=NORMAL_COS)
CKW = dict(occl_tol=DEPTH_TOL, min_cos=0.1, **KW)


def _bytes(arrays):
    return [a.tobytes() for a in arrays]


def test_coloured_mesh_with_decimation():
    sc = cached_scene(3, 96, 64, 30.0)
    sizes = [(sc.W, sc.H)] * sc.nviews
    seeds = synth.make_seeds(sc, PLAIN["level"], PLAIN["csize"], stride=1)
    e = engine_with_pool(sc, PLAIN, None, sizes, None, seeds)
    alive, thr = e.patches(), e.thresholds()
    vol = lattice(sc, PLAIN["level"])
    voxel = np.float32(vol.voxel)
    cell = float(2 * voxel)
    origin = tuple(float(np.float32(vol.origin[k]) - voxel / np.float32(2)) for k in range(3))
    assert engine.decimation_origin(vol) == origin

    # today's chain, and the defaults
    verts, tris = e.mesh(vol, **KW)
    normals = e.mesh_normals(verts, tris)
    rgb, used = e.mesh_colours(verts, normals, **CKW)
    assert verts.shape[0] > 256 and tris.shape[0] > 256
    assert _bytes(e.coloured_mesh(vol, **CKW)) == _bytes((verts, tris, normals, rgb, used))
    assert _bytes(e.coloured_mesh(vol, decimate_cell=0.0, decimate_placement="member", **CKW)) == _bytes((verts, tris, normals, rgb, used))

    # decimation alone, by hand, both placements
    for placement in ("mean", "member"):
        dv, dt, dmap = e.decimate_mesh(verts, tris, cell, origin, placement)
        assert _bytes((dv, dt, dmap)) == _bytes(dr.decimate(verts, tris, cell, origin, placement))
        assert 0 < dv.shape[0] < verts.shape[0] // 2 and 0 < dt.shape[0] < tris.shape[0] // 2
        dn = e.mesh_normals(dv, dt)
        drgb, dused = e.mesh_colours(dv, dn, **CKW)
        assert _bytes(e.coloured_mesh(vol, decimate_cell=cell, decimate_placement=placement, **CKW)) == _bytes((dv, dt, dn, drgb, dused))

    # with pruning and smoothing as well: the six calls
    _, ntris, n = e.mesh_components(verts.shape[0], tris)
    k = max(2, int(ntris.max()) // 2)
    pv, pt, _ = e.prune_mesh(verts, tris, min_triangles=k)
    sv = e.smooth_mesh(pv, pt, 2)
    dv, dt, dmap = e.decimate_mesh(sv, pt, cell, origin)
    assert _bytes((dv, dt, dmap)) == _bytes(dr.decimate(sv, pt, cell, origin))
    assert 0 < dt.shape[0] < pt.shape[0]
    dn = e.mesh_normals(dv, dt)
    drgb, dused = e.mesh_colours(dv, dn, **CKW)
    assert _bytes(e.coloured_mesh(vol, min_triangles=k, smooth_iterations=2, decimate_cell=cell, **CKW)) == _bytes((dv, dt, dn, drgb, dused))

    # nothing of the engine's state moved
    assert e.patches().tobytes() == alive.tobytes() and e.thresholds() == thr
    t = engine_with_pool(sc, PLAIN, None, sizes, None, seeds)
    assert t.patches().tobytes() == alive.tobytes()
    assert e.propagate(1) == t.propagate(1)
    assert e.patches().tobytes() == t.patches().tobytes()
    t.close()
    e.close()
