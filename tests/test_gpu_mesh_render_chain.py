"""The mesh render in the chain, on the pool and lattice of tests/test_gpu_mesh_fill_chain.py (3 views of 96 x 64 on the textured plane, csize
2): the engine's own mesh rendered back into the views lies within the truncation band of the dense maps it was fused from, the colouring
call with a visibility is the colouring call where every bit is set, grey where none is, never blends more views than without it, and
Engine.coloured_mesh(mesh_occlusion=True) is the calls made by hand while the default returns today's bytes; nothing of the engine's state
moves."""
import numpy as np
import pytest

from maps_reading import DEPTH_TOL, NORMAL_COS
from mvskit_amd import engine, synth
from scene_support import PLAIN, TRUNC_VOXELS, cached_scene, engine_with_pool, lattice

pytestmark = pytest.mark.gpu
KW = dict(min_consistent=1, depth_tol=DEPTH_TOL, normal_cos=NORMAL_COS)
CKW = dict(occl_tol=DEPTH_TOL, min_cos=0.1, **KW)


def _bytes(arrays):
    return [a.tobytes() for a in arrays]


def test_render_and_occlusion_in_the_chain():
    sc = cached_scene(3, 96, 64, 30.0)
    sizes = [(sc.W, sc.H)] * sc.nviews
    seeds = synth.make_seeds(sc, PLAIN["level"], PLAIN["csize"], stride=1)
    e = engine_with_pool(sc, PLAIN, None, sizes, None, seeds)
    alive, thr = e.patches(), e.thresholds()
    vol = lattice(sc, PLAIN["level"])

    # the mesh of the maps, seen from the views of the maps
    verts, tris = e.mesh(vol, **KW)
    assert verts.shape[0] > 256 and tris.shape[0] > 256
    maps, covered, skipped = e.render_mesh(verts, tris)
    dense = e.render_maps(depth_tol=DEPTH_TOL, normal_cos=NORMAL_COS)
    band = TRUNC_VOXELS * float(vol.voxel)
    for v in range(sc.nviews):
        both = np.isfinite(maps[v][0]) & np.isfinite(dense[v]["depth"])
        off = np.abs(maps[v][0][both].astype(np.float64) - dense[v]["depth"][both])
        print(f"view {v}: {int(covered[v])} covered, {int(skipped[v])} skipped, {int(both.sum())} pixels with both depths, off by at most {off.max():.4f} (band {band:.4f})")
        assert both.sum() > 100 and (off < band).all()  # the lattice spans some 36 x 30 pixels
        assert skipped[v] == 0 and covered[v] == int(np.isfinite(maps[v][0]).sum())
    only = e.render_mesh(verts, tris, views=[1])[0]
    assert only[0] is None and only[2] is None and _bytes(only[1]) == _bytes(maps[1])

    # the colouring call and the visibility
    normals = e.mesh_normals(verts, tris)
    rgb, used = e.mesh_colours(verts, normals, **CKW)
    ones = np.full(verts.shape[0], np.uint64(0xFFFFFFFFFFFFFFFF))
    assert _bytes(e.mesh_colours(verts, normals, visible=ones, **CKW)) == _bytes((rgb, used))
    grey, none = e.mesh_colours(verts, normals, visible=np.zeros(verts.shape[0], np.uint64), **CKW)
    assert (grey == 128).all() and (none == 0).all()
    visible = e.mesh_visibility(verts, tris)
    assert visible.dtype == np.uint64 and not (visible >> np.uint64(sc.nviews)).any()
    vrgb, vused = e.mesh_colours(verts, normals, visible=visible, **CKW)
    print("views blended without / with the mesh's visibility:", np.bincount(used & 0x7F).tolist(), "/", np.bincount(vused & 0x7F).tolist(),
          "; vertices whose colour changed:", int((vrgb != rgb).any(axis=1).sum()), "of", verts.shape[0])
    assert ((vused & 0x7F) <= (used & 0x7F)).all()
    with pytest.raises(ValueError):
        e.mesh_colours(verts, normals, visible=visible[:-1], **CKW)

    # the chain: the visibility is the final mesh's, behind the decimation
    chain = dict(largest_only=True, smooth_iterations=2, decimate_cell=2.0 * float(vol.voxel), **CKW)
    today = e.coloured_mesh(vol, **chain)
    assert _bytes(e.coloured_mesh(vol, mesh_occlusion=False, **chain)) == _bytes(today)
    dv, dt, dn = today[:3]
    hand = e.mesh_colours(dv, dn, visible=e.mesh_visibility(dv, dt), **CKW)
    got = e.coloured_mesh(vol, mesh_occlusion=True, **chain)
    assert _bytes(got[:3]) == _bytes(today[:3]) and _bytes(got[3:]) == _bytes(hand)
    tight = e.coloured_mesh(vol, mesh_occlusion=True, visibility_tol=0.0, **chain)
    assert _bytes(tight[3:]) == _bytes(e.mesh_colours(dv, dn, visible=e.mesh_visibility(dv, dt, tol=0.0), **CKW))

    # nothing of the engine's state moved
    assert e.patches().tobytes() == alive.tobytes() and e.thresholds() == thr
    t = engine_with_pool(sc, PLAIN, None, sizes, None, seeds)
    assert t.patches().tobytes() == alive.tobytes()
    assert e.propagate(1) == t.propagate(1)
    assert e.patches().tobytes() == t.patches().tobytes()
    t.close()
    e.close()
