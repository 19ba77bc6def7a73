"""Engine.coloured_mesh with hole filling switched on, on the smallest plane scene of tests/test_gpu_mesh_tsdf.py (3 views of 96 x 64 on the
textured plane, csize 2): the chain mesh -> prune -> fill -> smooth -> normals -> colours equals the calls made by hand with fill_holes
equal to the reading, fill_max_edges = 0 gives the bytes of today's chain, and nothing of the engine's state moves.  max_edges comes from
the mesh's own boundaries: the longest loop that is shorter than the rim, so that a loop is filled and the rim is not.  A mesh without
such a loop has the triangles around one interior vertex taken out by hand before fill_holes is compared with the reading."""
import numpy as np
import pytest

import mesh_fill_reading as fr
from maps_reading import DEPTH_TOL, NORMAL_COS
from mvskit_amd import synth
from scene_support import PLAIN, cached_scene, engine_with_pool, lattice

pytestmark = pytest.mark.gpu
KW = dict(min_consistent=1, depth_tol=DEPTH_TOL, normal_cos=NORMAL_COS)
CKW = dict(occl_tol=DEPTH_TOL, min_cos=0.1, **KW)


def _bytes(arrays):
    return [a.tobytes() for a in arrays]


def _loop_lengths(loop, length):
    return np.sort(length[(loop == np.arange(loop.shape[0])) & (length > 0)])


def test_coloured_mesh_with_hole_filling():
    sc = cached_scene(3, 96, 64, 30.0)
    sizes = [(sc.W, sc.H)] * sc.nviews
    seeds = synth.make_seeds(sc, PLAIN["level"], PLAIN["csize"], stride=1)
    e = engine_with_pool(sc, PLAIN, None, sizes, None, seeds)
    alive, thr = e.patches(), e.thresholds()
    vol = lattice(sc, PLAIN["level"])

    # today's chain, and the default
    verts, tris = e.mesh(vol, **KW)
    pv, pt, _ = e.prune_mesh(verts, tris, 1, True)
    sv = e.smooth_mesh(pv, pt, 2)
    sn = e.mesh_normals(sv, pt)
    srgb, sused = e.mesh_colours(sv, sn, **CKW)
    today = _bytes((sv, pt, sn, srgb, sused))
    assert pv.shape[0] > 256 and pt.shape[0] > 256
    assert _bytes(e.coloured_mesh(vol, largest_only=True, smooth_iterations=2, **CKW)) == today
    assert _bytes(e.coloured_mesh(vol, largest_only=True, smooth_iterations=2, fill_max_edges=0, **CKW)) == today

    # max_edges from the mesh's own boundaries
    n_v = pv.shape[0]
    found = e.mesh_boundaries(n_v, pt)
    want = fr.boundaries(n_v, pt)
    assert _bytes(found[:2]) == _bytes(want[:2]) and found[2:] == want[2:]
    loops = _loop_lengths(found[0], found[1])
    print("boundaries of the pruned mesh: loops", loops.tolist(), "complex", found[3], "irregular", found[4])
    assert loops.shape[0] >= 1  # the rim of the plane, at least
    rim = int(loops[-1])
    shorter = loops[loops < rim]
    k = int(shorter[-1]) if shorter.shape[0] else min(64, rim - 1)
    assert 3 <= k < rim

    # fill_holes against the reading
    fv, ft, nf = e.fill_holes(pv, pt, k)
    assert _bytes((fv, ft)) == _bytes(fr.fill(pv, pt, k)[:2]) and nf == fr.fill(pv, pt, k)[2] == shorter.shape[0]
    if shorter.shape[0] == 0:  # no loop but the rim: pierce the mesh by hand
        on = found[0] >= 0
        touches = np.zeros(n_v, bool)
        touches[pt[on[pt].any(axis=1)].reshape(-1)] = True  # on the rim or next to it
        valence = np.bincount(pt.reshape(-1), minlength=n_v)
        inner = int(np.flatnonzero(~touches & (valence >= 4))[0])
        holed = pt[~(pt == inner).any(axis=1)]
        hv, ht, hf = e.fill_holes(pv, holed, k)
        assert _bytes((hv, ht)) == _bytes(fr.fill(pv, holed, k)[:2]) and hf == 1 and hv.shape[0] == n_v + 1
        after = e.mesh_boundaries(hv.shape[0], ht)
        assert _loop_lengths(after[0], after[1]).tolist() == loops.tolist() and after[2:] == found[2:]
    else:
        after = e.mesh_boundaries(fv.shape[0], ft)
        assert _loop_lengths(after[0], after[1]).tolist() == [rim] * int((loops == rim).sum()) and after[3:] == found[3:]

    # the chain with filling equals the calls made by hand
    fs = e.smooth_mesh(fv, ft, 2)
    fn = e.mesh_normals(fs, ft)
    frgb, fused = e.mesh_colours(fs, fn, **CKW)
    assert _bytes(e.coloured_mesh(vol, largest_only=True, fill_max_edges=k, smooth_iterations=2, **CKW)) == _bytes((fs, ft, fn, frgb, fused))

    # nothing of the engine's state moved
    assert e.patches().tobytes() == alive.tobytes() and e.thresholds() == thr
    t = engine_with_pool(sc, PLAIN, None, sizes, None, seeds)
    assert t.patches().tobytes() == alive.tobytes()
    assert e.propagate(1) == t.propagate(1)
    assert e.patches().tobytes() == t.patches().tobytes()
    t.close()
    e.close()
