"""Known answers for tests/mesh_attr_reading.py itself, so that the yardstick of the GPU tests is checked without a GPU."""
import numpy as np

import mesh_attr_reading as ar
import mesh_reading as mr
from maps_reading import cameras64, render_agree64
from mvskit_amd import synth
from scene_support import grid_mesh


def test_flat_grid_gives_the_axis_exactly():
    verts, tris = grid_mesh(9, 7)
    n = ar.normals_exact(verts, tris)
    assert n.dtype == np.float32 and n.shape == verts.shape
    assert (n == np.array([0, 0, 1], np.float32)).all()
    assert (ar.normals_exact(verts, tris[:, [0, 2, 1]]) == np.array([0, 0, -1], np.float32)).all()
    # the order of the triangles plays no part
    z = np.random.default_rng(0).normal(size=(7, 9))
    verts, tris = grid_mesh(9, 7, z)
    perm = np.random.default_rng(1).permutation(tris.shape[0])
    assert ar.normals_exact(verts, tris).tobytes() == ar.normals_exact(verts, tris[perm]).tobytes()


def test_sphere_normals_are_radial():
    dims, origin, voxel = (11, 10, 10), (1.0, 2.0, 3.0), 0.5
    centre = np.array([1.0 + 0.5 * 5.2, 2.0 + 0.5 * 4.4, 3.0 + 0.5 * 4.6])
    F = mr.sphere_volume(dims, [centre], 0.5 * 3.3, origin=origin, voxel=voxel)
    verts, tris = mr.extract(origin, voxel, dims, F)
    assert mr.closed_and_oriented(tris)
    n = ar.normals_exact(verts, tris).astype(np.float64)
    radial = verts.astype(np.float64) - centre
    radial /= np.linalg.norm(radial, axis=1, keepdims=True)
    assert ((n * radial).sum(1) > 0.9).all()
    assert (np.abs(np.linalg.norm(n, axis=1) - 1.0) < 1e-6).all()


def test_unreferenced_degenerate_and_non_finite():
    verts, tris = grid_mesh(4, 4)
    extra = np.concatenate([verts, [[9, 9, 9]]]).astype(np.float32)
    n = ar.normals_exact(extra, tris)
    assert (n[-1] == 0).all() and (n[:-1] == np.array([0, 0, 1], np.float32)).all()
    # all degenerate: M = 0
    assert (ar.normals_exact(verts, np.array([[0, 0, 1], [2, 2, 2]], np.int32)) == 0).all()
    assert ar.normals_exact(verts, np.zeros((0, 3), np.int32)).shape == (16, 3)
    assert ar.normals_exact(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)).shape == (0, 3)
    # a triangle with a NaN corner adds nothing, to its finite corners either
    bad = np.concatenate([verts, [[np.nan, 0, 0]]]).astype(np.float32)
    with_nan = np.concatenate([tris, [[0, 5, 16]]]).astype(np.int32)
    assert ar.normals_exact(bad, with_nan)[:-1].tobytes() == n[:-1].tobytes()
    # a face 2^40 times smaller than the largest vanishes: its own vertex keeps a zero normal
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 0], [5 + 2.0 ** -20, 5, 0], [5, 5, 2.0 ** -20]], np.float32)
    n = ar.normals_exact(v, np.array([[0, 1, 2], [3, 4, 5]], np.int32))
    assert (n[:3] == np.array([0, 0, 1], np.float32)).all() and (n[3:] == 0).all()


def _plane_setup(colour):
    """three views of the plane z = 0 behind one exact patch that every pixel renders, images of one colour"""
    sc = synth.make_scene(nviews=3, W=48, H=32, arc_deg=30.0, radius=4.0, kind="plane")
    sizes = [(sc.W, sc.H)] * 3
    cams = cameras64(sc, 0, sizes)
    pat = np.zeros(1, synth.PATCH_DTYPE)
    pat["coord"][0, :4] = (0, 0, 0, 1)
    pat["normal"][0, :3] = (0, 0, 1)
    ids = [np.zeros((sc.H, sc.W), np.int32) for _ in range(3)]
    bits, unsure = render_agree64(pat, ids, cams, 0.004, 0.98)
    images = [np.full((sc.H, sc.W, 3), colour, np.uint8) for _ in range(3)]
    return pat, ids, bits, unsure, cams, images


def test_colours_of_constant_images():
    colour = (10, 200, 30)
    pat, ids, bits, unsure, cams, images = _plane_setup(colour)
    rng = np.random.default_rng(3)
    verts = np.concatenate([rng.uniform(-0.05, 0.05, (50, 2)), np.zeros((50, 1))], axis=1)
    up = np.tile([0.0, 0.0, 1.0], (50, 1))
    for normals in (up, None, np.zeros((50, 3))):
        r = ar.colours64(pat, ids, bits, unsure, cams, images, None, verts, normals, occl_tol=0.004)
        assert r["reached"].all() and r["confirmed"].all() and (r["used"] == (3 | 0x80)).all()
        assert np.abs(r["mean"] - np.array(colour, np.float64)).max() < 1e-9
    # facing away: no view at all
    r = ar.colours64(pat, ids, bits, unsure, cams, images, None, verts, -up, occl_tol=0.004)
    assert (r["used"] == 0).all() and np.isnan(r["mean"]).all() and r["reached"].all()
    # view 1 masked everywhere: two views left
    masks = [None, np.zeros(ids[1].shape, bool), None]
    r = ar.colours64(pat, ids, bits, unsure, cams, images, masks, verts, up, occl_tol=0.004)
    assert (r["used"] == (2 | 0x80)).all()
    # no pixel usable (nobody agrees often enough): every view unconfirmed
    r = ar.colours64(pat, ids, bits, unsure, cams, images, None, verts, up, min_consistent=3, occl_tol=0.004)
    assert (r["used"] == 3).all() and not r["confirmed"].any() and np.abs(r["mean"] - np.array(colour, np.float64)).max() < 1e-9
    # far outside every image
    r = ar.colours64(pat, ids, bits, unsure, cams, images, None, verts + [50.0, 0, 0], up, occl_tol=0.004)
    assert (r["used"] == 0).all() and not r["reached"].any()


def test_a_vertex_off_the_plane_is_confirmed_by_no_view():
    pat, ids, bits, unsure, cams, images = _plane_setup((90, 90, 90))
    rng = np.random.default_rng(4)
    xy = rng.uniform(-0.05, 0.05, (40, 2))
    up = np.tile([0.0, 0.0, 1.0], (40, 1))
    for dz in (0.2, -0.2):  # 5 % of the depth of 4
        verts = np.concatenate([xy, np.full((40, 1), dz)], axis=1)
        r = ar.colours64(pat, ids, bits, unsure, cams, images, None, verts, up, occl_tol=0.004)
        assert r["reached"].all() and (r["used"] == 0).all() and not r["confirmed"].any()
    # weights: a brighter view 0 pulls the mean towards it by its share of the weights
    images[0][:] = 190
    verts = np.concatenate([xy, np.zeros((40, 1))], axis=1)
    r = ar.colours64(pat, ids, bits, unsure, cams, images, None, verts, up, occl_tol=0.004)
    d = np.stack([c["C"] - verts for c in cams])
    w = d[:, :, 2] / np.linalg.norm(d, axis=2)
    want = (w[0] * 190 + (w[1] + w[2]) * 90) / w.sum(0)
    assert np.abs(r["mean"] - want[:, None]).max() < 1e-9 and (r["used"] == (3 | 0x80)).all()
