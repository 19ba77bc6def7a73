"""The textured mesh in the chain, on the pool and lattice of tests/test_gpu_mesh_fill_chain.py (3 views of 96 x 64 on the textured plane,
csize 2): Engine.textured_mesh is the calls made by hand, Engine.coloured_mesh returns the bytes it returned before, the atlas shows what
the labelled view shows at each triangle's centroid, and nothing of the engine's state moves."""
import numpy as np
import pytest

import mesh_render_reading as rr
import mesh_texture_reading as tr
from maps_reading import DEPTH_TOL, NORMAL_COS
from mvskit_amd import engine, synth
from scene_support import PLAIN, cached_scene, engine_with_pool, lattice

pytestmark = pytest.mark.gpu
KW = dict(min_consistent=1, depth_tol=DEPTH_TOL, normal_cos=NORMAL_COS)
RES, WIDTH = 8, 512


def _bytes(arrays):
    return [np.asarray(a).tobytes() for a in arrays]


def _bilinear64(img, x, y):
    """a float64 bilinear sample of img [H, W, 3] at (x, y) inside the bilinear window; written apart from the reading's"""
    x0, y0 = np.floor(x).astype(int), np.floor(y).astype(int)
    u, v = (x - x0)[:, None], (y - y0)[:, None]
    p = img.astype(np.float64)
    return (p[y0, x0] * (1 - u) + p[y0, x0 + 1] * u) * (1 - v) + (p[y0 + 1, x0] * (1 - u) + p[y0 + 1, x0 + 1] * u) * v


def test_textured_mesh_in_the_chain(tmp_path):
    sc = cached_scene(3, 96, 64, 30.0)
    sizes = [(sc.W, sc.H)] * sc.nviews
    seeds = synth.make_seeds(sc, PLAIN["level"], PLAIN["csize"], stride=1)
    e = engine_with_pool(sc, PLAIN, None, sizes, None, seeds)
    alive, thr = e.patches(), e.thresholds()
    vol = lattice(sc, PLAIN["level"])
    chain = dict(largest_only=True, fill_max_edges=16, smooth_iterations=2, decimate_cell=2.0 * float(vol.voxel), **KW)
    before = e.coloured_mesh(vol, **chain)

    # the chain is the calls made by hand
    verts, tris, normals, atlas, uv, label = e.textured_mesh(vol, res=RES, atlas_width=WIDTH, **chain)
    assert _bytes((verts, tris, normals)) == _bytes(before[:3])
    visible = e.mesh_visibility(verts, tris, 0.01)
    hand_label, area, faces = e.mesh_face_views(verts, tris, visible=visible, front_only=True)
    hand_atlas, hand_uv, n_textured = e.texture_mesh(verts, tris, hand_label, res=RES, width=WIDTH)
    assert _bytes((label, atlas, uv)) == _bytes((hand_label, hand_atlas, hand_uv))
    print(f"chain: {verts.shape[0]} vertices, {tris.shape[0]} triangles, faces {faces.tolist()}, {n_textured} textured, atlas {atlas.shape}")
    assert n_textured == int((label >= 0).sum()) > 0.5 * tris.shape[0] and faces.sum() == n_textured
    # the other arguments reach their calls
    loose = e.textured_mesh(vol, res=2, atlas_width=64, front_only=False, visibility_tol=0.0, **chain)
    l2 = e.mesh_face_views(verts, tris, visible=e.mesh_visibility(verts, tris, 0.0), front_only=False)[0]
    assert _bytes(loose[3:]) == _bytes(e.texture_mesh(verts, tris, l2, res=2, width=64)[:2] + (l2,))
    # and the writer takes the result
    engine.write_mesh_obj(str(tmp_path / "chain.obj"), verts, tris, atlas, uv, normals=normals)
    assert (tmp_path / "chain.png").stat().st_size > 1000 and (tmp_path / "chain.mtl").exists()

    # coloured_mesh returns the bytes it returned before
    assert _bytes(e.coloured_mesh(vol, **chain)) == _bytes(before)

    # photometric sanity, apart from the reading's sampling code: the texel nearest each textured triangle's centroid (weights 2, 3, 3 of
    # 8) against a float64 bilinear sample of the labelled view at the float64 projection of the 3-D centroid.  The two differ by what
    # the image does between the centroid and the texel's own point -- which the reading, on the device's snapped vertices, measures --
    # plus, for the device, no more than the rounding to a byte and the snapping of a position: sqrt(2) / 512 pixel times the steepest
    # step between neighbouring texels of the views (test_mesh_texture_reading's ramp bound with that slope)
    screen, vdepth = e.mesh_screen(verts, tris)
    images = [e.pyramid(v, 0) for v in range(sc.nviews)]
    reading = tr.texture(list(screen), list(vdepth), tris, label, images, RES, WIDTH)
    rows = np.flatnonzero(label >= 0)
    assert reading["flags"].tolist() == (label >= 0).tolist()
    k = np.arange(rows.shape[0])
    at = np.where((k % 2 == 1)[:, None], uv[rows, 0] - 3, uv[rows, 0] + 3)  # (i, j) = (3, 3) from vertex 0's corner, towards the inside
    centroid = verts.astype(np.float64)[tris[rows]].mean(axis=1)
    want = np.zeros((rows.shape[0], 3))
    for v in range(sc.nviews):
        mine = label[rows] == v
        xy = rr.project64(rr.camera64(sc.P[v], 0), centroid[mine])[2]
        want[mine] = _bilinear64(images[v], xy[:, 0], xy[:, 1])
    seen = np.abs(reading["atlas"][at[:, 1], at[:, 0]].astype(np.float64) - want).max()
    got = np.abs(atlas[at[:, 1], at[:, 0]].astype(np.float64) - want).max()
    slope = max(float(np.abs(np.diff(im.astype(np.float64), axis=a)).max()) for im in images for a in (0, 1))
    term = 0.5 + slope * np.sqrt(2.0) / 512
    print(f"centroid texels: the device is off by at most {got:.3f}, the reading by {seen:.3f}; steepest step {slope:.0f}, snapping term {term:.3f}")
    assert got <= seen + term
    # and what the reading sees is the image between two points a twelfth of a median apart, not another place: the texel's point and
    # the centroid differ by the barycentric step (1/12, -1/24, -1/24), on the screen (p0 - (p1 + p2) / 2) / 12 up to the perspective
    # across a triangle of a few pixels at depth 4 (5 % is generous), no longer than the longer edge at vertex 0 over 12; a bilinear
    # surface changes by at most the steepest step times |dx| + |dy| <= sqrt(2) |d|
    s = np.stack([screen[v][tris[rows]] for v in range(sc.nviews)])[label[rows], k].astype(np.float64) / 256.0
    reach = np.maximum(np.linalg.norm(s[:, 1] - s[:, 0], axis=1), np.linalg.norm(s[:, 2] - s[:, 0], axis=1)) / 12.0
    each = np.abs(reading["atlas"][at[:, 1], at[:, 0]].astype(np.float64) - want).max(axis=1)
    assert (each <= term + slope * np.sqrt(2.0) * 1.05 * reach).all()

    # nothing of the engine's state moved
    assert e.patches().tobytes() == alive.tobytes() and e.thresholds() == thr
    t = engine_with_pool(sc, PLAIN, None, sizes, None, seeds)
    assert t.patches().tobytes() == alive.tobytes()
    assert e.propagate(1) == t.propagate(1)
    assert e.patches().tobytes() == t.patches().tobytes()
    t.close()
    e.close()
