"""The numpy reading of the mesh render (tests/mesh_render_reading.py) on its own, without a GPU, on the cameras of the smallest plane
scene (3 views of 96 x 64 around the plane z = 0): the top-left rule is watertight, the depth is the plane's, the result does not depend
on the triangle order, and coincident triangles go to the smaller row.  These tests check the yardstick, not the engine: they run no
engine code (tests/test_mesh_render_abi.py and tests/test_gpu_mesh_render.py hold the engine to this reading)."""
import numpy as np
import pytest

import mesh_render_reading as rr
from scene_support import cached_scene, grid_mesh

CELL = 0.02  # world units a grid cell: about 0.57 pixel footprints (4 / 114.9) -- most triangles cover no centre, some cover one


@pytest.fixture(scope="module")
def case():
    sc = cached_scene(3, 96, 64, 20.0)
    verts, tris = grid_mesh(40, 30)
    verts = ((verts - np.float32([19.5, 14.5, 0.0])) * np.float32(CELL)).astype(np.float32)
    cams = [rr.camera64(sc.P[v], 0) for v in range(sc.nviews)]
    proj = [rr.project64(P, verts) for P in cams]
    maps = [rr.render(s, d, tris, sc.W, sc.H) for s, d, _, _ in proj]
    return sc, verts, tris, cams, proj, maps


def test_every_covered_pixel_is_covered_once(case):
    sc, verts, tris, cams, proj, maps = case
    for v, m in enumerate(maps):
        print(f"view {v}: {m['covered']} covered pixels, at most {int(m['count'].max())} triangles a pixel, {m['skipped']} skipped")
        assert m["skipped"] == 0
        assert m["covered"] > 300  # 39 x 29 cells of 0.57^2 pixels: about 370
        assert int(m["count"].max()) == 1, "a pixel centre inside the grid is covered twice: the top-left rule leaks"
        assert m["covered"] == int(m["count"].sum()) == int((m["tri"] >= 0).sum()) == int(np.isfinite(m["depth"]).sum())
        # and no hole: every centre that the unsnapped outline holds with a pixel to spare is covered (the grid is convex in the image)
        xy = proj[v][2][[0, 39, 30 * 40 - 1, 29 * 40]]
        yy, xx = np.mgrid[0:sc.H, 0:sc.W]
        inner = np.ones((sc.H, sc.W), bool)
        a1, a2 = xy[1] - xy[0], xy[2] - xy[0]
        sign = np.sign(a1[0] * a2[1] - a1[1] * a2[0])
        for a in range(4):
            e, q = xy[(a + 1) % 4] - xy[a], np.stack([xx - xy[a][0], yy - xy[a][1]], axis=-1)
            inner &= sign * (e[0] * q[..., 1] - e[1] * q[..., 0]) / np.hypot(*e) >= 1.0
        assert inner.sum() > 200 and (m["count"][inner] == 1).all()


def test_depth_is_the_planes(case):
    sc, verts, tris, cams, proj, maps = case
    delta = np.sqrt(2.0) / 512.0  # a vertex snaps by at most 1/512 pixel in x and in y
    worst = 0.0
    for v, m in enumerate(maps):
        P = cams[v]
        X = sc.points[v].astype(np.float64)
        true = X @ P[2, :3] + P[2, 3]  # the analytic depth of the plane at every pixel centre
        gy, gx = np.gradient(true)
        grad = float(np.sqrt(gx ** 2 + gy ** 2).max())  # depth per pixel
        # 1 / depth is affine over the image for a plane, and the rendered 1 / depth is the affine function that takes the true values
        # at the SNAPPED vertices: it differs from the true one by a convex combination of grad(1 / d) . (snap_i), at most
        # |grad(1 / d)| delta, which in depth is |grad d| delta, with the largest gradient of the whole image.  Then one float32 rounding
        # of the result.
        bound = grad * delta + rr.U * true
        have = m["tri"] >= 0
        err = np.abs(m["depth"].astype(np.float64) - true)[have]
        rel = float((err / true[have]).max())
        worst = max(worst, rel)
        print(f"view {v}: depth off the plane by at most {err.max():.3e} ({rel:.3e} relative), bound {float(np.max(bound)):.3e}")
        assert (err <= bound[have]).all()
    print(f"worst relative depth error {worst:.3e}")


def test_triangle_order_does_not_matter(case):
    sc, verts, tris, cams, proj, maps = case
    perm = np.random.RandomState(5).permutation(tris.shape[0])
    for v, m in enumerate(maps):
        s = rr.render(proj[v][0], proj[v][1], tris[perm], sc.W, sc.H)
        assert s["depth"].tobytes() == m["depth"].tobytes()
        have = m["tri"] >= 0
        assert ((s["tri"] >= 0) == have).all() and (perm[s["tri"][have]] == m["tri"][have]).all()


def test_coincident_copies_go_to_the_smaller_row(case):
    sc, verts, tris, cams, proj, maps = case
    n_t = tris.shape[0]
    perm = np.random.RandomState(6).permutation(n_t)
    twice = np.concatenate([tris[perm], tris])  # the second copy in another order: row n_t + t is triangle t again
    back = np.concatenate([perm, np.arange(n_t)])
    for v, m in enumerate(maps):
        s = rr.render(proj[v][0], proj[v][1], twice, sc.W, sc.H)
        assert s["depth"].tobytes() == m["depth"].tobytes()
        have = m["tri"] >= 0
        assert int(s["count"].max()) == 2 and (s["count"][have] == 2).all()
        assert (s["tri"][have] < n_t).all() and (back[s["tri"][have]] == m["tri"][have]).all()


def test_unusable_vertices_skip_their_triangles():
    sc = cached_scene(3, 96, 64, 20.0)
    P = rr.camera64(sc.P[0], 0)
    z = P[2, :3]
    side = np.cross(z, [0.0, 1.0, 0.0])
    wide = sc.centers[0] + 1e-3 * z + 10.0 * side / np.linalg.norm(side)  # a millimetre in front of the camera plane, ten units aside: 10^6 pixels
    verts = np.float32([[-0.5, -0.5, 0], [0.5, -0.5, 0], [0, 0.5, 0], [0, 0, 50.0], [np.nan, 0, 0], [np.inf, 0, 0], wide, [0.2, 0.2, 0.1]])
    tris = np.int32([[0, 1, 2], [0, 1, 3], [0, 1, 4], [0, 1, 5], [0, 1, 6], [0, 0, 1], [0, 1, 7]])
    s, d, _, _ = rr.project64(P, verts)
    ok = rr.usable(s, d)
    assert ok.tolist() == [True, True, True, False, False, False, False, True]
    m = rr.render(s, d, tris, sc.W, sc.H)
    assert m["skipped"] == 4  # behind the camera, NaN, infinite, beyond 2^24; the repeated id is no skip
    assert set(np.unique(m["tri"]).tolist()) <= {-1, 0, 6} and m["covered"] > 100
    alone = rr.render(s, d, tris[[0, 6]], sc.W, sc.H)
    assert alone["depth"].tobytes() == m["depth"].tobytes()
