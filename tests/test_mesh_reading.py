"""The yardstick of the mesh tests checked on its own, on the CPU: tests/mesh_reading.py's marching tetrahedra give closed, consistently
oriented, outward-facing surfaces of the right topology, and cover every sign pattern of one cube."""
import numpy as np

import mesh_reading as mr


def _normals_face_outward(verts, tris, grad):
    """every triangle's normal (v1 - v0) x (v2 - v0) has a positive component along grad(centroid): from inside (negative) to outside"""
    v = verts.astype(np.float64)
    a, b, c = v[tris[:, 0]], v[tris[:, 1]], v[tris[:, 2]]
    n = np.cross(b - a, c - a)
    keep = np.linalg.norm(n, axis=1) > 1e-12  # a crossing at a lattice point (t = 0) can give a triangle without area
    g = grad((a + b + c) / 3)
    return bool(((n * g).sum(1)[keep] > 0).all()) and keep.mean() > 0.9


def test_sphere():
    """a sphere in a 14^3 lattice (centre (6.4, 6.4, 6.0), radius 4.15): 970 vertices and 1936 triangles, closed, every directed edge
    paired with its reverse, Euler characteristic 2, normals outward, every vertex close to the sphere"""
    c, r = (6.4, 6.4, 6.0), 4.15
    F = mr.sphere_volume((14, 14, 14), [c], r)
    verts, tris = mr.extract((0, 0, 0), 1.0, (14, 14, 14), F)
    assert verts.dtype == np.float32 and tris.dtype == np.int32
    assert (verts.shape[0], tris.shape[0]) == (970, 1936)
    assert mr.closed_and_oriented(tris) and mr.euler(verts, tris) == 2
    assert np.unique(tris).shape[0] == verts.shape[0] and verts.shape[0] == 2 + tris.shape[0] // 2
    assert _normals_face_outward(verts, tris, lambda x: x - np.array(c))
    assert np.abs(np.linalg.norm(verts - np.array(c), axis=1) - r).max() < 0.15  # the distance is linear along an edge to second order


def test_two_spheres():
    """two spheres of radius 3.2 in 20 x 10 x 10: two closed components, Euler characteristic 4; 1122 vertices and 2236 triangles"""
    F = mr.sphere_volume((20, 10, 10), [(5.1, 4.6, 4.4), (14.2, 4.5, 4.7)], 3.2)
    verts, tris = mr.extract((0, 0, 0), 1.0, (20, 10, 10), F)
    assert (verts.shape[0], tris.shape[0]) == (1122, 2236)
    assert mr.closed_and_oriented(tris) and mr.euler(verts, tris) == 4


def test_random_volume_with_a_positive_border():
    rng = np.random.default_rng(11)
    F = rng.normal(size=(7, 8, 9)).astype(np.float32)
    F[0], F[-1], F[:, 0], F[:, -1], F[:, :, 0], F[:, :, -1] = 1, 1, 1, 1, 1, 1
    verts, tris = mr.extract((-1.0, 2.0, 0.5), 0.25, (9, 8, 7), F)
    assert tris.shape[0] > 500 and mr.closed_and_oriented(tris)
    assert np.unique(tris).shape[0] == verts.shape[0]  # nothing is unobserved: no rim vertex


def test_the_256_patterns_of_one_cube():
    """0 to 12 triangles per pattern, 1920 in all; a vertex per edge of the cube's 19 whose endpoints differ; no triangle without
    area (the crossings sit at the edge midpoints); the orientation is test_orientation_table_is_geometric's"""
    total, most = 0, 0
    for m in range(256):
        F = np.array([-1.0 if (m >> c) & 1 else 1.0 for c in range(8)], np.float32).reshape(2, 2, 2)
        verts, tris = mr.extract((0, 0, 0), 1.0, (2, 2, 2), F)
        total += tris.shape[0]
        most = max(most, tris.shape[0])
        edges = {(min(t[x], t[y]), max(t[x], t[y])) for t in mr.TETS for x in range(4) for y in range(x + 1, 4)}
        assert len(edges) == 19
        assert verts.shape[0] == sum(1 for a, b in edges if ((m >> a) ^ (m >> b)) & 1)
        assert (tris.shape[0] == 0) == (m in (0, 255))
        if tris.shape[0]:
            assert tris.min() >= 0 and tris.max() < verts.shape[0]
            v = verts.astype(np.float64)
            n = np.cross(v[tris[:, 1]] - v[tris[:, 0]], v[tris[:, 2]] - v[tris[:, 0]])
            assert (np.linalg.norm(n, axis=1) > 0).all()
    assert total == 1920 and most == 12


def test_orientation_table_is_geometric():
    """tet_triangles on real crossings, not midpoints: for random values with the given signs the oriented triangle's normal points along
    the gradient of the linear interpolant of the tetrahedron"""
    rng = np.random.default_rng(3)
    for t, tet in enumerate(mr.TETS):
        pos = np.array([[c & 1, (c >> 1) & 1, (c >> 2) & 1] for c in tet], np.float64)
        for m in range(1, 15):
            for _ in range(4):
                val = rng.uniform(0.05, 1.0, 4) * np.where([(m >> k) & 1 for k in range(4)], -1.0, 1.0)
                A = np.concatenate([pos, np.ones((4, 1))], axis=1)
                grad = np.linalg.solve(A, val)[:3]
                where = {c: k for k, c in enumerate(tet)}
                for tri in mr._CASES[(t, m)]:
                    pts = []
                    for lo, hi in tri:
                        a, b = where[lo], where[hi]
                        s = val[a] / (val[a] - val[b])
                        pts.append(pos[a] + s * (pos[b] - pos[a]))
                    n = np.cross(pts[1] - pts[0], pts[2] - pts[0])
                    assert np.dot(n, grad) > 0, (t, m)


def test_unobserved_points_cut_the_surface():
    """NaN values and counts below min_count: no vertex on an edge that touches one, no triangle from a cube that has one; count = None
    counts every non-NaN point"""
    F = mr.sphere_volume((8, 8, 8), [(3.5, 3.4, 3.6)], 2.2)
    count = np.full((8, 8, 8), 2, np.int32)
    count[:, :, 4:] = 1
    va, ta = mr.extract((0, 0, 0), 1.0, (8, 8, 8), F, count, min_count=2)
    G = F.copy()
    G[:, :, 4:] = np.nan
    vb, tb = mr.extract((0, 0, 0), 1.0, (8, 8, 8), G)
    vc, tc = mr.extract((0, 0, 0), 1.0, (8, 8, 8), F, None, min_count=2)
    assert va.tobytes() == vb.tobytes() and ta.tobytes() == tb.tobytes()
    assert 0 < ta.shape[0] < tc.shape[0] and (va[:, 0] <= 3.0).all() and not mr.closed_and_oriented(ta) and mr.closed_and_oriented(tc)
