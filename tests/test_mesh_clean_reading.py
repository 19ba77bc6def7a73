"""tests/mesh_clean_reading.py against independent statements of the same things (CPU): its components against a breadth-first search
(and scipy's connected_components where scipy imports), the invariants of prune, and what smoothing is for -- a jittered plane gets
flatter, and Taubin's second step keeps the volume of a closed surface better than plain Laplacian smoothing does."""
from collections import deque

import numpy as np
import pytest

import mesh_clean_reading as cr
import mesh_reading as mr
from scene_support import grid_mesh


def _bfs_labels(n_v, tris):
    adj = [[] for _ in range(n_v)]
    for a, b, c in np.asarray(tris).tolist():
        adj[a] += [b, c]
        adj[b] += [a, c]
        adj[c] += [a, b]
    label = [-1] * n_v
    for s in range(n_v):  # ascending: the first vertex met of a component is its smallest
        if label[s] >= 0:
            continue
        label[s] = s
        todo = deque([s])
        while todo:
            u = todo.popleft()
            for w in adj[u]:
                if label[w] < 0:
                    label[w] = s
                    todo.append(w)
    return np.array(label, np.int32)


def _cases():
    rng = np.random.default_rng(21)
    yield "empty", 5, np.zeros((0, 3), np.int32)
    yield "one", 3, np.array([[2, 0, 1]], np.int32)
    yield "random sparse", 400, rng.integers(0, 400, size=(150, 3)).astype(np.int32)  # repeated ids among them
    strip = np.stack([np.arange(600), np.arange(600) + 1, np.arange(600) + 2], 1).astype(np.int32)
    yield "shuffled strip", 602, strip[rng.permutation(600)]
    _, g = grid_mesh(9, 7)
    two = np.concatenate([g, g + 63])
    yield "two grids", 130, two
    yield "two grids sharing a vertex", 130, np.where(two == 63, 62, two).astype(np.int32)
    # the smallest id of a component only in its last triangle
    yield "late root", 12, np.array([[5, 6, 7], [7, 8, 9], [9, 10, 11], [11, 1, 5]], np.int32)


@pytest.mark.parametrize("name,n_v,tris", list(_cases()), ids=[c[0] for c in _cases()])
def test_components_against_breadth_first_search(name, n_v, tris):
    label, ntris, n_comp = cr.components(n_v, tris)
    want = _bfs_labels(n_v, tris)
    assert label.dtype == np.int32 and ntris.dtype == np.int32
    assert (label == want).all()
    count = np.bincount(want[tris[:, 0]], minlength=n_v) if tris.shape[0] else np.zeros(n_v, np.int64)
    assert (ntris == count[want]).all() and n_comp == int((count > 0).sum())
    assert int(ntris[label == np.arange(n_v)].sum()) == tris.shape[0]


@pytest.mark.parametrize("name,n_v,tris", list(_cases()), ids=[c[0] for c in _cases()])
def test_components_against_scipy(name, n_v, tris):
    sp = pytest.importorskip("scipy.sparse")
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    t = np.asarray(tris, np.int64)
    a = np.concatenate([t[:, 0], t[:, 0]])
    b = np.concatenate([t[:, 1], t[:, 2]])
    g = sp.coo_matrix((np.ones(a.shape[0]), (a, b)), shape=(n_v, n_v))
    n, lab = csgraph.connected_components(g, directed=False)
    label, _, _ = cr.components(n_v, tris)
    assert np.unique(label).shape[0] == n
    # the same partition: scipy's labels are arbitrary numbers, the reading's the smallest member
    first = np.full(n, n_v, np.int64)
    np.minimum.at(first, lab, np.arange(n_v))
    assert (first[lab] == label).all()


def _two_blobs_and_dust():
    """a 12 x 12 grid (242 triangles), a 4 x 4 grid (18), a single triangle, and unused vertices before, between and behind them"""
    rng = np.random.default_rng(22)
    v1, t1 = grid_mesh(12, 12, rng.normal(size=(12, 12)))
    v2, t2 = grid_mesh(4, 4)
    loose = rng.normal(size=(11, 3)).astype(np.float32)
    verts = np.concatenate([loose[:3], v1, loose[3:7], v2 + np.float32(50), loose[7:], [[0, 0, 9], [1, 0, 9], [0, 1, 9]]]).astype(np.float32)
    tris = np.concatenate([t1 + 3, t2 + 3 + 144 + 4, [[171, 172, 173]]]).astype(np.int32)
    return verts, tris[rng.permutation(tris.shape[0])]


@pytest.mark.parametrize("min_triangles,largest_only,n_t", [(1, False, 261), (2, False, 260), (19, False, 242), (1, True, 242), (243, False, 0), (243, True, 0)])
def test_prune_invariants(min_triangles, largest_only, n_t):
    verts, tris = _two_blobs_and_dust()
    pv, pt, vmap = cr.prune(verts, tris, min_triangles, largest_only)
    assert pv.dtype == np.float32 and pt.dtype == np.int32 and vmap.dtype == np.int32 and vmap.shape == (verts.shape[0],)
    assert pt.shape[0] == n_t
    kept = vmap >= 0
    # kept vertices in their input order with their bytes, new ids 0 .. n' - 1 ascending
    assert (vmap[kept] == np.arange(kept.sum())).all() and pv.tobytes() == verts[kept].tobytes()
    # no unused vertex left, and every kept vertex was used by a kept triangle
    assert np.unique(pt).shape[0] == pv.shape[0]
    # kept triangles in their input order, corner order unchanged: mapping back gives a subsequence of the input
    back = np.flatnonzero(kept)[pt]
    _, ntris, _ = cr.components(verts.shape[0], tris)
    want = ntris[tris[:, 0]] >= min_triangles
    if largest_only:
        want &= ntris[tris[:, 0]] == 242
    assert back.tobytes() == tris[want].astype(np.int64).tobytes()
    if min_triangles == 1 and not largest_only:
        assert (~kept).sum() == 11


def test_prune_tie_keeps_the_smaller_label():
    _, g = grid_mesh(5, 5)
    verts = np.random.default_rng(23).normal(size=(52, 3)).astype(np.float32)
    tris = np.concatenate([g + 27, g + 1]).astype(np.int32)
    pv, pt, vmap = cr.prune(verts, tris, 1, True)
    assert pt.tobytes() == g.astype(np.int32).tobytes() and (np.flatnonzero(vmap >= 0) == np.arange(1, 26)).all()


def jittered_grid(n=70, seed=3, amp=0.3):
    return grid_mesh(n, n, amp * np.random.default_rng(seed).normal(size=(n, n)))


def interior_rms_height(verts, n=70):
    z = verts[:, 2].astype(np.float64).reshape(n, n)[1:-1, 1:-1]
    return float(np.sqrt((z * z).mean()))


def sphere_mesh():
    dims, origin, voxel = (11, 10, 10), (1.0, 2.0, 3.0), 0.5
    centre = np.array([1.0 + 0.5 * 5.2, 2.0 + 0.5 * 4.4, 3.0 + 0.5 * 4.6])
    F = mr.sphere_volume(dims, [centre], 0.5 * 3.3, origin=origin, voxel=voxel)
    return mr.extract(origin, voxel, dims, F)


def enclosed_volume(verts, tris):
    v = verts.astype(np.float64)
    a, b, c = v[tris[:, 0]], v[tris[:, 1]], v[tris[:, 2]]
    return float(abs((a * np.cross(b, c)).sum()) / 6.0)


def test_smoothing_flattens_a_jittered_plane():
    """seen: interior rms height 0.3008 before, 0.1151 after 10 default iterations"""
    verts, tris = jittered_grid()
    out = cr.smooth_exact(verts, tris)
    assert out.dtype == np.float32 and out.shape == verts.shape
    before, after = interior_rms_height(verts), interior_rms_height(out)
    print(f"interior rms height {before:.6f} -> {after:.6f}")
    assert after < before


def test_taubin_keeps_the_volume_better_than_laplacian():
    """seen: volume 17.953 of the extracted sphere, 18.103 after 10 Taubin iterations, 14.372 after 10 Laplacian ones"""
    verts, tris = sphere_mesh()
    assert mr.closed_and_oriented(tris)
    v0 = enclosed_volume(verts, tris)
    taubin = enclosed_volume(cr.smooth_exact(verts, tris), tris)
    laplace = enclosed_volume(cr.smooth_exact(verts, tris, mu=0.0), tris)
    print(f"volume {v0:.6f}: Taubin {taubin:.6f}, Laplacian {laplace:.6f}")
    assert abs(taubin - v0) < abs(laplace - v0)


def test_smoothing_details():
    verts, tris = jittered_grid(12, seed=4)
    assert cr.smooth_exact(verts, tris, iterations=0).tobytes() == verts.tobytes()
    # triangle order plays no part
    perm = np.random.default_rng(5).permutation(tris.shape[0])
    assert cr.smooth_exact(verts, tris[perm], 3).tobytes() == cr.smooth_exact(verts, tris, 3).tobytes()
    # an unused vertex, and all-coincident vertices, keep their bytes (-0.0 and a NaN included)
    more = np.concatenate([verts, [[np.nan, -0.0, 5.0]]]).astype(np.float32)
    assert cr.smooth_exact(more, tris, 2)[-1].tobytes() == more[-1].tobytes()
    same = np.tile(np.float32([-0.0, 2.5, -1.0]), (144, 1))
    assert cr.smooth_exact(same, tris, 2).tobytes() == same.tobytes()
    # one triangle, one plain step: every vertex moves half way to the mean of the other two
    tri = np.array([[0, 0, 0], [4, 0, 0], [0, 8, 0]], np.float32)
    out = cr.smooth_exact(tri, np.array([[0, 1, 2]]), 1, 0.5, 0.0)
    assert (out == np.array([[1, 2, 0], [2, 2, 0], [1, 4, 0]], np.float32)).all()
