"""tests/mesh_decimate_reading.py on the sphere of the prune test (CPU): what vertex clustering does to a closed surface.  Cells of 2 and
3 voxels leave a closed, oriented sphere with fewer vertices; a cell of 1.5 makes the surface pass the same three cells twice, the
duplicate rule drops one of the two triangles and the result is no longer closed; a cell of 0.01 only welds the vertices that
marching tetrahedra leaves within a hundredth of a voxel of each other.  The member placement keeps more of the volume than the mean, and both lose some."""
import numpy as np
import pytest

import mesh_decimate_reading as dr
import mesh_reading as mr


@pytest.fixture(scope="module")
def sphere():
    dims = (24, 20, 20)
    F = mr.sphere_volume(dims, [(8.3, 9.6, 10.2)], 6.2)
    verts, tris = mr.extract((0.0, 0.0, 0.0), 1.0, dims, F)
    assert verts.shape == (2146, 3) and tris.shape == (4288, 3)
    return verts, tris


def test_the_fixture_is_a_closed_sphere(sphere):
    verts, tris = sphere
    assert abs(dr.signed_volume(verts, tris) - 985.3) < 0.1
    assert 4.0 / 3.0 * np.pi * 6.2 ** 3 > dr.signed_volume(verts, tris)


@pytest.mark.parametrize("cell,n_v,n_t", [(2.0, 184, 364), (3.0, 84, 164)])
def test_whole_voxel_cells_keep_the_sphere_closed(sphere, cell, n_v, n_t):
    verts, tris = sphere
    for placement in ("mean", "member"):
        st = {}
        v, t, vmap = dr.decimate(verts, tris, cell, placement=placement, stats=st)
        assert (v.shape[0], t.shape[0]) == (n_v, n_t) and st["duplicates"] == 0 and st["collapsed"] == tris.shape[0] - n_t
        assert mr.closed_and_oriented(t) and mr.euler(v, t) == 2
        assert (vmap >= 0).all() and np.unique(vmap).shape[0] == n_v  # every vertex of the sphere is used, every cluster survives


def test_a_cell_of_one_and_a_half_voxels_makes_duplicates(sphere):
    verts, tris = sphere
    st = {}
    v, t, vmap = dr.decimate(verts, tris, 1.5, stats=st)
    assert (v.shape[0], t.shape[0]) == (285, 569) and st["duplicates"] == 9
    assert not mr.closed_and_oriented(t)
    # the duplicates named the same three clusters as a kept triangle, in either orientation
    s = np.sort(t.astype(np.int64), axis=1)
    assert np.unique(s, axis=0).shape[0] == t.shape[0]


def test_a_tiny_cell_only_welds(sphere):
    verts, tris = sphere
    st = {}
    v, t, vmap = dr.decimate(verts, tris, 0.01, stats=st)
    assert (v.shape[0], t.shape[0]) == (2138, 4272) and st["collapsed"] == 16 and st["duplicates"] == 0
    # where no vertex merged the position keeps its bytes
    rows, counts = np.unique(vmap, return_counts=True)
    assert rows[0] == 0 and int((counts - 1).sum()) == 8
    single = np.flatnonzero(np.isin(vmap, rows[counts == 1]))
    assert v[vmap[single]].tobytes() == verts[single].tobytes()
    merged = np.flatnonzero(np.isin(vmap, rows[counts > 1]))
    first = np.unique(vmap, return_index=True)[1]
    # the merged ones crowd around a lattice point the surface all but passes through: one cell of 0.01 holds them and their mean
    assert np.abs(verts[merged] - verts[first[vmap[merged]]]).max() < 0.01
    assert np.abs(v[vmap[merged]] - verts[merged]).max() < 0.01
    # the member placement gives every cluster the bytes of one of its members
    m = dr.decimate(verts, tris, 0.01, placement="member")
    hit = (verts == m[0][vmap]).all(axis=1)
    assert np.unique(vmap[hit]).shape[0] == v.shape[0] and hit[single].all()
    assert m[1].tobytes() == t.tobytes() and m[2].tobytes() == vmap.tobytes()


def test_volumes_and_counts_fall_in_order(sphere):
    verts, tris = sphere
    v_in = dr.signed_volume(verts, tris)
    sizes = []
    for cell in (2.0, 3.0):
        mean = dr.decimate(verts, tris, cell, placement="mean")
        member = dr.decimate(verts, tris, cell, placement="member")
        assert member[1].tobytes() == mean[1].tobytes() and member[2].tobytes() == mean[2].tobytes()  # placement moves positions only
        assert v_in > dr.signed_volume(*member[:2]) > dr.signed_volume(*mean[:2]) > 0
        # a member position is one of the cluster's own positions
        hit = (verts == member[0][member[2]]).all(axis=1)
        assert np.unique(member[2][hit]).shape[0] == member[0].shape[0]
        sizes.append((mean[0].shape[0], mean[1].shape[0]))
    small = dr.decimate(verts, tris, 1.5)
    sizes.insert(0, (small[0].shape[0], small[1].shape[0]))
    sizes.insert(0, (verts.shape[0], tris.shape[0]))
    assert all(a[0] > b[0] and a[1] > b[1] for a, b in zip(sizes, sizes[1:]))


def test_order_of_the_triangles_and_unused_vertices(sphere):
    verts, tris = sphere
    rng = np.random.default_rng(51)
    shuffled = tris[rng.permutation(tris.shape[0])]
    a, b = dr.decimate(verts, tris, 2.0), dr.decimate(verts, shuffled, 2.0)
    assert a[0].tobytes() == b[0].tobytes() and a[2].tobytes() == b[2].tobytes()  # no duplicates here: the same clusters survive
    assert np.array_equal(np.sort(np.sort(a[1], axis=1), axis=0), np.sort(np.sort(b[1], axis=1), axis=0))
    # an unused vertex takes no part, whatever its bytes
    more = np.concatenate([[[np.nan, 1e30, -np.inf]], verts, [[8.0, 9.0, 10.0]]]).astype(np.float32)
    c = dr.decimate(more, tris + 1, 2.0)
    assert c[0].tobytes() == a[0].tobytes() and c[1].tobytes() == a[1].tobytes()
    assert c[2][0] == -1 and c[2][-1] == -1 and c[2][1:-1].tobytes() == a[2].tobytes()


def test_refusals():
    verts = np.array([[0, 0, 0], [3, 0, 0], [0, 3, 0]], np.float32)
    tris = np.array([[0, 1, 2]], np.int32)
    assert dr.decimate(verts, tris, 1.0)[1].tolist() == [[0, 1, 2]]
    for bad in (np.nan, np.inf, -np.inf):
        w = verts.copy()
        w[1, 2] = bad
        with pytest.raises(dr.Refused):
            dr.decimate(w, tris, 1.0)
    with pytest.raises(dr.Refused):
        dr.decimate(verts, np.array([[0, 1, 3]], np.int32), 1.0)
    for cell in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(dr.Refused):
            dr.decimate(verts, tris, cell)
    # the ends of the grid are inside, one cell beyond is not
    for g, ok in ((-(1 << 20), True), ((1 << 20) - 1, True), (-(1 << 20) - 1, False), (1 << 20, False)):
        w = verts.copy()
        w[1, 0] = np.float32(g) + np.float32(0.5)
        if ok:
            dr.decimate(w, tris, 1.0)
        else:
            with pytest.raises(dr.Refused):
                dr.decimate(w, tris, 1.0)
