"""tests/mesh_fill_reading.py on its own (CPU): the boundary loops of the sphere of the prune test with triangles taken out, doubled or
stuck on, and of a flat grid whose rim is longer than a block; what filling makes of them.  The figures are the reading's on these
meshes: a missing triangle is a loop of 3 and comes back as itself, the ring around a vertex of valence 6 is a loop of 6 and gets a fan,
two holes that meet in a vertex are one complex component and stay, and the rim of an open surface is a loop that only max_edges keeps
open."""
import numpy as np
import pytest

import mesh_fill_cases as mc
import mesh_fill_reading as fr
import mesh_reading as mr
from scene_support import grid_mesh


def test_the_fixture():
    verts, tris = mc.sphere()
    assert verts.shape == (2146, 3) and tris.shape == (4288, 3) and mr.closed_and_oriented(tris)
    valence = np.bincount(tris.reshape(-1))
    assert (valence.min(), valence.max()) == (4, 9)
    assert mc.ring(tris, 500).shape[0] == 6 and mc.ring(tris, 1500).shape[0] == 6
    assert mc.touching_vertex(tris, 500) == 314


@pytest.mark.parametrize("name", list(mc.cases()))
def test_counts_lengths_and_what_is_filled(name):
    verts, tris, counts, lengths, max_edges, (new_v, new_t, n_filled) = mc.cases()[name]
    n_v = verts.shape[0]
    loop, length, *got = fr.boundaries(n_v, tris)
    assert tuple(got) == counts and mc.component_lengths(loop, length) == lengths
    assert ((loop == -1) == (length == 0)).all() and (loop[loop >= 0] <= np.flatnonzero(loop >= 0)).all()
    assert fr.closed(n_v, tris) == (counts == (0, 0, 0))
    v, t, nf = fr.fill(verts, tris, max_edges)
    assert (v.shape[0] - n_v, t.shape[0] - tris.shape[0], nf) == (new_v, new_t, n_filled)
    assert v[:n_v].tobytes() == verts.tobytes() and t[:tris.shape[0]].tobytes() == tris.tobytes()
    # a filled loop is gone, nothing else about the boundaries changes
    loop2, length2, *after = fr.boundaries(v.shape[0], t)
    gone = (length >= 3) & (length <= max_edges)
    assert tuple(after) == (counts[0] - n_filled, counts[1], counts[2])
    assert (loop2[:n_v] == np.where(gone, -1, loop)).all() and (length2[:n_v] == np.where(gone, 0, length)).all() and (loop2[n_v:] == -1).all()
    # the fill triangles lie in ascending order of their half-edge's origin, the corner in the middle
    assert (np.diff(t[tris.shape[0]:, 1]) > 0).all()


def test_a_missing_triangle_comes_back_as_itself():
    verts, tris = mc.sphere()
    v, t, nf = fr.fill(verts, np.delete(tris, 100, axis=0))
    assert nf == 1 and v.tobytes() == verts.tobytes() and mr.closed_and_oriented(t)
    back, lost = t[-1], tris[100]
    assert back[1] == lost.min() and any(np.array_equal(np.roll(back, s), lost) for s in range(3))  # (b, a, c) with a the label


@pytest.mark.parametrize("name", ["two_rings_out", "two_adjacent_rings_out"])
def test_fans_close_the_sphere(name):
    verts, tris, _, lengths, max_edges, _ = mc.cases()[name]
    v, t, nf = fr.fill(verts, tris, max_edges)
    assert mr.closed_and_oriented(t) and fr.closed(v.shape[0], t)
    n_v = verts.shape[0]
    # the centroid lies within rounding of the mean of its loop, inside the sphere
    loop, length, *_ = fr.boundaries(n_v, tris)
    labels = np.flatnonzero((loop == np.arange(n_v)) & (length >= 4))
    for row, label in enumerate(labels):
        mean = verts[loop == label].astype(np.float64).mean(axis=0)
        assert np.abs(v[n_v + row] - mean).max() < 2e-6 and np.linalg.norm(v[n_v + row] - mc.CENTRE) < 6.2
    if name == "two_adjacent_rings_out":
        used = np.zeros(v.shape[0], bool)
        used[t.reshape(-1)] = True
        assert np.flatnonzero(~used).tolist() == sorted([500, int(mc.ring(mc.sphere()[1], 500).min())])  # the two centres are unused now


def test_max_edges_decides():
    verts, tris, *_ = mc.cases()["two_rings_out"]
    assert fr.fill(verts, tris, 5)[2] == 0 and fr.fill(verts, tris, 6)[2] == 2
    gv, gt = grid_mesh(70, 70)
    v, t, nf = fr.fill(gv, gt, 276)
    assert nf == 1 and v[-1].tolist() == [34.5, 34.5, 0.0] and fr.closed(v.shape[0], t)
    assert fr.fill(gv, gt, 275)[0].shape == gv.shape
    with pytest.raises(fr.Refused):
        fr.fill(verts, tris, 2)


def test_one_triangle_and_its_mirror_image():
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    for tri in ([0, 1, 2], [2, 1, 0], [1, 2, 0]):
        loop, length, *counts = fr.boundaries(3, [tri])
        assert loop.tolist() == [0, 0, 0] and length.tolist() == [3, 3, 3] and counts == [1, 0, 0]
        v, t, nf = fr.fill(verts, [tri])
        assert nf == 1 and v.tobytes() == verts.tobytes() and mr.closed_and_oriented(t) and t[1, 1] == 0


def test_the_order_of_the_triangles_plays_no_part():
    verts, tris, *_ = mc.cases()["two_rings_out"]
    shuffled = tris[np.random.default_rng(71).permutation(tris.shape[0])]
    a, b = fr.fill(verts, tris), fr.fill(verts, shuffled)
    n_t = tris.shape[0]
    assert a[0].tobytes() == b[0].tobytes() and a[1][n_t:].tobytes() == b[1][n_t:].tobytes() and b[1][:n_t].tobytes() == shuffled.tobytes()
    for x, y in zip(fr.boundaries(verts.shape[0], tris), fr.boundaries(verts.shape[0], shuffled)):
        assert np.array_equal(x, y)


def test_repeated_ids_have_no_edges_and_are_copied_through():
    verts, tris = grid_mesh(9, 7)
    more = np.concatenate([[[3, 3, 5]], tris[:40], [[1, 1, 1], [8, 2, 8]], tris[40:], [[60, 61, 61]]]).astype(np.int32)
    for x, y in zip(fr.boundaries(63, tris), fr.boundaries(63, more)):
        assert np.array_equal(x, y)
    a, b = fr.fill(verts, tris), fr.fill(verts, more)
    assert a[2] == b[2] == 1 and a[0].tobytes() == b[0].tobytes() and b[1][:more.shape[0]].tobytes() == more.tobytes()
    assert a[1][tris.shape[0]:].tobytes() == b[1][more.shape[0]:].tobytes()


def test_non_finite_positions_and_bad_ids():
    verts, tris, *_ = mc.cases()["two_rings_out"]
    loop, length, *_ = fr.boundaries(verts.shape[0], tris)
    on_loop, interior = int(np.flatnonzero(loop >= 0)[3]), int(np.flatnonzero(loop < 0)[0])
    want = fr.fill(verts, tris)
    for bad in (np.nan, np.inf, -np.inf):
        w = verts.copy()
        w[on_loop, 1] = bad
        with pytest.raises(fr.Refused, match="loop vertex"):
            fr.fill(w, tris)
        assert fr.fill(w, tris, 5)[2] == 0  # a loop that is not filled
        w = verts.copy()
        w[[500, interior], 2] = bad  # an unused vertex and an interior one
        got = fr.fill(w, tris)
        assert got[0][verts.shape[0]:].tobytes() == want[0][verts.shape[0]:].tobytes() and got[1].tobytes() == want[1].tobytes()
    t = tris.copy()
    t[7, 0] = verts.shape[0]
    w = verts.copy()
    w[on_loop, 1] = np.nan
    with pytest.raises(fr.Refused, match="index"):  # a bad id is reported before a bad loop vertex
        fr.fill(w, t)
    with pytest.raises(fr.Refused, match="index"):
        fr.boundaries(verts.shape[0], t)


def test_zeros_of_either_sign_give_plus_zero():
    verts = np.array([[0.0, -0.0, 0.0], [-0.0, -0.0, -0.0], [0.0, 0.0, 0.0], [-0.0, 0.0, -0.0], [5.0, 5.0, 5.0]], np.float32)
    tris = np.array([[0, 1, 4], [1, 2, 4], [2, 3, 4], [3, 0, 4]], np.int32)  # a closed cone without its base: the loop 0 <- 1 <- 2 <- 3
    loop, length, *counts = fr.boundaries(5, tris)
    assert counts == [1, 0, 0] and length.tolist() == [4, 4, 4, 4, 0]
    v, t, nf = fr.fill(verts, tris)
    assert nf == 1 and v[5].tobytes() == np.zeros(3, np.float32).tobytes() and mr.closed_and_oriented(t)


def test_the_fan_of_the_decimation_test():
    verts, tris = mc.fan()
    loop, length, *counts = fr.boundaries(verts.shape[0], tris)
    assert counts == [1, 0, 0] and loop[0] == -1 and (loop[1:] == 1).all() and (length[1:] == 19999).all()
    assert fr.fill(verts, tris, 64)[2] == 0
    v, t, nf = fr.fill(verts, tris, 1 << 30)
    assert nf == 1 and v.shape[0] == 20001 and t.shape[0] == 2 * 19999 and mr.closed_and_oriented(t)
    assert np.abs(v[-1] - verts[1:].astype(np.float64).mean(axis=0)).max() < 1e-6
