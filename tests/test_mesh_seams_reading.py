"""The numpy / Python reading of the seam calls (tests/mesh_seams_reading.py) against what include/mvskit_seams.h promises: the adjacency
on small meshes with fins, doubles and flipped pairs, a sphere and a grid; the smoothing's invariants on islands, fans and seeded random
quality tables; the levels on two identical cameras whose images differ by a constant.  CPU only."""
import numpy as np
import pytest

import mesh_fill_cases as mf
import mesh_fill_reading as fr
import mesh_render_reading as rr
import mesh_seams_reading as sr
import mesh_texture_reading as tr
from scene_support import cached_scene, grid_mesh

W, H = 96, 64


# ---- adjacency
def _check_adjacency(n_v, tris):
    tris = np.asarray(tris, np.int32).reshape(-1, 3)
    nbr, nirr = sr.adjacency(n_v, tris)
    assert nbr.dtype == np.int32 and nbr.shape == tris.shape
    assert nirr == fr.boundaries(n_v, tris)[4]
    for t in range(tris.shape[0]):
        for k in range(3):
            u = nbr[t, k]
            if u < 0:
                continue
            a, b = tris[t, k], tris[t, (k + 1) % 3]
            back = [j for j in range(3) if tris[u, j] == b and tris[u, (j + 1) % 3] == a]
            assert len(back) == 1 and nbr[u, back[0]] == t, (t, k)  # symmetric, and exactly the edge's two vertices
    # shuffled rows permute it
    perm = np.random.RandomState(5).permutation(tris.shape[0])
    inv = np.argsort(perm)
    snbr, snirr = sr.adjacency(n_v, tris[perm])
    want = nbr[perm]
    assert snirr == nirr and (snbr == np.where(want >= 0, inv[np.maximum(want, 0)], -1)).all()
    return nbr, nirr


def test_adjacency_small_cases():
    nbr, nirr = _check_adjacency(3, [[0, 1, 2]])
    assert (nbr == -1).all() and nirr == 0
    nbr, nirr = _check_adjacency(4, [[0, 1, 2], [2, 1, 3]])
    assert nbr.tolist() == [[-1, 1, -1], [0, -1, -1]] and nirr == 0
    # three on one edge: 1 -> 2 once, 2 -> 1 twice
    nbr, nirr = _check_adjacency(5, [[0, 1, 2], [2, 1, 3], [2, 1, 4]])
    assert (nbr == -1).all() and nirr == 1
    # a doubled triangle
    nbr, nirr = _check_adjacency(4, [[0, 1, 2], [0, 1, 2], [2, 1, 3]])
    assert (nbr == -1).all() and nirr == 3
    # (a, b, c) and (b, a, c): neighbours across all three edges
    nbr, nirr = _check_adjacency(3, [[0, 1, 2], [1, 0, 2]])
    assert nbr.tolist() == [[1, 1, 1], [0, 0, 0]] and nirr == 0
    # two equal ids: no edges
    nbr, nirr = _check_adjacency(4, [[0, 1, 2], [2, 1, 1], [2, 1, 3]])
    assert nbr.tolist() == [[-1, 2, -1], [-1, -1, -1], [0, -1, -1]] and nirr == 0
    assert sr.adjacency(0, np.zeros((0, 3), np.int32))[0].shape == (0, 3)
    with pytest.raises(fr.Refused):
        sr.adjacency(3, [[0, 1, 3]])


def test_adjacency_sphere_and_grid():
    verts, tris = mf.sphere()
    nbr, nirr = _check_adjacency(verts.shape[0], tris)
    assert nirr == 0 and (nbr >= 0).all()  # closed
    verts, tris = grid_mesh(40, 30)
    nbr, nirr = _check_adjacency(verts.shape[0], tris)
    assert nirr == 0 and int((nbr < 0).sum()) == 2 * (39 + 29)


# ---- smoothing
def _gains(nbr, quality, label, keep):
    return sr.proposals(nbr, quality, np.asarray(label, np.int64), keep)[1] >> 8


def _check_smoothing(n_v, tris, quality, label, keep=192, iterations=64):
    tris = np.asarray(tris, np.int32).reshape(-1, 3)
    quality, label = np.asarray(quality, np.uint8), np.asarray(label, np.int32)
    out, stats = sr.smooth_labels(n_v, tris, quality, label, keep, iterations)
    nbr, _ = sr.adjacency(n_v, tris)
    assert out.dtype == np.int32 and stats.dtype == np.int64
    assert stats[0] == sr.count_seams(nbr, label) and stats[1] == sr.count_seams(nbr, out) and stats[1] <= stats[0]
    assert stats[3] <= iterations and stats[2] >= stats[3] and (stats[2] == 0) == (out == label).all()
    if stats[2]:
        assert stats[1] < stats[0]
    changed = np.flatnonzero(out != label)
    assert (quality[changed, out[changed]] >= keep).all() and (label[changed] >= 0).all() and ((out == -1) == (label == -1)).all()
    if stats[3] < iterations:  # the loop ended by itself: nobody is left with a gain, unless two triangles on the same vertices tie
        left = np.flatnonzero(_gains(nbr, quality, out, keep) > 0)
        triples = [tuple(sorted(r)) for r in tris.tolist()]
        assert all(triples.count(triples[t]) > 1 for t in left)
    if iterations >= 64:
        assert stats[3] < 64, "did not end within the default iterations"
    perm = np.random.RandomState(6).permutation(tris.shape[0])
    sout, sstats = sr.smooth_labels(n_v, tris[perm], quality[perm], label[perm], keep, iterations)
    assert (sout == out[perm]).all() and (sstats == stats).all()
    return out, stats


def test_an_island_of_two_disappears():
    verts, tris = grid_mesh(6, 5)
    label = np.zeros(tris.shape[0], np.int32)
    nbr, _ = sr.adjacency(verts.shape[0], tris)
    t = 12
    u = int(nbr[t][nbr[t] >= 0][0])
    label[[t, u]] = 1
    quality = np.full((tris.shape[0], 2), 255, np.uint8)
    out, stats = _check_smoothing(verts.shape[0], tris, quality, label)
    assert (out == 0).all() and stats.tolist() == [4, 0, 2, 2]
    # an inadmissible view keeps the island
    quality[[t, u], 0] = 100
    out, stats = _check_smoothing(verts.shape[0], tris, quality, label)
    assert (out == label).all() and stats.tolist() == [4, 4, 0, 0]
    out, stats = _check_smoothing(verts.shape[0], tris, quality, label, keep=100)
    assert (out == 0).all()


def test_a_fan_of_four():
    tris = np.int32([[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 1]])
    quality = np.uint8([[255, 200], [200, 255], [255, 200], [200, 255]])
    label = np.int32([0, 1, 0, 1])
    out, stats = _check_smoothing(5, tris, quality, label)
    # every triangle has gain 2 towards the other label with quality 200: the smallest triple, (0, 1, 2), moves first and the rest follow it
    assert stats[1] == 0 and len(set(out.tolist())) == 1


def test_keep_255_on_the_labellings_own_quality_moves_nothing_without_ties():
    verts, tris = grid_mesh(40, 30)
    rng = np.random.RandomState(7)
    area = rng.randint(1, 1 << 20, (tris.shape[0], 3)).astype(np.int64)
    area[:, 1] += (area[:, 1] == area[:, 0]) | (area[:, 1] == area[:, 2])
    quality = np.maximum(1, 255 * area // area.max(axis=1, keepdims=True)).astype(np.uint8)
    label = area.argmax(axis=1).astype(np.int32)
    untied = (quality == 255).sum(axis=1) == 1
    out, stats = _check_smoothing(verts.shape[0], tris, quality, label, keep=255)
    assert (out[untied] == label[untied]).all()
    out, stats = _check_smoothing(verts.shape[0], tris, quality, label, keep=128)
    assert stats[2] > 0 and stats[1] < stats[0]


def test_iterations_zero_one_and_labels_of_minus_one():
    verts, tris = grid_mesh(12, 9)
    rng = np.random.RandomState(8)
    quality = rng.randint(0, 256, (tris.shape[0], 3)).astype(np.uint8)
    label = rng.randint(-1, 3, tris.shape[0]).astype(np.int32)
    out, stats = _check_smoothing(verts.shape[0], tris, quality, label, keep=64, iterations=0)
    assert (out == label).all() and stats[2] == 0 and stats[0] == stats[1]
    one, s1 = _check_smoothing(verts.shape[0], tris, quality, label, keep=64, iterations=1)
    full, sf = _check_smoothing(verts.shape[0], tris, quality, label, keep=64)
    assert s1[3] == 1 and 0 < s1[2] <= sf[2] and sf[1] <= s1[1] < s1[0]
    assert (full[label == -1] == -1).all()
    with pytest.raises(fr.Refused):
        sr.smooth_labels(verts.shape[0], tris, quality, np.full(tris.shape[0], 3, np.int32))


@pytest.mark.parametrize("nviews", [3, 12])
def test_random_quality_tables(nviews):
    verts, tris = grid_mesh(40, 30)
    rng = np.random.RandomState(nviews)
    quality = rng.randint(0, 256, (tris.shape[0], nviews)).astype(np.uint8)
    label = quality.argmax(axis=1).astype(np.int32)
    for keep in (128, 192):
        out, stats = _check_smoothing(verts.shape[0], tris, quality, label, keep=keep)
        print(f"{nviews} views, keep {keep}: seams {stats[0]} -> {stats[1]}, {stats[2]} moves in {stats[3]} iterations")
        assert stats[2] > 0


# ---- levelling
@pytest.fixture(scope="module")
def twins():
    """two identical cameras; the second image is the first plus 24 on every channel, the first scaled into 0 .. 231"""
    sc = cached_scene(3, W, H, 20.0)
    P = rr.camera64(sc.P[1], 0)
    rng = np.random.RandomState(9)
    base = (rng.randint(0, 256, (H, W, 3)).astype(np.int64) * 231 // 255).astype(np.uint8)
    verts, tris = grid_mesh(40, 30)
    verts = ((verts - np.float32([19.5, 14.5, 0.0])) * np.float32(0.02)).astype(np.float32)
    screen, vdepth = rr.project64(P, verts)[:2]
    vdepth = vdepth.astype(np.float32)  # as the device hands it out
    row = np.arange(tris.shape[0]) % (39 * 29)
    label = ((row % 39 + row // 39) % 2).astype(np.int32)  # a checkerboard over the cells
    return dict(screens=[screen, screen], vdepths=[vdepth, vdepth], verts=verts, tris=tris, images=[base, base + np.uint8(24)], label=label)


def test_levels_of_twin_cameras(twins):
    s = twins
    offset, pairs, n_edges = sr.seam_levels(s["screens"], s["vdepths"], s["tris"], s["label"], s["images"])
    nbr, _ = sr.adjacency(s["verts"].shape[0], s["tris"])
    assert n_edges == sr.count_seams(nbr, s["label"]) > 0
    N = pairs[0, 1, 0]
    assert N == 5 * n_edges >= 1000 and pairs[1, 0, 0] == N and (pairs[1, 0, 1:] == -pairs[0, 1, 1:]).all() and (pairs[[0, 1], [0, 1]] == 0).all()
    for ch in range(3):
        assert abs(pairs[0, 1, 1 + ch] / N + 384) <= 1
        assert abs(int(offset[1, ch]) - int(offset[0, ch]) + 384) <= 2
    # samples and max_shift reach their places
    assert sr.seam_pairs(s["screens"], s["vdepths"], s["tris"], s["label"], s["images"], samples=1)[0][0, 1, 0] == 2 * n_edges
    assert (sr.offsets(pairs, 0) == 0).all() and np.abs(sr.offsets(pairs, 5)).max() == 80
    # a view without a seam gets 0
    three = np.zeros((3, 3, 4), np.int64)
    three[:2, :2] = pairs
    assert (sr.offsets(three)[2] == 0).all() and (sr.offsets(three)[:2] == offset).all()


def test_the_levelled_atlas(twins):
    s = twins
    offset, _, _ = sr.seam_levels(s["screens"], s["vdepths"], s["tris"], s["label"], s["images"])
    args = (s["screens"], s["vdepths"], s["tris"])
    mixed = sr.texture_levelled(*args, s["label"], s["images"], offset, 2, 256)
    zeros = np.zeros_like(s["label"])
    alone = sr.texture_levelled(*args, zeros, s["images"], offset, 2, 256)
    assert mixed["n_textured"] == alone["n_textured"] == s["tris"].shape[0]
    assert np.abs(mixed["atlas"].astype(int) - alone["atlas"].astype(int)).max() <= 1
    plain = tr.texture(*args, s["label"], s["images"], 2, 256)
    assert np.abs(plain["atlas"].astype(int) - tr.texture(*args, zeros, s["images"], 2, 256)["atlas"].astype(int)).max() == 24
    # zero offsets reproduce texture()'s bytes
    for off in (None, np.zeros((2, 3), np.int32)):
        assert sr.texture_levelled(*args, s["label"], s["images"], off, 2, 256)["atlas"].tobytes() == plain["atlas"].tobytes()
    # the clamp to a byte
    bright = sr.texture_levelled(*args, s["label"], s["images"], np.full((2, 3), 16 * 255, np.int32), 2, 256)
    assert (bright["atlas"][bright["owner"] >= 0] == 255).all() and (bright["atlas"][bright["owner"] < 0] == 128).all()
