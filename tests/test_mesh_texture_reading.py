"""The numpy reading of the textured mesh (tests/mesh_texture_reading.py) against what the contract in include/mvskit_texture.h promises,
on the cameras of the plane scene (3 views of 96 x 64) with a float64 projection snapped to 1/256 pixel: the layout's invariants, a flat
and a ramp view through the perspective-correct lookup, the labels of a plane and a sphere, ties and shuffled triangles.  CPU only."""
import types

import numpy as np
import pytest

import mesh_fill_cases as mf
import mesh_render_reading as rr
import mesh_texture_reading as tr
from scene_support import cached_scene, grid_mesh

W, H = 96, 64


@pytest.fixture(scope="module")
def cams():
    sc = cached_scene(3, W, H, 20.0)
    return types.SimpleNamespace(P=[rr.camera64(sc.P[v], 0) for v in range(3)], centers=np.asarray(sc.centers, dtype=np.float64)[:, :3])


def project(P, verts):
    """-> (screens, vdepths, xys) per camera: the float64 projection snapped to 1/256, its depth, the unsnapped position"""
    out = [rr.project64(p, verts) for p in P]
    return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out]


def plane_grid(flip=False):
    verts, tris = grid_mesh(40, 30)
    verts = ((verts - np.float32([19.5, 14.5, 0.0])) * np.float32(0.02)).astype(np.float32)
    return verts, (tris[:, [0, 2, 1]] if flip else tris).copy()


def images(fill):
    return [fill(v) for v in range(3)]


@pytest.mark.parametrize("res", [1, 2, 8, 33])
def test_layout_invariants(res):
    B = res + 3
    for width in (B, 2 * B + 1, 256):
        for nt in (0, 1, 2, 7, 20):
            Bq, cpr, n_cells, height = tr.layout(nt, res, width)
            assert Bq == B and cpr == width // B and n_cells == 1 + (nt + 1) // 2 and height == -(-n_cells // cpr) * B
            h, k, n1, n2 = tr.owners(nt, res, width)
            assert h == height and k.shape == (height, width)
            flags = np.zeros(nt + 3, bool)
            flags[1:nt + 1] = True  # the first and the last two triangles are untextured
            uv = tr.corners(flags, res, width)
            assert (uv[~flags] == B // 2).all() and (k[uv[~flags][..., 1], uv[~flags][..., 0]] == -1).all()
            lower, upper = (res + 3) * (res + 4) // 2, B * B - (res + 3) * (res + 4) // 2
            for j in range(nt):
                # every texel of a textured half has one owner (k is one number per texel: the cells are disjoint), the half is whole
                assert int((k == j).sum()) == (upper if j % 2 else lower), (res, width, nt, j)
                cu = uv[1 + j]
                assert (k[cu[:, 1], cu[:, 0]] == j).all(), "a corner texel outside its own half"
                # and the weights there name the vertex: (res, 0, 0), (0, res, 0), (0, 0, res)
                w1, w2 = n1[cu[:, 1], cu[:, 0]], n2[cu[:, 1], cu[:, 0]]
                assert w1.tolist() == [0, res, 0] and w2.tolist() == [0, 0, res]
                yy, xx = np.nonzero(k == j)
                q = 1 + j // 2
                assert (xx // B == q % cpr).all() and (yy // B == q // cpr).all(), "a texel outside its cell"
            assert (k[:B, :B] == -1).all() and (k[:, cpr * B:] == -1).all()  # cell 0 and the right margin


def test_flat_view_gives_its_byte_everywhere(cams):
    verts, tris = plane_grid()
    screens, vdepths, _ = project(cams.P, verts)
    sizes = [(W, H)] * 3
    label, area, faces = tr.face_views(screens, vdepths, tris, sizes, [tr.front_sign(p) for p in cams.P])
    assert (label >= 0).all() and faces.sum() == tris.shape[0]
    for res in (1, 8):
        r = tr.texture(screens, vdepths, tris, label, images(lambda v: np.full((H, W, 3), 40 + 30 * v, np.uint8)), res, 256)
        assert r["n_textured"] == tris.shape[0]
        own = r["owner"] >= 0
        assert own.sum() == tris.shape[0] // 2 * (res + 3) ** 2
        want = (40 + 30 * label[r["owner"][own]]).astype(np.uint8)
        assert (r["atlas"][own] == want[:, None]).all(), "an owned texel, gutter included, is not its view's colour"
        assert (r["atlas"][~own] == 128).all()


def tilted_quad():
    """two triangles 57 x 34 pixels across, tilted so that their depths run from 3.4 to 4.6: the perspective shows"""
    verts, tris = grid_mesh(2, 2)
    verts = (verts - np.float32([0.5, 0.5, 0.0])) * np.float32([2.0, 1.2, 1.0])
    verts[:, 2] = np.float32(0.6) * verts[:, 0]
    return verts.astype(np.float32), tris


@pytest.mark.parametrize("mesh, res, least", [("grid", 8, 20000), ("quad", 33, 1000)])
def test_ramp_view_through_the_perspective_correct_lookup(cams, mesh, res, least):
    """The view is the ramp c(x) = 2 x + 3, which the bilinear lookup reproduces exactly.  An interior texel (n0, n1, n2 >= 0) stands
    for the 3-D point X = (n0 X0 + n1 X1 + n2 X2) / res, whose homogeneous image is sum(n_m d_m (x_m, y_m, 1)): with a_m = n_m d_m the
    projection of X is sum(a_m p_m) / sum(a_m) over the unsnapped positions p_m, exactly, and the contract's position is the same
    expression over the SNAPPED ones.  The weights a_m / sum(a) are a convex combination, so the two positions differ by no more than
    the largest snapping distance, sqrt(2) / 512 pixel, and the bytes by 0.5 (the rounding to a byte) plus the slope times that; 1e-9
    stands for the fp64 roundings of both chains.  On the tilted quad the depths differ by a third across a triangle: the screen-space
    affine map, or the weights n_m / d_m, would miss the bound there by whole pixels."""
    slope = 2.0
    verts, tris = plane_grid() if mesh == "grid" else tilted_quad()
    screens, vdepths, _ = project(cams.P, verts)
    label, _, _ = tr.face_views(screens, vdepths, tris, [(W, H)] * 3, [tr.front_sign(p) for p in cams.P])
    assert (label >= 0).all()
    ramp = (slope * np.arange(W) + 3.0).astype(np.uint8)
    r = tr.texture(screens, vdepths, tris, label, images(lambda v: np.broadcast_to(ramp[None, :, None], (H, W, 3)).copy()), res, 256)
    _, k, n1, n2 = tr.owners(r["n_textured"], res, 256)
    n0 = res - n1 - n2
    inner = (k >= 0) & (n0 >= 0) & (n1 >= 0) & (n2 >= 0)
    t = r["owner"][inner]
    X = (n0[inner][:, None] * verts[tris[t, 0]].astype(np.float64) + n1[inner][:, None] * verts[tris[t, 1]].astype(np.float64)
         + n2[inner][:, None] * verts[tris[t, 2]].astype(np.float64)) / res
    x = np.zeros(t.shape[0])
    for v in range(3):
        mine = label[t] == v
        x[mine] = rr.project64(cams.P[v], X[mine])[2][:, 0]
    bound = 0.5 + slope * np.sqrt(2.0) / 512 + 1e-9
    got = r["atlas"][inner][:, 0].astype(np.float64)
    err = np.abs(got - (slope * x + 3.0))
    print(f"ramp on the {mesh}: {inner.sum()} interior texels, largest error {err.max():.4f} of {bound:.4f}")
    assert inner.sum() > least and (err <= bound).all()
    assert (r["atlas"][..., 0] == r["atlas"][..., 1]).all() and (r["atlas"][..., 1] == r["atlas"][..., 2]).all()


def test_plane_is_labelled_and_its_flip_is_not(cams):
    assert (cams.centers[:, 2] > 0).all() and all(tr.front_sign(p) == -1 for p in cams.P)  # grid_mesh faces +z, where the cameras are
    sizes, signs = [(W, H)] * 3, [tr.front_sign(p) for p in cams.P]
    verts, tris = plane_grid()
    screens, vdepths, _ = project(cams.P, verts)
    label, area, faces = tr.face_views(screens, vdepths, tris, sizes, signs)
    assert (label >= 0).all() and (area > 0).all() and faces.tolist() == [int((label == v).sum()) for v in range(3)]
    flipped = plane_grid(flip=True)[1]
    label, area, faces = tr.face_views(screens, vdepths, flipped, sizes, signs)
    assert (label == -1).all() and (area == 0).all() and (faces == 0).all()
    both = tr.face_views(screens, vdepths, flipped, sizes, signs, front_only=False)
    assert (both[0] >= 0).all()
    # visibility: a view whose bit is missing on one vertex is no candidate for the triangles around it
    visible = np.full(verts.shape[0], 7, np.uint64)
    visible[0] = 6
    gated = tr.face_views(screens, vdepths, tris, sizes, signs, visible=visible)[0]
    assert (gated[(tris == 0).any(axis=1)] != 0).all()


def test_sphere_labels_face_their_view(cams):
    """With front_only a label is a view the face vector points towards.  The reading decides on the snapped vertices, the check on the
    float64 ones: moving each vertex by up to sqrt(2) / 2 units of 1/256 pixel changes the doubled area by at most sqrt(2) / 2 times the
    triangle's perimeter (each vertex sweeps the opposite edge) plus the second-order term 3 * (sqrt(2) / 2)^2 * 2, so a label whose
    |area| is above that bound cannot have changed sign.  Every labelled triangle is above it or faces its view."""
    verts, tris = mf.sphere()
    verts = ((verts - np.float32(mf.CENTRE)) * np.float32(0.5 / 6.2)).astype(np.float32)
    screens, vdepths, _ = project(cams.P, verts)
    label, area, faces = tr.face_views(screens, vdepths, tris, [(W, H)] * 3, [tr.front_sign(p) for p in cams.P])
    X = verts.astype(np.float64)[tris]
    face = np.cross(X[:, 1] - X[:, 0], X[:, 2] - X[:, 0])
    got = label >= 0
    towards = np.einsum("ij,ij->i", face, cams.centers[np.maximum(label, 0)] - X[:, 0]) > 0
    s = np.stack([screens[v][tris] for v in range(3)])[np.maximum(label, 0), np.arange(tris.shape[0])].astype(np.float64)
    perimeter = sum(np.linalg.norm(s[:, a] - s[:, b], axis=1) for a, b in ((0, 1), (1, 2), (2, 0)))
    safe = area > np.sqrt(0.5) * perimeter + 3.0
    print(f"sphere: {int(got.sum())} of {tris.shape[0]} triangles labelled, {int((got & ~safe).sum())} within the snapping bound")
    assert 0.3 * tris.shape[0] < got.sum() < 0.7 * tris.shape[0]  # the back has no label
    assert (towards | ~safe)[got].all() and (got & safe).sum() > 0.95 * got.sum()
    # and a triangle that faces a view squarely is labelled
    n = face / np.linalg.norm(face, axis=1, keepdims=True)
    for v in range(3):
        d = cams.centers[v] - X[:, 0]
        square = np.einsum("ij,ij->i", n, d / np.linalg.norm(d, axis=1, keepdims=True)) > 0.5
        assert got[square].all()


def test_a_tie_goes_to_the_lower_view(cams):
    verts, tris = plane_grid()
    P = [cams.P[1], cams.P[0], cams.P[1]]  # views 0 and 2 are one camera
    screens, vdepths, _ = project(P, verts)
    label, area, _ = tr.face_views(screens, vdepths, tris, [(W, H)] * 3, [tr.front_sign(p) for p in P])
    assert (label != 2).all() and (label == 0).any()
    a0, a2 = np.abs(tr.signed_area(screens[0], tris)), np.abs(tr.signed_area(screens[2], tris))
    assert (a0 == a2).all()


def test_shuffled_triangles_permute_the_results(cams):
    verts, tris = plane_grid()
    screens, vdepths, _ = project(cams.P, verts)
    sizes, signs = [(W, H)] * 3, [tr.front_sign(p) for p in cams.P]
    label, area, faces = tr.face_views(screens, vdepths, tris, sizes, signs)
    perm = np.random.RandomState(5).permutation(tris.shape[0])
    l2, a2, f2 = tr.face_views(screens, vdepths, tris[perm], sizes, signs)
    assert (l2 == label[perm]).all() and (a2 == area[perm]).all() and (f2 == faces).all()
    imgs = images(lambda v: np.random.RandomState(v).randint(0, 256, (H, W, 3)).astype(np.uint8))
    a, b = tr.texture(screens, vdepths, tris, label, imgs, 2, 64), tr.texture(screens, vdepths, tris[perm], l2, imgs, 2, 64)
    # per triangle the same texels under the same weights, whichever half of whichever cell it landed in
    for t in range(0, tris.shape[0], 97):
        ca, cb = tr.by_weights(a, 2, 64, perm[t]), tr.by_weights(b, 2, 64, t)
        common = set(ca) & set(cb)
        assert len(common) >= (2 + 2) * (2 + 3) // 2 and all(ca[w] == cb[w] for w in common)
