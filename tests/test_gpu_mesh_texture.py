"""mvs_engine_mesh_face_views and mvs_engine_mesh_texture on the GPU against tests/mesh_texture_reading.py.  The device's own screen and
vdepth (Engine.mesh_screen) and its own pyramid level (Engine.pyramid) go into the reading, which leaves integer arithmetic and an IEEE
fp64 chain between the two: label, area, n_faces, height, n_textured, uv and every byte of the atlas are compared for equality, with no
margins and nothing left out.  Each call is made once through Python with host arrays and once through the C ABI with device tensors.
Engines have views only (no pool); 3 views of 96 x 64 around the plane z = 0 unless a case says otherwise."""
import ctypes as C

import numpy as np
import pytest
import torch

import camera_scenes as cs
import mesh_fill_cases as mf
import mesh_render_reading as rr
import mesh_texture_reading as tr
from mvskit_amd import engine
from mvskit_amd.engine import MVS_ERR_ARG, MVS_ERR_CAPACITY, MVS_ERR_STATE
from scene_support import cached_scene, grid_mesh

pytestmark = pytest.mark.gpu
vp = C.c_void_p
FOOT = 4.0 / (765.702941895 * 96 / 640.0)  # world units a pixel at the target


def _engine(sc, sizes=None, level=0, **kw):
    e = engine.Engine(sc.nviews, level=level, **kw)
    e.set_scene(sc, sizes=sizes)
    return e


@pytest.fixture(scope="module")
def plane():
    sc = cached_scene(3, 96, 64, 20.0)
    e = _engine(sc)
    yield e, sc
    e.close()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _face_views_device(e, x, verts, tris, visible):
    """the labelling through the C ABI with every array in device memory -> (label, area, n_faces) as numpy"""
    n, n_t = e.cfg.nviews, tris.shape[0]
    dV, dT = _dev(verts.reshape(-1)), _dev(tris.reshape(-1))
    dvis = None if visible is None else _dev(visible.view(np.int64))
    dl = torch.full((n_t + 1,), -7, dtype=torch.int32, device="cuda")
    da = torch.full((n_t + 1,), -7, dtype=torch.int64, device="cuda")
    df = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
    e._check(e.L.mvs_engine_mesh_face_views(e.h, C.byref(x), verts.shape[0], vp(dV.data_ptr()), n_t, vp(dT.data_ptr()), None if dvis is None else vp(dvis.data_ptr()),
                                            vp(dl.data_ptr()), vp(da.data_ptr()), vp(df.data_ptr())))
    torch.cuda.synchronize()
    assert int(dl[-1]) == -7 and int(da[-1]) == -7 and int(df[-1]) == -7, "a write behind label, area or n_faces"
    return dl[:-1].cpu().numpy(), da[:-1].cpu().numpy(), df[:-1].cpu().numpy()


def _texture_device(e, x, verts, tris, label):
    """the atlas through the C ABI with every array in device memory: the size call, then the full call -> (atlas, uv, height, n_textured)"""
    n_t = tris.shape[0]
    dV, dT, dL = _dev(verts.reshape(-1)), _dev(tris.reshape(-1)), _dev(label)
    h, n = C.c_int64(-7), C.c_int64(-7)
    head = (e.h, C.byref(x), verts.shape[0], vp(dV.data_ptr()), n_t, vp(dT.data_ptr()), vp(dL.data_ptr()))
    duv = torch.full((n_t * 6 + 1,), -7, dtype=torch.int32, device="cuda")
    e._check(e.L.mvs_engine_mesh_texture(*head, 0, None, vp(duv.data_ptr()), C.byref(h), C.byref(n)))
    torch.cuda.synchronize()
    assert int((duv != -7).sum()) == 0, "the size call wrote uv"
    height = h.value
    drgb = torch.full((height * x.width * 3 + 1,), 7, dtype=torch.uint8, device="cuda")
    e._check(e.L.mvs_engine_mesh_texture(*head, height, vp(drgb.data_ptr()), vp(duv.data_ptr()), C.byref(h), C.byref(n)))
    torch.cuda.synchronize()
    assert int(drgb[-1]) == 7 and int(duv[-1]) == -7 and h.value == height, "a write behind rgb or uv"
    return drgb[:-1].cpu().numpy().reshape(height, x.width, 3), duv[:-1].cpu().numpy().reshape(n_t, 3, 2), height, n.value


def check(e, sc, verts, tris, res=8, width=256, visible=None, front_only=True, label=None):
    """every check of the module's docstring on one mesh -> dict(label, area, faces, atlas, uv, height, n_textured, reading, screen,
    vdepth).  label: forced labels for the atlas (default: the labelling's own)"""
    verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    tris = np.ascontiguousarray(tris, dtype=np.int32).reshape(-1, 3)
    n, level = e.cfg.nviews, e.cfg.level
    shapes = [e.level_shape(v) for v in range(n)]
    sizes = [(w, h) for h, w in shapes]
    screen, vdepth = e.mesh_screen(verts, tris)
    images = [e.pyramid(v, level) for v in range(n)]
    signs = [tr.front_sign(rr.camera64(sc.P[v], level)) for v in range(n)]
    x = engine.MeshTexturing(res, width, int(front_only), 0)
    # the labelling: Python with host arrays, the C ABI with device tensors, the reading
    got = e.mesh_face_views(verts, tris, visible=visible, front_only=front_only)
    dev = _face_views_device(e, x, verts, tris, visible)
    want = tr.face_views(list(screen), list(vdepth), tris, sizes, signs, visible=visible, front_only=front_only)
    for name, a, b, c in zip(("label", "area", "n_faces"), got, dev, want):
        assert a.dtype == c.dtype and a.tobytes() == b.tobytes(), f"{name}: two calls give different bytes"
        assert a.tobytes() == c.tobytes(), f"{name}: {int((a != c).sum())} values differ from the reading"
    # the atlas under those labels, or the forced ones
    lab = got[0] if label is None else np.ascontiguousarray(label, dtype=np.int32)
    atlas, uv, nt = e.texture_mesh(verts, tris, lab, res=res, width=width)
    datlas, duv, dheight, dnt = _texture_device(e, x, verts, tris, lab)
    r = tr.texture(list(screen), list(vdepth), tris, lab, images, res, width)
    assert atlas.shape == (r["height"], width, 3) and dheight == r["height"], f"height {atlas.shape[0]}, {dheight} against {r['height']}"
    assert nt == dnt == r["n_textured"], f"n_textured {nt}, {dnt} against {r['n_textured']}"
    assert uv.tobytes() == duv.tobytes() and atlas.tobytes() == datlas.tobytes(), "two calls give different bytes"
    assert uv.tobytes() == r["uv"].tobytes(), f"{int((uv != r['uv']).any(axis=(1, 2)).sum())} triangles' uv differ from the reading"
    diff = (atlas != r["atlas"]).any(axis=2)
    assert atlas.tobytes() == r["atlas"].tobytes(), f"{int(diff.sum())} of {diff.size} texels differ from the reading, the first at {np.argwhere(diff)[:3].tolist()}"
    return dict(label=got[0], area=got[1], faces=got[2], atlas=atlas, uv=uv, height=atlas.shape[0], n_textured=nt, reading=r, screen=screen, vdepth=vdepth)


def small_grid(z=0.0, wobble=0.02):
    """grid_mesh(40, 30) at 0.02: triangles of half a pixel, on a gently waved surface"""
    verts, tris = grid_mesh(40, 30)
    verts = (verts - np.float32([19.5, 14.5, 0.0])) * np.float32(0.02)
    verts[:, 2] = z + wobble * np.sin(9.0 * verts[:, 0]) * np.cos(7.0 * verts[:, 1])
    return verts.astype(np.float32), tris


def coarse_grid(z=0.0):
    """3 x 3 vertices, ten times the image's footprint across"""
    verts, tris = grid_mesh(3, 3)
    verts = (verts - np.float32([1.0, 1.0, 0.0])) * np.float32([5.0 * 96 * FOOT, 5.0 * 64 * FOOT, 1.0])
    verts[:, 2] = z
    return verts.astype(np.float32), tris


def sphere():
    verts, tris = mf.sphere()
    return ((verts - np.float32(mf.CENTRE)) * np.float32(0.5 / 6.2)).astype(np.float32), tris.copy()


def unproject(sc, v, uvd):
    """world points of (u, v, depth) in view v at level 0, float64"""
    P = sc.P[v].astype(np.float64)
    uvd = np.asarray(uvd, dtype=np.float64)
    rhs = np.stack([uvd[:, 0] * uvd[:, 2], uvd[:, 1] * uvd[:, 2], uvd[:, 2]], axis=1) - P[:, 3]
    return np.linalg.solve(P[:, :3], rhs.T).T


def test_small_triangles(plane):
    e, sc = plane
    verts, tris = small_grid()
    r = check(e, sc, verts, tris, res=2, width=256)
    print("small grid: faces", r["faces"].tolist(), "atlas", r["atlas"].shape)
    assert (r["label"] >= 0).all() and r["n_textured"] == tris.shape[0] and r["faces"].sum() == tris.shape[0]
    own = r["reading"]["owner"] >= 0
    assert (r["atlas"][own] != 128).any() and (r["atlas"][~own] == 128).all()
    # the flipped mesh faces no view
    f = check(e, sc, verts, tris[:, [0, 2, 1]], res=2, width=256)
    assert (f["label"] == -1).all() and f["n_textured"] == 0 and f["height"] == 5 and (f["atlas"] == 128).all()
    b = check(e, sc, verts, tris[:, [0, 2, 1]], res=2, width=256, front_only=False)
    assert (b["label"] >= 0).all()


def test_coarse_grid_window_clamp_and_grey_paths(plane):
    e, sc = plane
    verts, tris = coarse_grid()
    r = check(e, sc, verts, tris, res=8)
    print("coarse grid: labels", r["label"].tolist())
    assert (r["label"] == -1).all()  # gate (b): no triangle has its three vertices inside a view
    # forced labels: every vertex is usable in every view, the texels clamp at all four borders of view 1
    r = check(e, sc, verts, tris, res=8, label=np.full(tris.shape[0], 1, np.int32))
    xy = r["reading"]["xy"]
    assert r["n_textured"] == tris.shape[0]
    assert (xy[..., 0] < 0).any() and (xy[..., 0] > 95).any() and (xy[..., 1] < 0).any() and (xy[..., 1] > 63).any()
    assert ((xy[..., 0] > 1) & (xy[..., 0] < 94) & (xy[..., 1] > 1) & (xy[..., 1] < 62)).any()
    # a vertex behind camera 1 dishonours its triangles' labels; one next to the camera makes den <= 0 in a gutter at res 1: grey texels
    # inside an owned half
    behind = verts.copy()
    behind[4] = unproject(sc, 1, [[48.0, 32.0, -1.0]])[0]
    r = check(e, sc, behind, tris, res=8, label=np.full(tris.shape[0], 1, np.int32))
    touched = (tris == 4).any(axis=1)
    assert r["reading"]["flags"].tolist() == (~touched).tolist() and 0 < r["n_textured"] < tris.shape[0]
    near = unproject(sc, 1, [[10.0, 10.0, 8.0], [80.0, 12.0, 1.0], [40.0, 55.0, 1.2]]).astype(np.float32)
    r = check(e, sc, near, np.int32([[0, 1, 2]]), res=1, front_only=False, label=np.int32([1]))
    own = r["reading"]["owner"] == 0
    assert r["n_textured"] == 1 and np.isnan(r["reading"]["xy"][own]).any() and (~np.isnan(r["reading"]["xy"][own])).any()


def test_sphere_with_and_without_visibility(plane):
    e, sc = plane
    verts, tris = sphere()
    r = check(e, sc, verts, tris, res=8, width=512)
    visible = e.mesh_visibility(verts, tris)
    g = check(e, sc, verts, tris, res=8, width=512, visible=visible)
    print("sphere:", tris.shape[0], "triangles, labelled", int((r["label"] >= 0).sum()), "and", int((g["label"] >= 0).sum()), "with the visibility")
    assert ((g["label"] >= 0) <= (r["label"] >= 0)).all() and 0 < (g["label"] >= 0).sum() <= (r["label"] >= 0).sum()
    # back triangles get no label: a triangle that looks away from every camera by more than the snapping can hide (a cosine of 0.02:
    # test_mesh_texture_reading.test_sphere_labels_face_their_view has the bound, these triangles are 2 pixels across)
    X = verts.astype(np.float64)[tris]
    face = np.cross(X[:, 1] - X[:, 0], X[:, 2] - X[:, 0])
    face /= np.linalg.norm(face, axis=1, keepdims=True)
    rays = [np.asarray(sc.centers[v], dtype=np.float64)[:3] - X.mean(axis=1) for v in range(3)]
    away = np.all([np.einsum("ij,ij->i", face, d / np.linalg.norm(d, axis=1, keepdims=True)) < -0.02 for d in rays], axis=0)
    assert away.sum() > 0.3 * tris.shape[0] and (r["label"][away] == -1).all() and (g["label"][away] == -1).all()


def test_shuffled_triangles(plane):
    e, sc = plane
    verts, tris = small_grid()
    perm = np.random.RandomState(11).permutation(tris.shape[0])
    a, b = check(e, sc, verts, tris, res=2, width=128), check(e, sc, verts, tris[perm], res=2, width=128)
    assert (b["label"] == a["label"][perm]).all() and (b["area"] == a["area"][perm]).all() and (b["faces"] == a["faces"]).all()
    ra, rb = dict(a["reading"], atlas=a["atlas"]), dict(b["reading"], atlas=b["atlas"])
    for t in range(0, tris.shape[0], 61):
        ca, cb = tr.by_weights(ra, 2, 128, perm[t]), tr.by_weights(rb, 2, 128, t)
        common = set(ca) & set(cb)
        assert len(common) >= 10 and all(ca[w] == cb[w] for w in common), t


@pytest.mark.parametrize("res", [1, 8, 33])
def test_resolutions_and_the_narrowest_atlas(plane, res):
    e, sc = plane
    verts, tris = small_grid()
    keep = slice(0, 301)  # an odd number of triangles: the last upper half is grey
    r = check(e, sc, verts, tris[keep], res=res, width=4 * (res + 3) + 1)
    B = res + 3
    assert r["n_textured"] == 301 and r["height"] == -(-152 // 4) * B
    q = 151
    cell = r["atlas"][(q // 4) * B:(q // 4 + 1) * B, (q % 4) * B:(q % 4 + 1) * B]
    i, j = np.meshgrid(np.arange(B), np.arange(B))
    assert (cell[i + j >= res + 3] == 128).all() and (cell[i + j <= res + 2] != 128).any()
    # width == B: one cell a row
    n = check(e, sc, verts, tris[keep], res=res, width=B)
    assert n["height"] == 152 * B and (n["uv"][:, :, 0] < B).all()


def test_all_labels_minus_one_and_empty_inputs(plane):
    e, sc = plane
    verts, tris = small_grid()
    r = check(e, sc, verts, tris, res=8, label=np.full(tris.shape[0], -1, np.int32))
    assert r["n_textured"] == 0 and r["atlas"].shape == (11, 256, 3) and (r["atlas"] == 128).all() and (r["uv"] == 5).all()
    for v_, t_ in ((verts, np.zeros((0, 3), np.int32)), (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))):
        r = check(e, sc, v_, t_, res=8)
        assert r["label"].shape == (0,) and (r["faces"] == 0).all() and r["atlas"].shape == (11, 256, 3) and (r["atlas"] == 128).all() and r["uv"].shape == (0, 3, 2)


def test_a_dishonoured_forced_label(plane):
    e, sc = plane
    verts, tris = small_grid()
    verts, tris = verts.copy(), tris[:40].copy()
    # triangle 3 collapses to a point (no area anywhere); triangle 5 gets a vertex that no view can use
    tris[3] = tris[3, 0]
    verts = np.concatenate([verts, np.float32([[np.nan, 0.0, 0.0]])])
    tris[5, 2] = verts.shape[0] - 1
    label = np.full(40, 2, np.int32)
    label[7] = -1
    r = check(e, sc, verts, tris, res=8, label=label)
    want = np.ones(40, bool)
    want[[3, 5, 7]] = False
    assert r["reading"]["flags"].tolist() == want.tolist() and r["n_textured"] == 37
    assert (r["uv"][[3, 5, 7]] == 5).all() and (r["label"][[3, 5]] == -1).all()


def test_odd_views():
    sc = cached_scene(3, 97, 61, 20.0)
    e = _engine(sc)
    verts, tris = small_grid()
    r = check(e, sc, verts, tris, res=2)
    assert (r["label"] >= 0).all()
    cv, ct = coarse_grid()
    check(e, sc, cv, ct, res=8, label=np.int32([0, 1, 2, 0, 1, 2, 0, 1]))
    e.close()


def test_unequal_view_sizes(plane):
    _, sc = plane
    e = _engine(sc, sizes=[(96, 64), (80, 50), (61, 64)])
    verts, tris = small_grid()
    r = check(e, sc, verts * np.float32(3.0), tris, res=2)  # wider than the smaller views: gate (b) differs from view to view
    print("unequal views: faces", r["faces"].tolist())
    assert (r["faces"] > 0).sum() >= 2
    cv, ct = coarse_grid()
    check(e, sc, cv, ct, res=8, label=np.int32([0, 1, 2, 0, 1, 2, 0, 1]))
    e.close()


def test_level_one(plane):
    _, sc = plane
    e = _engine(sc, level=1)
    verts, tris = small_grid()
    r = check(e, sc, verts, tris, res=2)
    assert e.level_shape(0) == (32, 48) and (r["label"] >= 0).all()
    cv, ct = coarse_grid()
    check(e, sc, cv, ct, res=8, label=np.int32([0, 1, 2, 0, 1, 2, 0, 1]))
    e.close()


def test_size_call_and_capacity(plane):
    e, sc = plane
    verts, tris = small_grid()
    label = e.mesh_face_views(verts, tris)[0]
    x = engine.MeshTexturing(8, 256, 1, 0)
    h, n = C.c_int64(-7), C.c_int64(-7)
    head = (e.h, C.byref(x), verts.shape[0], verts.ctypes.data_as(vp), tris.shape[0], tris.ctypes.data_as(vp), label.ctypes.data_as(vp))
    uv = np.full((tris.shape[0], 3, 2), -7, np.int32)
    assert e.L.mvs_engine_mesh_texture(*head, 0, None, uv.ctypes.data_as(vp), C.byref(h), C.byref(n)) == 0
    height = tr.layout(tris.shape[0], 8, 256)[3]
    assert (h.value, n.value) == (height, tris.shape[0]) and (uv == -7).all()
    rgb = np.full((height, 256, 3), 7, np.uint8)
    h.value = n.value = -7
    assert e.L.mvs_engine_mesh_texture(*head, height - 1, rgb.ctypes.data_as(vp), uv.ctypes.data_as(vp), C.byref(h), C.byref(n)) == MVS_ERR_CAPACITY
    assert b"cap_h" in e.L.mvs_last_error() and (h.value, n.value) == (height, tris.shape[0]) and (uv == -7).all() and (rgb == 7).all()
    # an atlas higher than 32768: res 33 in a width of one cell
    x = engine.MeshTexturing(33, 36, 1, 0)
    head = (e.h, C.byref(x)) + head[2:]
    assert e.L.mvs_engine_mesh_texture(*head, 1 << 20, rgb.ctypes.data_as(vp), uv.ctypes.data_as(vp), C.byref(h), C.byref(n)) == MVS_ERR_CAPACITY
    assert h.value == (1 + tris.shape[0] // 2) * 36 > 32768 and (uv == -7).all() and (rgb == 7).all()


def test_bad_id_and_bad_label_write_nothing(plane):
    e, sc = plane
    verts, tris = small_grid()
    x = engine.MeshTexturing(8, 256, 1, 0)
    good = e.mesh_face_views(verts, tris)[0]
    label, area, faces = np.full(tris.shape[0], -7, np.int32), np.full(tris.shape[0], -7, np.int64), np.full(3, -7, np.int64)
    rgb, uv = np.full((4096, 256, 3), 7, np.uint8), np.full((tris.shape[0], 3, 2), -7, np.int32)
    h, n = C.c_int64(-7), C.c_int64(-7)
    for bad in (-1, verts.shape[0], 1 << 30):
        t = tris.copy()
        t[tris.shape[0] // 2, 1] = bad
        p = [a.ctypes.data_as(vp) for a in (verts, t, label, area, faces, good, rgb, uv)]
        assert e.L.mvs_engine_mesh_face_views(e.h, C.byref(x), verts.shape[0], p[0], t.shape[0], p[1], None, p[2], p[3], p[4]) == MVS_ERR_ARG
        assert b"index outside" in e.L.mvs_last_error()
        assert e.L.mvs_engine_mesh_texture(e.h, C.byref(x), verts.shape[0], p[0], t.shape[0], p[1], p[5], 4096, p[6], p[7], C.byref(h), C.byref(n)) == MVS_ERR_ARG
        assert b"index outside" in e.L.mvs_last_error()
    for bad in (-2, 3, 1 << 20):
        lab = good.copy()
        lab[17] = bad
        assert e.L.mvs_engine_mesh_texture(e.h, C.byref(x), verts.shape[0], verts.ctypes.data_as(vp), tris.shape[0], tris.ctypes.data_as(vp), lab.ctypes.data_as(vp),
                                           4096, rgb.ctypes.data_as(vp), uv.ctypes.data_as(vp), C.byref(h), C.byref(n)) == MVS_ERR_ARG
        assert b"label outside" in e.L.mvs_last_error()
    for a in (label, area, faces, uv):
        assert (a == -7).all()
    assert (rgb == 7).all() and (h.value, n.value) == (-7, -7)


def test_state_errors():
    e = engine.Engine(3)
    verts, tris = coarse_grid()
    with pytest.raises(engine.EngineError) as err:
        e.mesh_face_views(verts, tris)
    assert err.value.status == MVS_ERR_STATE and "views not set" in str(err.value)
    with pytest.raises(engine.EngineError) as err:
        e.texture_mesh(verts, tris, np.zeros(tris.shape[0], np.int32))
    assert err.value.status == MVS_ERR_STATE and "views not set" in str(err.value)
    e.close()


@pytest.mark.parametrize("family", ["roll", "mixed"])
def test_camera_families(family):
    sc = cs.reading_scene(family)
    e = _engine(sc)
    T = np.float32(sc.meta["target"])
    verts, tris = small_grid()
    r = check(e, sc, verts + T, tris, res=2)
    print(family, "faces", r["faces"].tolist())
    assert (r["label"] >= 0).sum() > 0.9 * tris.shape[0]
    cv, ct = coarse_grid()
    check(e, sc, cv * np.float32([0.5, 0.5, 1.0]) + T, ct, res=8, label=np.int32([0, 1, 2, 0, 1, 2, 0, 1]))
    e.close()
