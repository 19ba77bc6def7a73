"""The seam calls of include/mvskit_seams.h on the GPU against tests/mesh_seams_reading.py, on the meshes and the scene of
tests/test_gpu_mesh_texture.py.  The device's own screen and vdepth (Engine.mesh_screen) and its own pyramid level (Engine.pyramid) go
into the reading, which leaves integer arithmetic and IEEE fp64 chains between the two: nbr, n_irregular, quality, label_out, stats,
pairs, n_seam_edges, offset and the levelled atlas with its uv are compared for equality, with no margins and nothing left out.  Each call
is made once through Python with host arrays and once through the C ABI with device tensors, a guard element behind every output."""
import ctypes as C

import numpy as np
import pytest
import torch

import camera_scenes as cs
import mesh_render_reading as rr
import mesh_seams_reading as sr
import mesh_texture_reading as tr
from maps_reading import DEPTH_TOL, NORMAL_COS
from mvskit_amd import engine, synth
from mvskit_amd.engine import MVS_ERR_ARG, MVS_ERR_STATE
from scene_support import PLAIN, cached_scene, engine_with_pool, lattice
from test_gpu_mesh_texture import _dev, _engine, coarse_grid, small_grid, sphere

pytestmark = pytest.mark.gpu
vp = C.c_void_p


@pytest.fixture(scope="module")
def plane():
    sc = cached_scene(3, 96, 64, 20.0)
    e = _engine(sc)
    yield e, sc
    e.close()


def noisy(n_t, nviews):
    """a label drawn at random for every triangle: seams at most edges, and most triangles with a gain"""
    return np.random.RandomState(3).randint(0, nviews, n_t).astype(np.int32)


def _guarded(n, dtype, fill=-7):
    return torch.full((n + 1,), fill, dtype=dtype, device="cuda")


def _take(t, shape, fill=-7):
    torch.cuda.synchronize()
    assert int(t[-1]) == fill, "a write behind an output"
    return t[:-1].cpu().numpy().reshape(shape)


def _device_calls(e, verts, tris, visible, front_only, seams, label_in, label_tex, offset, res, width):
    """the five calls through the C ABI with every array in device memory -> dict of numpy results"""
    n, n_v, n_t = e.cfg.nviews, verts.shape[0], tris.shape[0]
    dV, dT = _dev(verts.reshape(-1)), _dev(tris.reshape(-1))
    dvis = None if visible is None else _dev(visible.view(np.int64))
    x = engine.MeshTexturing(res, width, int(front_only), 0)
    out = {}
    dn, ni = _guarded(3 * n_t, torch.int32), C.c_int64(-7)
    e._check(e.L.mvs_engine_mesh_adjacency(e.h, n_v, n_t, vp(dT.data_ptr()), vp(dn.data_ptr()), C.byref(ni)))
    out["nbr"], out["n_irregular"] = _take(dn, (n_t, 3)), ni.value
    dq = _guarded(n_t * n, torch.uint8, 7)
    e._check(e.L.mvs_engine_mesh_face_quality(e.h, C.byref(x), n_v, vp(dV.data_ptr()), n_t, vp(dT.data_ptr()), None if dvis is None else vp(dvis.data_ptr()),
                                              vp(dq.data_ptr())))
    out["quality"] = _take(dq, (n_t, n), 7)
    dl, ds = _guarded(n_t, torch.int32), _guarded(4, torch.int64)
    dli = _dev(label_in)
    e._check(e.L.mvs_engine_mesh_smooth_labels(e.h, C.byref(seams), n_v, n_t, vp(dT.data_ptr()), n, vp(dq.data_ptr()), vp(dli.data_ptr()), vp(dl.data_ptr()),
                                               vp(ds.data_ptr())))
    out["label"], out["stats"] = _take(dl, (n_t,)), _take(ds, (4,))
    do, dp, ne = _guarded(3 * n, torch.int32), _guarded(4 * n * n, torch.int64), C.c_int64(-7)
    dlt = _dev(label_tex)
    e._check(e.L.mvs_engine_mesh_seam_levels(e.h, C.byref(seams), C.byref(x), n_v, vp(dV.data_ptr()), n_t, vp(dT.data_ptr()), vp(dlt.data_ptr()), vp(do.data_ptr()),
                                             vp(dp.data_ptr()), C.byref(ne)))
    out["offset"], out["pairs"], out["n_seam_edges"] = _take(do, (n, 3)), _take(dp, (n, n, 4)), ne.value
    doff = _dev(offset)
    h, nt = C.c_int64(-7), C.c_int64(-7)
    head = (e.h, C.byref(x), n_v, vp(dV.data_ptr()), n_t, vp(dT.data_ptr()), vp(dlt.data_ptr()), vp(doff.data_ptr()))
    duv = _guarded(6 * n_t, torch.int32)
    e._check(e.L.mvs_engine_mesh_texture_levelled(*head, 0, None, vp(duv.data_ptr()), C.byref(h), C.byref(nt)))
    torch.cuda.synchronize()
    assert int((duv != -7).sum()) == 0, "the size call wrote uv"
    drgb = _guarded(h.value * width * 3, torch.uint8, 7)
    e._check(e.L.mvs_engine_mesh_texture_levelled(*head, h.value, vp(drgb.data_ptr()), vp(duv.data_ptr()), C.byref(h), C.byref(nt)))
    out["atlas"], out["uv"], out["n_textured"] = _take(drgb, (h.value, width, 3), 7), _take(duv, (n_t, 3, 2)), nt.value
    return out


def _same(name, *arrays):
    first = np.asarray(arrays[0])
    for other in arrays[1:]:
        other = np.asarray(other)
        assert first.shape == other.shape and first.dtype == other.dtype, f"{name}: {first.shape} {first.dtype} against {other.shape} {other.dtype}"
        assert first.tobytes() == other.tobytes(), f"{name}: {int((first != other).sum())} of {first.size} values differ"


def check(e, sc, verts, tris, visible=None, front_only=True, keep=192, iterations=64, max_shift=32, samples=4, label=None, res=2, width=256):
    """the five calls on one mesh, Python and device tensors against the reading -> dict of the Python results and the reading's inputs.
    label: forced labels in front of the smoothing (default: mesh_face_views' own).  The levels and the atlas take the smoothed labels"""
    verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    tris = np.ascontiguousarray(tris, dtype=np.int32).reshape(-1, 3)
    n, level = e.cfg.nviews, e.cfg.level
    sizes = [(w, h) for h, w in (e.level_shape(v) for v in range(n))]
    screen, vdepth = e.mesh_screen(verts, tris)
    screens, vdepths = list(screen), list(vdepth)
    images = [e.pyramid(v, level) for v in range(n)]
    signs = [tr.front_sign(rr.camera64(sc.P[v], level)) for v in range(n)]
    label_in = e.mesh_face_views(verts, tris, visible=visible, front_only=front_only)[0] if label is None else np.ascontiguousarray(label, dtype=np.int32)
    got = {}
    got["nbr"], got["n_irregular"] = e.mesh_adjacency(verts.shape[0], tris)
    got["quality"] = e.mesh_face_quality(verts, tris, visible=visible, front_only=front_only)
    got["label"], got["stats"] = e.smooth_face_views(tris, got["quality"], label_in, keep=keep, iterations=iterations)
    got["offset"], got["pairs"], got["n_seam_edges"] = e.seam_levels(verts, tris, got["label"], max_shift=max_shift, samples=samples)
    got["atlas"], got["uv"], got["n_textured"] = e.texture_mesh_levelled(verts, tris, got["label"], got["offset"], res=res, width=width)
    want = {}
    want["nbr"], want["n_irregular"] = sr.adjacency(verts.shape[0], tris)
    want["quality"] = sr.face_quality(screens, vdepths, tris, sizes, signs, visible=visible, front_only=front_only)
    if tris.shape[0] and (want["quality"].max(axis=1) > 0).any():
        rows = want["quality"].max(axis=1) > 0
        assert (want["quality"][rows].max(axis=1) == 255).all()  # the labelling's winner has 255
    want["label"], want["stats"] = sr.smooth_labels(verts.shape[0] if tris.size else 0, tris, want["quality"], label_in, keep, iterations)
    want["offset"], want["pairs"], want["n_seam_edges"] = sr.seam_levels(screens, vdepths, tris, want["label"], images, max_shift, samples)
    r = sr.texture_levelled(screens, vdepths, tris, want["label"], images, want["offset"], res, width)
    want["atlas"], want["uv"], want["n_textured"] = r["atlas"], r["uv"], r["n_textured"]
    dev = _device_calls(e, verts, tris, visible, front_only, engine.MeshSeams(keep, iterations, max_shift, samples), label_in, got["label"], got["offset"], res, width)
    for name in ("nbr", "quality", "label", "stats", "pairs", "offset", "uv", "atlas"):
        _same(name + " (two calls)", got[name], dev[name])
        _same(name + " (the reading)", got[name], want[name])
    for name in ("n_irregular", "n_seam_edges", "n_textured"):
        assert got[name] == dev[name] == want[name], f"{name}: {got[name]}, {dev[name]} against {want[name]}"
    return dict(got, label_in=label_in, reading=r, screens=screens, vdepths=vdepths, images=images)


def test_small_grid_every_call(plane):
    e, sc = plane
    verts, tris = small_grid()
    assert tris.shape[0] == 2262
    r = check(e, sc, verts, tris)
    print("small grid: stats", r["stats"].tolist(), "seam edges", r["n_seam_edges"], "offsets", r["offset"].tolist())
    assert r["n_irregular"] == 0 and (r["label"] >= 0).all() and r["stats"][1] <= r["stats"][0]
    # labels drawn at random: the smoothing has work, the levels have samples
    forced = noisy(tris.shape[0], 3)
    for keep in (128, 240):
        f = check(e, sc, verts, tris, keep=keep, label=forced)
        print(f"forced labels, keep {keep}: stats", f["stats"].tolist(), "seam edges", f["n_seam_edges"], "offsets", f["offset"].tolist())
        assert f["stats"][1] <= f["stats"][0] and (keep == 240 or f["stats"][2] > 0)
    # the smoothing off: the levels of the forced labels themselves
    f = check(e, sc, verts, tris, iterations=0, label=forced)
    assert (f["label"] == forced).all() and f["stats"][0] == f["stats"][1] > 0 and f["stats"][2] == 0 and f["n_seam_edges"] == f["stats"][1]
    assert f["pairs"][0, 1, 0] > 0 and (f["pairs"][:, :, 0] == f["pairs"][:, :, 0].T).all() and (f["pairs"][:, :, 1:] == -f["pairs"][:, :, 1:].transpose(1, 0, 2)).all()
    one = check(e, sc, verts, tris, iterations=1, label=forced)
    assert one["stats"][3] == 1


def test_samples_and_max_shift(plane):
    e, sc = plane
    verts, tris = small_grid()
    forced = noisy(tris.shape[0], 3)
    a = check(e, sc, verts, tris, iterations=0, samples=1, label=forced)
    b = check(e, sc, verts, tris, iterations=0, samples=16, label=forced, res=1, width=64)
    assert a["pairs"][:, :, 0].sum() == 2 * 2 * a["n_seam_edges"] and b["pairs"][:, :, 0].sum() == 2 * 17 * b["n_seam_edges"]
    z = check(e, sc, verts, tris, iterations=0, max_shift=0, label=forced)
    plain = e.texture_mesh(verts, tris, forced, res=2, width=256)
    assert (z["offset"] == 0).all() and z["atlas"].tobytes() == plain[0].tobytes() and z["uv"].tobytes() == plain[1].tobytes()
    assert e.texture_mesh_levelled(verts, tris, forced, None, res=2, width=256)[0].tobytes() == plain[0].tobytes()


def test_sphere_with_and_without_visibility(plane):
    e, sc = plane
    verts, tris = sphere()
    r = check(e, sc, verts, tris, res=2, width=512)
    g = check(e, sc, verts, tris, visible=e.mesh_visibility(verts, tris), res=2, width=512)
    print("sphere:", tris.shape[0], "triangles; stats", r["stats"].tolist(), "and", g["stats"].tolist(), "with the visibility")
    assert r["n_irregular"] == 0 and (r["nbr"] >= 0).all()
    assert ((g["quality"] > 0) <= (r["quality"] > 0)).all() and ((r["label"] == -1) == (r["label_in"] == -1)).all()


def test_coarse_grid_forced_labels(plane):
    e, sc = plane
    verts, tris = coarse_grid()
    r = check(e, sc, verts, tris, res=8)
    assert (r["quality"] == 0).all() and (r["label"] == -1).all() and r["n_seam_edges"] == 0 and (r["offset"] == 0).all()
    # quality 0 everywhere: nothing is admissible, the forced labels stay, and their seams are sampled at clamped positions
    r = check(e, sc, verts, tris, res=8, label=np.int32([0, 1, 2, 0, 1, 2, 0, 1]))
    assert (r["label"] == r["label_in"]).all() and r["n_seam_edges"] > 0 and r["pairs"][:, :, 0].sum() > 0


def test_shuffled_triangles(plane):
    e, sc = plane
    verts, tris = small_grid()
    forced = noisy(tris.shape[0], 3)
    perm = np.random.RandomState(11).permutation(tris.shape[0])
    inv = np.argsort(perm)
    a, b = check(e, sc, verts, tris, keep=128, label=forced), check(e, sc, verts, tris[perm], keep=128, label=forced[perm])
    assert (b["nbr"] == np.where(a["nbr"][perm] >= 0, inv[np.maximum(a["nbr"][perm], 0)], -1)).all()
    assert (b["quality"] == a["quality"][perm]).all() and (b["label"] == a["label"][perm]).all()
    for name in ("stats", "pairs", "offset"):
        assert (a[name] == b[name]).all(), name
    assert a["n_seam_edges"] == b["n_seam_edges"]


def test_all_labels_minus_one_and_empty_inputs(plane):
    e, sc = plane
    verts, tris = small_grid()
    r = check(e, sc, verts, tris, res=8, label=np.full(tris.shape[0], -1, np.int32))
    assert (r["label"] == -1).all() and r["stats"].tolist() == [0, 0, 0, 0] and r["n_seam_edges"] == 0 and (r["pairs"] == 0).all() and (r["atlas"] == 128).all()
    for v_, t_ in ((verts, np.zeros((0, 3), np.int32)), (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))):
        r = check(e, sc, v_, t_, res=8)
        assert r["nbr"].shape == (0, 3) and r["quality"].shape == (0, 3) and r["label"].shape == (0,) and r["stats"].tolist() == [0, 0, 0, 0]
        assert (r["offset"] == 0).all() and r["atlas"].shape == (11, 256, 3) and (r["atlas"] == 128).all()


def test_irregular_edges_and_degenerate_triangles(plane):
    e, sc = plane
    verts, tris = small_grid()
    tris = np.concatenate([tris[:200], tris[10:12], [[tris[20, 0], tris[20, 1], tris[20, 1]]], [[tris[30, 1], tris[30, 0], tris[30, 2]]]]).astype(np.int32)
    r = check(e, sc, verts, tris, keep=128, label=noisy(tris.shape[0], 3))
    assert r["n_irregular"] > 0 and (r["nbr"][[10, 11, 200, 201, 202]] == -1).all()


def test_level_one(plane):
    _, sc = plane
    e = _engine(sc, level=1)
    verts, tris = small_grid()
    r = check(e, sc, verts, tris, keep=128, label=noisy(tris.shape[0], 3))
    assert e.level_shape(0) == (32, 48) and r["n_seam_edges"] > 0
    e.close()


def test_unequal_view_sizes(plane):
    _, sc = plane
    e = _engine(sc, sizes=[(96, 64), (80, 50), (61, 64)])
    verts, tris = small_grid()
    r = check(e, sc, verts * np.float32(3.0), tris)
    print("unequal views: stats", r["stats"].tolist(), "seam edges", r["n_seam_edges"])
    assert ((r["quality"] > 0).sum(axis=0) > 0).sum() >= 2
    cv, ct = coarse_grid()
    check(e, sc, cv, ct, res=8, label=np.int32([0, 1, 2, 0, 1, 2, 0, 1]))
    e.close()


@pytest.mark.parametrize("family", ["roll", "mixed"])
def test_camera_families(family):
    sc = cs.reading_scene(family)
    e = _engine(sc)
    T = np.float32(sc.meta["target"])
    verts, tris = small_grid()
    r = check(e, sc, verts + T, tris, keep=128)
    print(family, "stats", r["stats"].tolist(), "seam edges", r["n_seam_edges"], "offsets", r["offset"].tolist())
    f = check(e, sc, verts + T, tris, iterations=0, label=noisy(tris.shape[0], sc.nviews))
    assert f["n_seam_edges"] > 0
    e.close()


def test_bad_id_and_bad_label_write_nothing(plane):
    e, sc = plane
    verts, tris = small_grid()
    n_t = tris.shape[0]
    good = e.mesh_face_views(verts, tris)[0]
    x, s = engine.MeshTexturing(8, 256, 1, 0), engine.MeshSeams(192, 64, 32, 4)
    nbr, quality, out = np.full((n_t, 3), -7, np.int32), np.full((n_t, 3), 7, np.uint8), np.full(n_t, -7, np.int32)
    stats, offset, pairs = np.full(4, -7, np.int64), np.full((3, 3), -7, np.int32), np.full((3, 3, 4), -7, np.int64)
    rgb, uv = np.full((4096, 256, 3), 7, np.uint8), np.full((n_t, 3, 2), -7, np.int32)
    ni, ne, h, n = C.c_int64(-7), C.c_int64(-7), C.c_int64(-7), C.c_int64(-7)
    p = {k: a.ctypes.data_as(vp) for k, a in dict(verts=verts, good=good, nbr=nbr, quality=quality, out=out, stats=stats, offset=offset, pairs=pairs, rgb=rgb,
                                                  uv=uv).items()}
    zeros = np.zeros((3, 3), np.int32)
    for bad in (-1, verts.shape[0], 1 << 30):
        t = tris.copy()
        t[n_t // 2, 1] = bad
        tp = t.ctypes.data_as(vp)
        assert e.L.mvs_engine_mesh_adjacency(e.h, verts.shape[0], n_t, tp, p["nbr"], C.byref(ni)) == MVS_ERR_ARG and b"index outside" in e.L.mvs_last_error()
        assert e.L.mvs_engine_mesh_face_quality(e.h, C.byref(x), verts.shape[0], p["verts"], n_t, tp, None, p["quality"]) == MVS_ERR_ARG
        assert b"index outside" in e.L.mvs_last_error()
        assert e.L.mvs_engine_mesh_smooth_labels(e.h, C.byref(s), verts.shape[0], n_t, tp, 3, p["quality"], p["good"], p["out"], p["stats"]) == MVS_ERR_ARG
        assert b"index outside" in e.L.mvs_last_error()
        assert e.L.mvs_engine_mesh_seam_levels(e.h, C.byref(s), C.byref(x), verts.shape[0], p["verts"], n_t, tp, p["good"], p["offset"], p["pairs"],
                                               C.byref(ne)) == MVS_ERR_ARG and b"index outside" in e.L.mvs_last_error()
        assert e.L.mvs_engine_mesh_texture_levelled(e.h, C.byref(x), verts.shape[0], p["verts"], n_t, tp, p["good"], zeros.ctypes.data_as(vp), 4096, p["rgb"],
                                                    p["uv"], C.byref(h), C.byref(n)) == MVS_ERR_ARG and b"index outside" in e.L.mvs_last_error()
    tp = tris.ctypes.data_as(vp)
    for bad in (-2, 3, 1 << 20):
        lab = good.copy()
        lab[17] = bad
        lp = lab.ctypes.data_as(vp)
        assert e.L.mvs_engine_mesh_smooth_labels(e.h, C.byref(s), verts.shape[0], n_t, tp, 3, p["quality"], lp, p["out"], p["stats"]) == MVS_ERR_ARG
        assert b"label outside" in e.L.mvs_last_error()
        assert e.L.mvs_engine_mesh_seam_levels(e.h, C.byref(s), C.byref(x), verts.shape[0], p["verts"], n_t, tp, lp, p["offset"], p["pairs"],
                                               C.byref(ne)) == MVS_ERR_ARG and b"label outside" in e.L.mvs_last_error()
        assert e.L.mvs_engine_mesh_texture_levelled(e.h, C.byref(x), verts.shape[0], p["verts"], n_t, tp, lp, zeros.ctypes.data_as(vp), 4096, p["rgb"], p["uv"],
                                                    C.byref(h), C.byref(n)) == MVS_ERR_ARG and b"label outside" in e.L.mvs_last_error()
    for a in (nbr, out, stats, offset, pairs, uv):
        assert (a == -7).all()
    assert (quality == 7).all() and (rgb == 7).all() and (ni.value, ne.value, h.value, n.value) == (-7, -7, -7, -7)


def test_state_errors_for_the_calls_that_need_views():
    e = engine.Engine(3)
    verts, tris = coarse_grid()
    label = np.zeros(tris.shape[0], np.int32)
    for call in (lambda: e.mesh_face_quality(verts, tris), lambda: e.seam_levels(verts, tris, label),
                 lambda: e.texture_mesh_levelled(verts, tris, label, np.zeros((3, 3), np.int32))):
        with pytest.raises(engine.EngineError) as err:
            call()
        assert err.value.status == MVS_ERR_STATE and "views not set" in str(err.value)
    # the graph calls need none
    nbr, nirr = e.mesh_adjacency(verts.shape[0], tris)
    assert nbr.tobytes() == sr.adjacency(verts.shape[0], tris)[0].tobytes() and nirr == 0
    quality = np.full((tris.shape[0], 2), 255, np.uint8)
    lab = np.int32([0, 0, 1, 0, 0, 0, 0, 0])
    out, stats = e.smooth_face_views(tris, quality, lab)
    want = sr.smooth_labels(verts.shape[0], tris, quality, lab)
    assert out.tobytes() == want[0].tobytes() and stats.tobytes() == want[1].tobytes() and stats[1] == 0
    e.close()


def test_the_chain():
    sc = cached_scene(3, 96, 64, 30.0)
    sizes = [(sc.W, sc.H)] * sc.nviews
    seeds = synth.make_seeds(sc, PLAIN["level"], PLAIN["csize"], stride=1)
    e = engine_with_pool(sc, PLAIN, None, sizes, None, seeds)
    alive, thr = e.patches(), e.thresholds()
    vol = lattice(sc, PLAIN["level"])
    chain = dict(largest_only=True, fill_max_edges=16, smooth_iterations=2, decimate_cell=2.0 * float(vol.voxel), min_consistent=1, depth_tol=DEPTH_TOL,
                 normal_cos=NORMAL_COS, res=8, atlas_width=512)
    before = e.textured_mesh(vol, **chain)
    verts, tris, normals, atlas, uv, label = e.textured_mesh(vol, seam_keep=192, level_colours=True, **chain)
    assert [a.tobytes() for a in (verts, tris, normals)] == [a.tobytes() for a in before[:3]]
    # the calls by hand
    visible = e.mesh_visibility(verts, tris, 0.01)
    l0 = e.mesh_face_views(verts, tris, visible=visible, front_only=True)[0]
    assert l0.tobytes() == before[5].tobytes() and before[3].tobytes() == e.texture_mesh(verts, tris, l0, res=8, width=512)[0].tobytes()
    quality = e.mesh_face_quality(verts, tris, visible=visible, front_only=True)
    l1, stats = e.smooth_face_views(tris, quality, l0, keep=192)
    offset, pairs, n_edges = e.seam_levels(verts, tris, l1)
    hand = e.texture_mesh_levelled(verts, tris, l1, offset, res=8, width=512)
    print(f"chain: {tris.shape[0]} triangles, stats {stats.tolist()}, {n_edges} seam edges, offsets {offset.tolist()}")
    assert [a.tobytes() for a in (label, atlas, uv)] == [a.tobytes() for a in (l1, hand[0], hand[1])]
    assert ((quality[np.arange(tris.shape[0]), np.maximum(l0, 0)] == 255) | (l0 < 0)).all()
    # each switch alone reaches its call; the defaults return the present bytes
    only_smooth = e.textured_mesh(vol, seam_keep=192, **chain)
    assert only_smooth[5].tobytes() == l1.tobytes() and only_smooth[3].tobytes() == e.texture_mesh(verts, tris, l1, res=8, width=512)[0].tobytes()
    assert [a.tobytes() for a in e.textured_mesh(vol, **chain)] == [a.tobytes() for a in before]
    assert [a.tobytes() for a in e.textured_mesh(vol, seam_keep=0, level_colours=False, **chain)] == [a.tobytes() for a in before]
    # nothing of the engine's state moved
    assert e.patches().tobytes() == alive.tobytes() and e.thresholds() == thr
    t = engine_with_pool(sc, PLAIN, None, sizes, None, seeds)
    assert e.propagate(1) == t.propagate(1)
    assert e.patches().tobytes() == t.patches().tobytes()
    t.close()
    e.close()
