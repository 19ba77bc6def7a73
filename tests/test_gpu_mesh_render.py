"""mvs_engine_mesh_render and mvs_engine_mesh_visibility on the GPU against tests/mesh_render_reading.py.  The device's own screen and
vdepth go into the reading, which leaves integer coverage and an IEEE fp64 chain between the two: depth, tri, n_covered, n_skipped and
visible are compared byte for byte, with no margins and nothing left out.  The projection itself is held to the float64 one within
maps_reading.margins.  Engines have views only (no pool); 3 views of 96 x 64 around the plane z = 0 unless a case says otherwise."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import camera_scenes as cs
import mesh_reading as mr
import mesh_render_reading as rr
from maps_reading import margins
from mvskit_amd import engine
from mvskit_amd.engine import MVS_ERR_ARG
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


def _render_device(e, verts, tris, shapes):
    """one call with every output and both inputs in device memory -> (maps, screen, vdepth, covered, skipped) as numpy"""
    n, n_v = e.cfg.nviews, verts.shape[0]
    dV, dT = _dev(verts.reshape(-1)), _dev(tris.reshape(-1))
    dd = [torch.full((h * w,), -7.0, dtype=torch.float32, device="cuda") for h, w in shapes]
    dt = [torch.full((h * w,), -7, dtype=torch.int32, device="cuda") for h, w in shapes]
    ds = torch.full((n * n_v * 2 + 1,), -7, dtype=torch.int32, device="cuda")
    dz = torch.full((n * n_v + 1,), -7.0, dtype=torch.float32, device="cuda")
    dc, dk = torch.full((n,), -7, dtype=torch.int64, device="cuda"), torch.full((n,), -7, dtype=torch.int64, device="cuda")
    slots = (engine.MeshViewRender * n)()
    for v in range(n):
        slots[v].depth, slots[v].tri = dd[v].data_ptr(), dt[v].data_ptr()
    e._check(e.L.mvs_engine_mesh_render(e.h, n_v, vp(dV.data_ptr()), tris.shape[0], vp(dT.data_ptr()), slots, vp(ds.data_ptr()), vp(dz.data_ptr()),
                                        vp(dc.data_ptr()), vp(dk.data_ptr())))
    torch.cuda.synchronize()
    assert int(ds[-1]) == -7 and float(dz[-1]) == -7.0, "a write behind screen or vdepth"
    maps = [(dd[v].cpu().numpy().reshape(shapes[v]), dt[v].cpu().numpy().reshape(shapes[v])) for v in range(n)]
    return maps, ds[:-1].cpu().numpy().reshape(n, n_v, 2), dz[:-1].cpu().numpy().reshape(n, n_v), dc.cpu().numpy(), dk.cpu().numpy()


def _visibility_device(e, verts, tris, tol):
    dV, dT = _dev(verts.reshape(-1)), _dev(tris.reshape(-1))
    out = torch.full((verts.shape[0] + 1,), 7, dtype=torch.int64, device="cuda")
    e._check(e.L.mvs_engine_mesh_visibility(e.h, C.c_float(tol), verts.shape[0], vp(dV.data_ptr()), tris.shape[0], vp(dT.data_ptr()), vp(out.data_ptr())))
    torch.cuda.synchronize()
    assert int(out[-1]) == 7
    return out[:-1].cpu().numpy().view(np.uint64)


def check(e, sc, verts, tris, tol=0.01, kappa=1.0, sizes=None):
    """every check of the module's docstring on one mesh -> dict(maps, screen, vdepth, covered, skipped, visible, listed, reading)"""
    verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    tris = np.ascontiguousarray(tris, dtype=np.int32).reshape(-1, 3)
    n, level = e.cfg.nviews, e.cfg.level
    shapes = [e.level_shape(v) for v in range(n)]
    # host outputs through the Python surface, device tensors through the C ABI: two calls, the same bytes
    maps, covered, skipped = e.render_mesh(verts, tris)
    screen, vdepth = e.mesh_screen(verts, tris)
    dmaps, dscreen, dvdepth, dcovered, dskipped = _render_device(e, verts, tris, shapes)
    assert screen.tobytes() == dscreen.tobytes() and vdepth.tobytes() == dvdepth.tobytes(), "two calls give different vertices"
    assert covered.tobytes() == dcovered.tobytes() and skipped.tobytes() == dskipped.tobytes(), "two calls give different counts"
    for v in range(n):
        assert maps[v][0].shape == shapes[v] and maps[v][0].tobytes() == dmaps[v][0].tobytes(), f"view {v}: two calls give different depth bytes"
        assert maps[v][1].tobytes() == dmaps[v][1].tobytes(), f"view {v}: two calls give different triangle rows"
    # the projection against float64
    for v in range(n):
        H, W = shapes[v]
        s64, d64, xy, mag = rr.project64(rr.camera64(sc.P[v], level), verts)
        fin = np.isfinite(verts).all(axis=1)
        assert (np.abs(vdepth[v][fin].astype(np.float64) - d64[fin]) <= 4 * rr.U * mag[fin]).all(), f"view {v}: vdepth"
        # maps_reading.margins(kappa, W, H)["edge"] for every vertex in front of the camera that the snapping can hold (|sx|, |sy| within
        # int32).  Its derivation supposes |X|_inf <= kappa depth and a position within max(W, H) of the origin: the numerator's share
        # grows with |X|_inf / depth and the denominator's, which is relative, with the position.  A vertex outside those (the corners
        # of the coarse grids, the whole-image triangle, a vertex next to the camera plane) gets its own ratio for kappa and the margin
        # times |position| / max(W, H); for every vertex inside them this is margins(kappa, W, H)["edge"] itself
        with np.errstate(invalid="ignore", divide="ignore"):
            held = fin & (d64 > 0) & (np.abs(xy).max(axis=1) < 2.0 ** 22)
            ratio = np.maximum(kappa, np.abs(verts).max(axis=1).astype(np.float64)[held] / d64[held])
        reach = np.maximum(1.0, np.abs(xy[held]).max(axis=1) / max(W, H))
        edge = np.array([margins(float(k), W, H)["edge"] for k in ratio]) * reach
        inside = (ratio == kappa) & (reach == 1.0)
        assert (edge[inside] == margins(kappa, W, H)["edge"]).all()
        err = np.abs(screen[v][held].astype(np.float64) / 256.0 - xy[held]).max(axis=1)
        assert (err <= edge + 0.5 / 256).all(), f"view {v}: screen off by {(err - edge).max()} pixels more than the margin"
    # the reading on the device's own vertices: bytes
    reading, listed = [], []
    for v in range(n):
        H, W = shapes[v]
        m = rr.render(screen[v], vdepth[v], tris, W, H)
        reading.append(m)
        listed.append(rr.listed(screen[v], vdepth[v], tris, W, H))
        assert maps[v][1].tobytes() == m["tri"].tobytes(), f"view {v}: {int((maps[v][1] != m['tri']).sum())} triangle rows differ from the reading"
        assert maps[v][0].tobytes() == m["depth"].tobytes(), f"view {v}: depth bytes differ from the reading"
        assert covered[v] == m["covered"] and skipped[v] == m["skipped"], f"view {v}: {covered[v]}, {skipped[v]} against {m['covered']}, {m['skipped']}"
    # which of the two rasterising kernels took each triangle: the device's own count of its list
    assert e.mesh_render_lists(verts, tris).tolist() == listed, "the device listed other triangles for the wave-per-triangle kernel than the reading"
    visible = e.mesh_visibility(verts, tris, tol)
    assert visible.tobytes() == _visibility_device(e, verts, tris, tol).tobytes(), "two calls give different visibility"
    want = rr.visibility(screen, vdepth, [m["depth"] for m in reading], tol) if verts.shape[0] else np.zeros(0, np.uint64)
    assert visible.tobytes() == want.tobytes(), f"{int((visible != want).sum())} visibility words differ from the reading"
    assert not (visible >> np.uint64(n)).any()
    return dict(maps=maps, screen=screen, vdepth=vdepth, covered=covered, skipped=skipped, visible=visible, listed=listed, reading=reading)


def fine_grid(z=0.0, wobble=0.03):
    """200 x 140 vertices a third of a pixel apart around the target, on a gently waved surface"""
    verts, tris = grid_mesh(200, 140)
    verts = (verts - np.float32([99.5, 69.5, 0.0])) * np.float32(0.34 * FOOT)
    verts[:, 2] = z + wobble * np.sin(7.0 * verts[:, 0]) * np.cos(5.0 * verts[:, 1])
    return verts.astype(np.float32), tris


def coarse_grid(z=0.0):
    """3 x 3 vertices, ten times the image's footprint across"""
    verts, tris = grid_mesh(3, 3)
    verts = (verts - np.float32([1.0, 1.0, 0.0])) * np.float32([5.0 * 96 * FOOT, 5.0 * 64 * FOOT, 1.0])
    verts[:, 2] = z
    return verts.astype(np.float32), tris


def unproject(sc, v, uvd):
    """world points of (u, v, depth) in view v at level 0, float64"""
    P = sc.P[v].astype(np.float64)
    uvd = np.asarray(uvd, dtype=np.float64)
    rhs = np.stack([uvd[:, 0] * uvd[:, 2], uvd[:, 1] * uvd[:, 2], uvd[:, 2]], axis=1) - P[:, 3]
    return np.linalg.solve(P[:, :3], rhs.T).T


def test_fine_grid_runs_the_small_path(plane):
    e, sc = plane
    r = check(e, sc, *fine_grid())
    print("fine grid: covered", r["covered"].tolist(), "listed", r["listed"])
    assert r["listed"] == [0, 0, 0] and (r["skipped"] == 0).all() and (r["covered"] > 2000).all()
    assert max(int(m["count"].max()) for m in r["reading"]) == 1  # a height field seen from above: watertight, no double cover


def test_coarse_grid_runs_the_large_path(plane):
    e, sc = plane
    r = check(e, sc, *coarse_grid())
    print("coarse grid: covered", r["covered"].tolist(), "listed", r["listed"], "skipped", r["skipped"].tolist())
    assert min(r["listed"]) >= 2 and r["skipped"][1] == 0 and r["covered"][1] == 96 * 64  # clipped on all four borders


def test_both_grids_in_one_call(plane):
    e, sc = plane
    fv, ft = fine_grid(z=0.1)
    cv, ct = coarse_grid()
    r = check(e, sc, np.concatenate([cv, fv]), np.concatenate([ct, ft + cv.shape[0]]))
    assert min(r["listed"]) >= 2 and r["covered"][1] == 96 * 64
    front = r["maps"][1][1] >= ct.shape[0]
    assert 2000 < int(front.sum()) < 96 * 64  # the fine grid in front of the coarse one, which shows around it


def test_one_triangle_over_the_whole_image(plane):
    e, sc = plane
    verts = unproject(sc, 1, [[-1000.0, -700.0, 4.0], [1100.0, -700.0, 4.2], [48.0, 1500.0, 3.9]]).astype(np.float32)
    r = check(e, sc, verts, np.int32([[0, 1, 2]]))
    assert r["listed"][1] == 1 and r["covered"][1] == 96 * 64 and (r["maps"][1][1] == 0).all()
    r = check(e, sc, verts, np.int32([[0, 2, 1]]))  # the other face
    assert r["covered"][1] == 96 * 64


def test_sliver(plane):
    e, sc = plane
    # one sub-pixel unit wide along a pixel row of view 1, its long edges on the pixel centres' line and just below it
    verts = unproject(sc, 1, [[-10.0, 31.0, 4.0], [110.0, 31.0, 4.0], [110.0, 31.0 + 1.0 / 256, 4.0], [-10.0, 31.0 + 1.0 / 256, 4.0]]).astype(np.float32)
    r = check(e, sc, verts, np.int32([[0, 1, 2], [0, 2, 3]]))
    print("sliver: covered", r["covered"].tolist(), "screen of view 1", r["screen"][1].tolist())
    assert r["covered"][1] <= 96


def test_sphere_front_layer_wins(plane):
    e, sc = plane
    dims = (24, 20, 20)
    centre = np.float32([8.3, 9.6, 10.2])
    verts, tris = e.extract_mesh(engine.make_volume((0.0, 0.0, 0.0), 1.0, dims, 1.0), mr.sphere_volume(dims, [tuple(centre)], 6.2))
    print("sphere:", verts.shape[0], "vertices,", tris.shape[0], "triangles")
    assert verts.shape[0] > 2000 and mr.closed_and_oriented(tris)
    verts = ((verts - centre) * np.float32(0.5 / 6.2)).astype(np.float32)
    r = check(e, sc, verts, tris)
    for v in range(sc.nviews):
        P = rr.camera64(sc.P[v], 0)
        depth = verts.astype(np.float64) @ P[2, :3] + P[2, 3]
        mid = P[2, 3]  # the depth of the sphere's centre, the origin
        seen = r["maps"][v][0]
        assert (seen[np.isfinite(seen)] < mid).all(), f"view {v}: the back hemisphere won a pixel"
        assert int(r["reading"][v]["count"].max()) >= 2  # two layers at least
        # away from the limb: there a vertex's nearest pixel centre may lie off the sphere, or on a slope of more than the tolerance
        back, front = depth > mid + 0.25, depth < mid - 0.3
        bit = (r["visible"] >> np.uint64(v)) & np.uint64(1)
        print(f"view {v}: visible {int(bit[front].sum())} of {int(front.sum())} front and {int(bit[back].sum())} of {int(back.sum())} back vertices")
        assert bit[back].sum() == 0 and bit[front].sum() > 0.9 * front.sum()


def two_layers():
    av, at = fine_grid(z=0.0, wobble=0.0)
    bv, bt = fine_grid(z=0.2, wobble=0.0)
    tris = np.empty((2 * at.shape[0], 3), np.int32)
    tris[0::2], tris[1::2] = at, bt + av.shape[0]  # interleaved rows
    return np.concatenate([av, bv]), tris, av.shape[0]


def test_two_layers_and_the_tolerance(plane):
    e, sc = plane
    verts, tris, n0 = two_layers()
    r = check(e, sc, verts, tris)
    for v in range(sc.nviews):
        both = r["reading"][v]["count"] >= 2  # seen at an angle, the layer behind shows along two borders
        assert both.sum() > 2000 and (r["maps"][v][1][both] % 2 == 1).all(), f"view {v}: the layer behind won a pixel"
    bit1 = (r["visible"] >> np.uint64(1)) & np.uint64(1)
    inner = np.abs(verts[:n0, :2]).max(axis=1) < 0.3  # under the middle of the front layer
    assert bit1[:n0][inner].sum() == 0 and bit1[n0:].sum() > 0.9 * n0
    # tol = 0: the front layer's own vertices pass only where the interpolated depth at the nearest centre is not nearer; 0.05 = 0.2 / 4
    # and a little lets nothing of the back layer through, 0.06 does
    r0 = check(e, sc, verts, tris, tol=0.0)
    r5 = check(e, sc, verts, tris, tol=0.05)
    assert ((r0["visible"] & ~r["visible"]) == 0).all() and ((r["visible"] & ~r5["visible"]) == 0).all()
    assert (r0["visible"] != r["visible"]).any()
    r6 = check(e, sc, verts, tris, tol=0.06)
    assert ((r6["visible"][:n0][inner] >> np.uint64(1)) & np.uint64(1)).sum() > 0


def test_coincident_grids_and_shuffled_triangles(plane):
    e, sc = plane
    verts, tris = fine_grid()
    once = check(e, sc, verts, tris)
    perm = np.random.RandomState(11).permutation(tris.shape[0])
    twice = check(e, sc, np.concatenate([verts, verts]), np.concatenate([tris, tris[perm] + verts.shape[0]]))
    shuffled = check(e, sc, verts, tris[perm])
    for v in range(sc.nviews):
        assert twice["maps"][v][0].tobytes() == once["maps"][v][0].tobytes() == shuffled["maps"][v][0].tobytes()
        assert twice["maps"][v][1].tobytes() == once["maps"][v][1].tobytes()  # the smaller row
        have = once["maps"][v][1] >= 0
        assert (perm[shuffled["maps"][v][1][have]] == once["maps"][v][1][have]).all()
    assert shuffled["visible"].tobytes() == once["visible"].tobytes()


def test_skipped_and_zero_area_triangles():
    # cameras whose third row is (0, 0, 1, 0): the depth of a vertex is its z, exactly
    f, W, H = 100.0, 96, 64
    K = np.array([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1.0]])
    P = np.stack([K @ np.concatenate([np.eye(3), np.array([[t], [0.0], [0.0]])], axis=1) for t in (0.0, -0.3)]).astype(np.float32)
    rng = np.random.RandomState(3)
    sc = types.SimpleNamespace(nviews=2, W=W, H=H, P=P, images=rng.randint(0, 255, (2, H, W, 3)).astype(np.uint8))
    e = _engine(sc)
    good = np.float32([[-0.3, -0.2, 1.0], [0.3, -0.2, 1.0], [0.0, 0.25, 1.2], [0.1, 0.1, 0.9]])
    bad = np.float32([[0, 0, -1.0], [0.1, 0.1, 0.0], [np.nan, 0, 1], [0, np.inf, 1], [0, 0, -np.inf], [1e5, 0, 0.1], [0, 0, np.inf]])
    near = np.float32([[0.0, 0.0, 1.0], [1e-6, 0.0, 1.0], [0.0, 1e-6, 1.0]])  # one snapped point
    line = np.float32([[-0.2, 0.1, 1.0], [0.0, 0.1, 1.0], [0.2, 0.1, 1.0]])   # a row of pixels' line: collinear after snapping
    verts = np.concatenate([good, bad, near, line])
    nb, nn, nl = 4, 4 + len(bad), 4 + len(bad) + 3
    tris = [[0, 1, 2], [0, 1, 3]] + [[0, 1, nb + k] for k in range(len(bad))] + [[0, 0, 1], [2, 2, 2], [nn, nn + 1, nn + 2], [nl, nl + 1, nl + 2], [1, 2, 3]]
    tris = np.int32(tris)
    r = check(e, sc, verts, tris)
    assert (r["vdepth"][0][nb:nb + 2] == np.float32([-1.0, 0.0])).all()
    assert (r["skipped"] == len(bad)).all(), r["skipped"]
    keep = np.int32([0, 1, len(tris) - 1])
    alone = check(e, sc, verts, tris[keep])
    for v in range(2):
        assert alone["maps"][v][0].tobytes() == r["maps"][v][0].tobytes() and (alone["skipped"] == 0).all()
        have = r["maps"][v][1] >= 0
        assert have.sum() > 200 and (keep[alone["maps"][v][1][have]] == r["maps"][v][1][have]).all()
    e.close()


def test_empty_inputs(plane):
    e, sc = plane
    verts = fine_grid()[0][:700]
    for v_, t_ in ((verts, np.zeros((0, 3), np.int32)), (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))):
        r = check(e, sc, v_, t_)
        assert (r["covered"] == 0).all() and (r["skipped"] == 0).all()
        for d, t in r["maps"]:
            assert np.isnan(d).all() and (t == -1).all()
    # a vertex alone hides nothing: every one inside the image is visible
    assert (check(e, sc, verts, np.zeros((0, 3), np.int32))["visible"] == np.uint64(7)).all()


def test_odd_views():
    sc = cached_scene(3, 97, 61, 20.0)
    e = _engine(sc)
    cv, ct = coarse_grid()
    fv, ft = fine_grid(z=0.1)
    r = check(e, sc, np.concatenate([cv, fv]), np.concatenate([ct, ft + cv.shape[0]]))
    assert r["maps"][0][0].shape == (61, 97) and r["covered"][1] == 97 * 61
    e.close()


def test_unequal_view_sizes(plane):
    _, sc = plane
    sizes = [(96, 64), (80, 50), (61, 64)]
    e = _engine(sc, sizes=sizes)
    cv, ct = coarse_grid()
    fv, ft = fine_grid(z=0.1)
    r = check(e, sc, np.concatenate([cv, fv]), np.concatenate([ct, ft + cv.shape[0]]))
    assert [m[0].shape for m in r["maps"]] == [(64, 96), (50, 80), (64, 61)] and r["covered"][1] == 80 * 50
    e.close()


def test_level_one(plane):
    _, sc = plane
    e = _engine(sc, level=1)
    cv, ct = coarse_grid()
    fv, ft = fine_grid(z=0.1)
    r = check(e, sc, np.concatenate([cv, fv]), np.concatenate([ct, ft + cv.shape[0]]))
    assert r["maps"][0][0].shape == (32, 48) and r["covered"][1] == 48 * 32
    e.close()


def test_bad_id_writes_nothing(plane):
    e, sc = plane
    verts, tris = fine_grid()
    for bad in (-1, verts.shape[0], 1 << 30):
        t = tris.copy()
        t[tris.shape[0] // 2, 1] = bad
        depth, tri = np.full((64, 96), -7, np.float32), np.full((64, 96), -7, np.int32)
        screen, vdepth = np.full((3, verts.shape[0], 2), -7, np.int32), np.full((3, verts.shape[0]), -7, np.float32)
        cov, skip, vis = np.full(3, -7, np.int64), np.full(3, -7, np.int64), np.full(verts.shape[0], 7, np.uint64)
        slots = (engine.MeshViewRender * 3)()
        for s in slots:
            s.depth, s.tri = depth.ctypes.data, tri.ctypes.data
        p = [a.ctypes.data_as(vp) for a in (verts, t, screen, vdepth, cov, skip, vis)]
        assert e.L.mvs_engine_mesh_render(e.h, verts.shape[0], p[0], t.shape[0], p[1], slots, p[2], p[3], p[4], p[5]) == MVS_ERR_ARG
        assert b"index outside" in e.L.mvs_last_error()
        assert e.L.mvs_engine_mesh_visibility(e.h, C.c_float(0.01), verts.shape[0], p[0], t.shape[0], p[1], p[6]) == MVS_ERR_ARG
        assert e.L.mvs_engine_mesh_render_lists(e.h, verts.shape[0], p[0], t.shape[0], p[1], p[4]) == MVS_ERR_ARG
        for a in (depth, tri, screen, vdepth, cov, skip):
            assert (a == -7).all()
        assert (vis == 7).all()


def test_every_output_null_in_turn(plane):
    e, sc = plane
    cv, ct = coarse_grid()
    fv, ft = fine_grid(z=0.1)
    verts, tris = np.concatenate([cv, fv]), np.concatenate([ct, ft + cv.shape[0]])
    full = check(e, sc, verts, tris)
    n_v = verts.shape[0]
    for drop in ("out", "depth", "tri", "screen", "vdepth", "covered", "skipped"):
        depth, tri = [np.full((64, 96), -7, np.float32) for _ in range(3)], [np.full((64, 96), -7, np.int32) for _ in range(3)]
        screen, vdepth = np.full((3, n_v, 2), -7, np.int32), np.full((3, n_v), -7, np.float32)
        cov, skip = np.full(3, -7, np.int64), np.full(3, -7, np.int64)
        slots = (engine.MeshViewRender * 3)()
        for v in range(3):
            slots[v].depth = None if drop == "depth" else depth[v].ctypes.data
            slots[v].tri = None if drop == "tri" else tri[v].ctypes.data

        def arg(name, a):
            return None if drop == name else a.ctypes.data_as(vp)

        e._check(e.L.mvs_engine_mesh_render(e.h, n_v, verts.ctypes.data_as(vp), tris.shape[0], tris.ctypes.data_as(vp), None if drop == "out" else slots,
                                            arg("screen", screen), arg("vdepth", vdepth), arg("covered", cov), arg("skipped", skip)))
        for v in range(3):
            assert depth[v].tobytes() == (full["maps"][v][0].tobytes() if drop not in ("out", "depth") else np.full((64, 96), -7, np.float32).tobytes()), drop
            assert tri[v].tobytes() == (full["maps"][v][1].tobytes() if drop not in ("out", "tri") else np.full((64, 96), -7, np.int32).tobytes()), drop
        assert (screen == -7).all() if drop == "screen" else screen.tobytes() == full["screen"].tobytes(), drop
        assert (vdepth == -7).all() if drop == "vdepth" else vdepth.tobytes() == full["vdepth"].tobytes(), drop
        assert (cov == -7).all() if drop == "covered" else (cov == full["covered"]).all(), drop
        assert (skip == -7).all() if drop == "skipped" else (skip == full["skipped"]).all(), drop


def test_state_errors():
    e = engine.Engine(3)
    verts, tris = coarse_grid()
    with pytest.raises(engine.EngineError) as err:
        e.mesh_screen(verts, tris)
    assert err.value.status == engine.MVS_ERR_STATE and "views not set" in str(err.value)
    with pytest.raises(engine.EngineError) as err:
        e.mesh_visibility(verts, tris)
    assert err.value.status == engine.MVS_ERR_STATE
    e.close()


@pytest.mark.parametrize("family", ["roll", "far", "mixed"])
def test_camera_families(family):
    sc = cs.reading_scene(family)
    e = _engine(sc)
    T = np.float32(sc.meta["target"])
    cv, ct = coarse_grid()
    fv, ft = fine_grid(z=0.1)
    verts, tris = np.concatenate([cv * np.float32([0.5, 0.5, 1.0]), fv]) + T, np.concatenate([ct, ft + cv.shape[0]])
    r = check(e, sc, verts, tris, kappa=cs.kappa(sc))
    print(family, "kappa", cs.kappa(sc), "covered", r["covered"].tolist(), "listed", r["listed"], "skipped", r["skipped"].tolist())
    assert min(r["listed"]) >= 1 and (r["covered"] > 2000).all()
    e.close()
