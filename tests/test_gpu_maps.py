"""Dense per-view maps and their fusion on the GPU: mvs_engine_render_maps / mvs_engine_fused_points against a float64 numpy reading.

The pool of every case: synth.make_seeds uploaded, then propagate(0) once -- the patches carry real m_ncc, lists and some noise.  The
yardstick (render64, agree64, fused64 of tests/maps_reading.py) works on e.patches() and float64 copies of the float32 cameras, read at level L as tests/test_gpu_seed_points.py
reads them (P[:2] /= 2**L, oaxis64, center64).  Every decision of the feature is integer-exact against code from before it (the ids of
mvs_engine_depth_normal_map) or lies outside a stated margin, so float64 never disagrees on one: a pair (pixel of v, view u) whose
projection lies within 1e-3 pixel of a rounding boundary (image edges are such boundaries), whose | |s - 1| - depth_tol | is below 1e-5 or
whose |n.n_q - normal_cos| is below 1e-5 is left out (the GPU may set or clear its bit), and a pixel with such a pair is left out of the
fused-point comparison.  Every case asserts that the reading leaves out fewer than 5 % of the valid pixels and finds at least 10 % of them
with no agreeing view and at least 10 % with all other views agreeing: a vacuous or one-sided case fails.

Depth bound: the reading is about 30 float32 operations at unit roundoff 2^-24 divided by the cosine between the normal and the ray, about
2e-6 / cos; the bound 2e-5 / |cos| relative keeps a tenfold margin.

Cameras off the arc (camera_scenes.py): where the world lies off the origin every one of those roundings is relative to the coordinates,
kappa(sc) times the depths, so the depth bound is 2e-5 kappa / |cos|, and the margins are maps_reading.margins(kappa, W, H), which
derives them from the operation counts: max(1e-3, 48 kappa 2^-24 max(W, H)) pixels, max(1e-5, 128 kappa 2^-24) on s, 1e-5 on n . n_q.
The caps do not move."""
import ctypes as C

import numpy as np
import pytest

import camera_scenes as cs
from maps_reading import DEPTH_TOL, NORMAL_COS, agree64, cameras64, expected_ids, fused64, margins, popcount, render64
from mvskit_amd import engine, synth
from mvskit_amd.engine import MVS_ERR_CAPACITY, MVS_ERR_STATE
from scene_support import PLAIN, cached_scene, engine_with_pool, mask_at

pytestmark = pytest.mark.gpu


def _check_fused(e, pts, maps, cams, want, source, dedupe, edge_px=1e-3):
    """the records of one fused_points call against the reading's (emit, sure) masks; -> the set of (view, y, x) emitted"""
    got = set()
    last = (-1, -1, -1)
    n_sure = 0
    for v, cam in enumerate(cams):
        r = pts[pts["view"] == v]
        if r.shape[0] == 0:
            continue
        h = r["xyz"].astype(np.float64) @ cam["P"][:, :3].T + cam["P"][:, 3]
        px, py = h[:, 0] / h[:, 2], h[:, 1] / h[:, 2]
        x, y = np.rint(px).astype(int), np.rint(py).astype(int)
        assert np.abs(px - x).max() < edge_px and np.abs(py - y).max() < edge_px, "xyz does not project onto its pixel"
        assert (x >= 0).all() and (x < cam["W"]).all() and (y >= 0).all() and (y < cam["H"]).all()
        assert (r["rgb"] == e.pyramid(v, e.cfg.level)[y, x]).all()
        assert r["normal"].tobytes() == maps[v]["normal"][y, x].tobytes() and r["conf"].tobytes() == maps[v]["conf"][y, x].tobytes()
        emit, sure = want[v]
        assert not (sure[y, x] & ~emit[y, x]).any(), "a pixel the reading does not emit"
        n_sure += int(sure[y, x].sum())
        for k in zip(y.tolist(), x.tolist()):
            assert (v,) + k > last, "records out of (view, y, x) order"
            last = (v,) + k
            got.add(last)
    assert (np.diff(pts["view"].astype(int)) >= 0).all()
    assert n_sure == sum(int((emit & sure).sum()) for emit, sure in want), "the count over the pixels inside the margins differs"
    assert len(got) == pts.shape[0]
    return got


def _case(sc, ekw, source=0, masks=None, sizes=None, list_cap=None, seeds=None, twin=True, kappa=1.0):
    level, csize = ekw["level"], ekw["csize"]
    mg = margins(kappa, sc.W >> level, sc.H >> level)
    sizes = sizes or [(sc.W, sc.H)] * sc.nviews
    seeds = synth.make_seeds(sc, level, csize, stride=1) if seeds is None else seeds
    e = engine_with_pool(sc, ekw, masks, sizes, list_cap, seeds)
    alive = e.patches()
    assert alive.shape[0] > 0 and np.unique(alive["id"]).shape[0] == alive.shape[0] and (alive["id"] >= 0).all()
    pat = np.zeros(int(alive["id"].max()) + 1, alive.dtype)  # the records by pool index, which is what the maps' ids are
    pat[alive["id"]] = alive
    thr = e.thresholds()
    cams = cameras64(sc, level, sizes)
    lmasks = [None if masks is None or masks[v] is None else mask_at(masks[v], sizes[v], level) for v in range(sc.nviews)]
    maps = e.render_maps(source=source, depth_tol=DEPTH_TOL, normal_cos=NORMAL_COS)
    assert (e.valid_pixels(source=source) == [int((m["ids"] >= 0).sum()) for m in maps]).all()
    # ids, normal, conf: exact; depth within the bound
    ids, X, worst = [], [], 0.0
    for v, cam in enumerate(cams):
        m = maps[v]
        want_ids = expected_ids(e, v, 1 if source == 0 else 0, csize, cam, lmasks[v])
        depth, Xv, cos, t = render64(pat, want_ids, cam)
        have = want_ids >= 0
        assert (cos[have] > 0.3).all() and (t[have] > 0).all() and (depth[have] > 0).all(), "the scene has a grazing or back-facing selection"
        assert (m["ids"] == want_ids).all(), f"view {v}: ids differ from depth_normal_map's"
        assert m["normal"][have].tobytes() == pat["normal"][want_ids[have]][:, :3].tobytes()
        assert m["conf"][have].tobytes() == pat["ncc"][want_ids[have]].tobytes()
        for k in ("depth", "normal", "conf"):
            assert np.isnan(m[k][~have]).all() and not np.isnan(m[k][have]).any()
        assert (m["agree"][~have] == 0).all()
        ratio = np.abs(m["depth"][have].astype(np.float64) - depth[have]) / np.abs(depth[have]) / (2e-5 * kappa / cos[have])
        worst = max(worst, float(ratio.max()) if have.any() else 0.0)
        ids.append(want_ids)
        X.append(Xv)
    print(f"maps: depth error at most {worst:.4f} of its bound")
    assert worst <= 1.0
    # agree: every bit outside the margins
    bits, unsure = [], []
    nvalid = nout = none = full = 0
    hist = np.zeros(sc.nviews, int)
    for v in range(sc.nviews):
        b, u = agree64(pat, ids, X, cams, v, DEPTH_TOL, NORMAL_COS, mg["edge"], mg["s"], mg["cos"])
        got = maps[v]["agree"]
        assert (((got >> np.uint64(v)) & np.uint64(1)) == 0).all(), f"view {v}: its own bit is set"
        assert ((got >> np.uint64(sc.nviews)) == 0).all(), f"view {v}: a bit beyond the last view is set"
        assert ((got ^ b) & ~u == 0).all(), f"view {v}: an agree bit outside the margins differs from the float64 reading"
        have = ids[v] >= 0
        pc = popcount(b)[have]
        hist += np.bincount(pc, minlength=sc.nviews)[:sc.nviews]
        nvalid += int(have.sum()); nout += int((u[have] != 0).sum()); none += int((pc == 0).sum()); full += int((pc == sc.nviews - 1).sum())
        bits.append(b)
        unsure.append(u)
    print(f"maps: {nvalid} valid pixels, agreeing views histogram {hist.tolist()}, {nout / nvalid:.4f} outside the margins")
    assert nout < 0.05 * nvalid, "the float64 reading leaves out too many pixels"
    assert none >= 0.10 * nvalid and full >= 0.10 * nvalid, f"one-sided case: {none} pixels without and {full} with all views agreeing of {nvalid}"
    # fused points
    c = e._maps_config(source, 1, DEPTH_TOL, NORMAL_COS, 1)
    n = C.c_int64()
    e._check(e.L.mvs_engine_fused_points(e.h, C.byref(c), 0, None, C.byref(n)))
    pts = e.fused_points(source=source, min_consistent=1, depth_tol=DEPTH_TOL, normal_cos=NORMAL_COS)
    assert pts.shape[0] == n.value > 0, "the size call and the real count differ"
    again = e.fused_points(source=source, min_consistent=1, depth_tol=DEPTH_TOL, normal_cos=NORMAL_COS)
    assert again.tobytes() == pts.tobytes(), "two calls give different bytes"
    small = np.frombuffer(bytearray(b"\xab" * (32 * n.value)), dtype=engine.FUSED_POINT_DTYPE)
    keep = small.tobytes()
    m = C.c_int64()
    assert e.L.mvs_engine_fused_points(e.h, C.byref(c), n.value - 1, small.ctypes.data_as(C.c_void_p), C.byref(m)) == MVS_ERR_CAPACITY
    assert m.value == n.value and small.tobytes() == keep, "a call with cap = n - 1 wrote to out"
    deduped = _check_fused(e, pts, maps, cams, fused64(ids, bits, unsure, 1, True), source, True, mg["edge"])
    all_pts = e.fused_points(source=source, min_consistent=1, depth_tol=DEPTH_TOL, normal_cos=NORMAL_COS, dedupe=False)
    everyone = _check_fused(e, all_pts, maps, cams, fused64(ids, bits, unsure, 1, False), source, False, mg["edge"])
    assert deduped <= everyone and len(everyone) > len(deduped), "dedupe = 0 does not emit a superset"
    print(f"maps: {pts.shape[0]} fused points, {all_pts.shape[0]} without dedupe")
    # nothing of the engine's state moved: the pool, the thresholds, and the pass that follows against a twin that never rendered
    assert e.patches().tobytes() == alive.tobytes() and e.thresholds() == thr
    if twin:
        t = engine_with_pool(sc, ekw, masks, sizes, list_cap, seeds)
        assert t.patches().tobytes() == alive.tobytes()
        assert e.propagate(1) == t.propagate(1)
        assert e.patches().tobytes() == t.patches().tobytes()
        t.close()
    e.close()
    return maps, pts


@pytest.mark.parametrize("source", [0, 1])
def test_plain(source):
    """3 views of 96 x 64, csize 2, level 0: the plain path, both selections"""
    _case(cached_scene(3, 96, 64, 30.0), PLAIN, source=source)


@pytest.mark.parametrize("family", cs.FAMILIES)
def test_camera_families(family):
    """3 views of 96 x 64 on the plane, off the arc: rolled views (the agreement gather takes a pixel of a view turned by 90 degrees to
    a column of another), per-view intrinsics and distances (P_L, Minv, centre and oaxis indexed by view), the world at (6, -4, 8)
    (`far`, and `mixed` with all three)"""
    sc = cs.reading_scene(family)
    _case(sc, PLAIN, kappa=cs.kappa(sc))


def test_ragged_grid():
    """4 views of 97 x 63, csize 3: the last cell column is one pixel wide, the tiles overhang the image"""
    _case(cached_scene(4, 97, 63, 30.0), dict(level=0, csize=3, minImageNum=2, depth=0, max_patches=4 * 33 * 21 * 2 * 9))


def test_level_one():
    """3 views of 192 x 128 at level 1: P_L, Minv and the mask of a level above 0"""
    sc = cached_scene(3, 192, 128, 30.0)
    band = np.full((sc.H, sc.W), 255, np.uint8)
    band[:, 150:171] = 0
    _case(sc, dict(level=1, csize=2, minImageNum=2, depth=0), masks=[None, band, None])


def test_unequal_views():
    """views of 96 x 64 and 80 x 56: per-view sizes in the agreement gather"""
    _case(cached_scene(2, 96, 64, 15.0), PLAIN, sizes=[(96, 64), (80, 56)])


def test_mask_band():
    """view 0 with a background band: holes in its maps, and the other views' pixels that project into the band agree with nothing there"""
    sc = cached_scene(3, 96, 64, 30.0)
    band = np.full((sc.H, sc.W), 255, np.uint8)
    band[:, 20:31] = 0
    maps, _ = _case(sc, PLAIN, masks=[band, None, None])
    assert (maps[0]["ids"][:, 20:31] == -1).all() and (maps[0]["ids"][:, :20] >= 0).mean() > 0.5
    assert ((maps[1]["agree"] & np.uint64(1)) == 0).any() and ((maps[1]["agree"] & np.uint64(1)) != 0).any()


def test_many_views():
    """40 views of 48 x 32, the 64-view library (192-byte records), make_seeds(stride=2): bits 32..39 of agree.
    Not on an arc of 60 degrees: a pixel has 39 pairs there, each within 1e-3 pixel of a rounding boundary with probability 4e-3, so the
    float64 reading alone leaves out 13 % of the valid pixels (seen on the CPU oracle's pool) and no pixel has all 39 views agreeing.  On an
    arc of 1 degree every point projects within a fifth of a pixel of a pixel centre in every view.  For the two-sided histogram the seeds
    are exact to 2 % of a pixel footprint and half a degree where x < 0 and off by 10 footprints and 12 degrees where x >= 0 (a patch of
    the second kind still faces its camera: |cos(n, dir)| > 0.3); the CPU oracle's pool gave 45 % of the valid pixels without and 38 %
    with all views agreeing, 0.6 % outside the margins."""
    sc = cached_scene(40, 48, 32, 1.0)
    seeds = synth.make_seeds(sc, 0, 2, stride=2, depth_noise=0.02, normal_noise_deg=0.5)
    rough = synth.make_seeds(sc, 0, 2, stride=2, depth_noise=10.0, normal_noise_deg=12.0, seed=4242)
    assert seeds.shape == rough.shape and (seeds["images"][:, 0] == rough["images"][:, 0]).all()
    right = seeds["coord"][:, 0] >= 0
    seeds[right] = rough[right]
    seeds["id"] = np.arange(seeds.shape[0])
    maps, pts = _case(sc, dict(level=0, csize=2, minImageNum=3, depth=0), list_cap=64, seeds=seeds)
    high = np.uint64(0xFF) << np.uint64(32)
    assert any(((m["agree"] & high) != 0).any() for m in maps[:32]), "no bit above 31 is ever set"
    assert (pts["view"] < 40).all()


def test_empty_pool_and_staged_pass():
    """an empty pool gives all-hole maps and no points; a pass staged and not committed is refused on the host"""
    sc = cached_scene(3, 96, 64, 30.0)
    e = engine_with_pool(sc, PLAIN, None, None, None, None)
    for source in (0, 1):
        maps = e.render_maps(source=source)
        for m in maps:
            assert m["ids"].shape == (64, 96) and (m["ids"] == -1).all() and (m["agree"] == 0).all()
            assert np.isnan(m["depth"]).all() and np.isnan(m["normal"]).all() and np.isnan(m["conf"]).all()
        assert (e.valid_pixels(source=source) == 0).all()
        assert e.fused_points(source=source, min_consistent=0).shape[0] == 0
    with pytest.raises(engine.EngineError) as err:
        e.fused_points(min_consistent=3)  # more than the two other views
    assert err.value.status == -1
    e.upload_patches(synth.make_seeds(sc, 0, 2, stride=4))
    e.engine_pass(0, 0)
    for call in (e.render_maps, e.fused_points):
        with pytest.raises(engine.EngineError) as err:
            call()
        assert err.value.status == MVS_ERR_STATE
    e.commit_local()
    assert e.render_maps(views=[1])[0] is None
    e.close()


def test_device_pointers():
    """outputs as torch device tensors: the same bytes as through host pointers"""
    import torch

    sc = cached_scene(3, 96, 64, 30.0)
    e = engine_with_pool(sc, PLAIN, None, None, None, synth.make_seeds(sc, 0, 2, stride=1))
    host = e.render_maps(depth_tol=DEPTH_TOL, normal_cos=NORMAL_COS)
    pts = e.fused_points(depth_tol=DEPTH_TOL, normal_cos=NORMAL_COS)
    dev = torch.device("cuda", e.cfg.device)
    kinds = dict(depth=((64, 96), torch.float32), normal=((64, 96, 3), torch.float32), conf=((64, 96), torch.float32), ids=((64, 96), torch.int32),
                 agree=((64, 96), torch.int64))
    tens = [{k: torch.zeros(shape, dtype=dt, device=dev) for k, (shape, dt) in kinds.items()} for _ in range(3)]
    slots = (engine.ViewMaps * 3)()
    for v in range(3):
        for k, t in tens[v].items():
            setattr(slots[v], k, t.data_ptr())
    c = e._maps_config(0, 1, DEPTH_TOL, NORMAL_COS, 1)
    nvalid = np.zeros(3, np.int64)
    torch.cuda.synchronize(dev)
    e._check(e.L.mvs_engine_render_maps(e.h, C.byref(c), slots, nvalid.ctypes.data_as(C.c_void_p)))
    for v in range(3):
        for k, t in tens[v].items():
            assert t.cpu().numpy().tobytes() == host[v][k].tobytes(), (v, k)
        assert nvalid[v] == (host[v]["ids"] >= 0).sum()
    out = torch.zeros((pts.shape[0], 32), dtype=torch.uint8, device=dev)
    n = C.c_int64()
    torch.cuda.synchronize(dev)
    e._check(e.L.mvs_engine_fused_points(e.h, C.byref(c), pts.shape[0], C.c_void_p(out.data_ptr()), C.byref(n)))
    assert n.value == pts.shape[0] > 0 and out.cpu().numpy().tobytes() == pts.tobytes()
    e.close()
