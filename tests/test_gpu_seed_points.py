"""The warm start on the GPU: mvs_engine_seed_points against code from before it, mvs_engine_probe's ops 1, 0, 2 and 3.

The yardstick chain (points_yardstick of tests/scene_support.py): the hypotheses of every point (mvs_engine_seed_points_hypotheses) go through MVS_PROBE_PREPROCESS and
MVS_PROBE_NCC; numpy picks each point's winner among its count[i] hypotheses -- preProcess flag 0, the highest score strictly above
min_ncc, the lowest k among equals; the winner of point i sits at batch index i of a batch of npoints records (a valid record in the
other slots), so that MVS_PROBE_REFINE's key (0, 0, i, 0) is the kernel's; then MVS_PROBE_REFINE and MVS_PROBE_POSTPROCESS, and the
records with flag 0 are kept, in point order.  What seed_points appended must be that list byte for byte, `id` and `flags` aside.

Against a vacuous pass the chain itself must keep a patch for at least half of the points that at least minImageNum views qualify for
(the number of qualifying views is count[i] of a window with K = nviews: with K >= minImageNum that is the same set of points as
count[i] >= minImageNum of the case's own window, and with K = 1, where no count reaches minImageNum, it is the set the share is about).

The scenes are one textured plane seen from an arc of radius 4; the points are the ground-truth surface points of every `stride`-th
pixel of every view, concatenated: what structure-from-motion would hand over, without its noise."""
import numpy as np
import pytest

import camera_scenes as cams_off_arc
from maps_reading import center64, oaxis64
from mvskit_amd import engine, synth
from parity_support import COUNTERS, REL_TOL, pair
from scene_support import PLAIN, cached_scene, mask_at, points_yardstick, strip

pytestmark = pytest.mark.gpu
U = 2.0 ** -24  # the unit roundoff of float32


def _points(sc, stride):
    pts = np.concatenate([sc.points[v, stride // 2::stride, stride // 2::stride].reshape(-1, 3) for v in range(sc.nviews)])
    return np.ascontiguousarray(pts[np.isfinite(pts).all(axis=1)], dtype=np.float32)


def _case(sc, ekw, K, stride=4, pts=None, masks=None, sizes=None, list_cap=None, seeds=None, refiner=None, min_kept=0.5):
    """seed_points on an engine (over `seeds`, if any, which must come through untouched), then the yardstick chain on the same engine
    with the pool put back to the seeds; asserts equality and the floor on what the chain keeps.  -> the appended records"""
    pts = _points(sc, stride) if pts is None else pts
    e = engine.Engine(sc.nviews, list_cap=list_cap, enable_check=0, **ekw)
    e.set_scene(sc, masks=masks, sizes=sizes)
    if refiner:
        e.set_refiner(**refiner)
    if seeds is not None:
        e.upload_patches(seeds)
    before = e.patches()
    added = e.seed_points(pts, hypotheses=K)
    after = e.patches()
    assert after.shape[0] == before.shape[0] + added
    assert after[:before.shape[0]].tobytes() == before.tobytes(), "seed_points modified an existing record"
    got = after[before.shape[0]:]
    assert (got["flags"] == 1).all() and (after["id"] == np.arange(after.shape[0])).all()
    e.clear_patches()
    if seeds is not None:
        e.upload_patches(seeds)
    want, denom = points_yardstick(e, pts, K, ekw["minImageNum"])
    e.close()
    print(f"seed_points: {pts.shape[0]} points, {added} appended, chain keeps {want.shape[0]} of {denom} points with enough views "
          f"({want.shape[0] / max(denom, 1):.3f})")
    assert got.shape[0] == want.shape[0], (got.shape[0], want.shape[0])
    assert strip(got).tobytes() == strip(want).tobytes()
    if min_kept:
        assert want.shape[0] >= min_kept * denom, f"the yardstick chain keeps {want.shape[0]} patches for {denom} points: the case shows too little"
    return got


# ---- the parity cases
@pytest.mark.parametrize("K", [3, 1])
def test_plain(K):
    """3 views of 96 x 64, csize 2, level 0, depth 0, every 4th pixel: 1152 points"""
    sc = cached_scene(3, 96, 64, 30.0)
    assert _points(sc, 4).shape[0] == 1152
    got = _case(sc, PLAIN, K=K)
    assert (got["nvimages"] == 0).all()


def test_level_and_depth():
    """level 1 and depth 1 over a few uploaded patches: postProcess reads the depth maps of the pool as it was at entry"""
    sc = cached_scene(3, 192, 128, 30.0)
    seeds = synth.make_seeds(sc, level=1, csize=2, stride=8)
    assert 10 < seeds.shape[0] < 200
    _case(sc, dict(level=1, csize=2, minImageNum=2, depth=1), K=3, stride=8, seeds=seeds)


def test_ragged_grids():
    """97 x 63 and csize 3: 33 x 21 cells"""
    _case(cached_scene(3, 97, 63, 30.0), dict(level=0, csize=3, minImageNum=2, depth=0), K=3)


def test_unequal_views():
    """views of 96 x 64 and 80 x 56: a point outside the smaller crop qualifies for one view only and leaves the denominator"""
    _case(cached_scene(2, 96, 64, 15.0), PLAIN, K=2, sizes=[(96, 64), (80, 56)])


@pytest.mark.parametrize("list_cap", [16, 64])
def test_many_views(list_cap):
    """20 views of 48 x 32, every view a hypothesis: the 16-view library cuts the lists, the 64-view library (192-byte records) holds them"""
    _case(cached_scene(20, 48, 32, 60.0), dict(level=0, csize=2, minImageNum=3, depth=0), K=20, list_cap=list_cap)


@pytest.mark.parametrize("family", cams_off_arc.FAMILIES)
def test_camera_families(family):
    """3 views of 96 x 64 off the arc (camera_scenes.py; `far` at (300, -150, 500), `mixed` at (12, -8, 16)): the SeedCam table differs
    by view, the nearest views are not the arc's neighbours, the unit vector to the camera is a difference of coordinates hundreds of
    units large"""
    _case(cams_off_arc.family_scene(family, 3, 96, 64, 30.0, "plane"), PLAIN, K=3)


# ---- further cases, each held to bit-equality with the chain
def test_mask_band():
    """view 0 with a background band, views 1 and 2 without a mask: no hypothesis with reference view 0 projects into the band"""
    sc = cached_scene(3, 96, 64, 30.0)
    band = np.full((sc.H, sc.W), 255, np.uint8)
    band[:, 20:31] = 0
    masks = [band, None, None]
    _case(sc, PLAIN, K=3, masks=masks)
    e = engine.Engine(3, enable_check=0, **PLAIN)
    e.set_scene(sc, masks=masks)
    pts = _points(sc, 4)
    hyp, count = e.seed_points_hypotheses(pts, hypotheses=3)
    e.close()
    P = sc.P[0].astype(np.float64)
    x = pts.astype(np.float64) @ P[:, :3].T + P[:, 3]
    px = np.floor(x[:, 0] / x[:, 2] + 0.5)
    inside = (px >= 20) & (px <= 30)
    assert inside.sum() > 50
    views = hyp["images"][:, 0].reshape(-1, 3)
    live = np.arange(3)[None, :] < count[:, None]
    assert not (live & (views == 0))[inside].any()
    assert (live & (views == 0))[~inside].any(axis=1).mean() > 0.9
    assert (count[inside] <= 2).all() and (count[inside] == 2).mean() > 0.9  # views 1 and 2, where both see the point


def test_converged_refiner():
    _case(cached_scene(3, 96, 64, 30.0), PLAIN, K=3, refiner=dict(mode="converged", max_evals=200, xtol=1e-3))


def _bad_points(sc):
    """a NaN point, a point behind every camera (the cameras look at the origin from z > 0: far beyond them), a point that projects
    outside every image (far off to the side, in front of the cameras)"""
    return np.array([[np.nan, 0.0, 0.0], [0.0, 0.0, 50.0], [40.0, 0.0, 0.0]], np.float32)


def test_points_that_give_nothing():
    """bad points interleaved with good ones get count 0 and give nothing; the good points' hypotheses are those of the call without the
    bad ones, and so are -- in records and order -- their patches under the CONVERGED refiner.  (HALVING draws under the point's index
    in the call, which the interleaving shifts: there the chain on the mixed list is the yardstick.)"""
    sc = cached_scene(3, 96, 64, 30.0)
    good = _points(sc, 4)
    bad = _bad_points(sc)
    at = np.array([0, 5, 300, 301, 302, 1151, 1152])  # positions in `good` a bad point goes in front of (1152: behind the last)
    mixed = np.insert(good, at, bad[np.arange(at.size) % 3], axis=0)
    is_bad = np.ones(mixed.shape[0], bool)
    is_bad[np.setdiff1d(np.arange(mixed.shape[0]), at + np.arange(at.size))] = False
    assert is_bad.sum() == at.size and mixed[~is_bad].tobytes() == good.tobytes()
    _case(sc, PLAIN, K=3, pts=mixed)
    e = engine.Engine(3, enable_check=0, **PLAIN)
    e.set_scene(sc)
    hm, cm = e.seed_points_hypotheses(mixed, hypotheses=3)
    hg, cg = e.seed_points_hypotheses(good, hypotheses=3)
    assert (cm[is_bad] == 0).all() and (cm[~is_bad] == cg).all() and (cg > 0).all()
    assert hm.reshape(-1, 3)[~is_bad].tobytes() == hg.tobytes()
    e.set_refiner(mode="converged", max_evals=200, xtol=1e-3)
    n = e.seed_points(good, hypotheses=3)
    assert n > 500 and e.seed_points(mixed, hypotheses=3) == n
    pool = e.patches()
    assert strip(pool[:n]).tobytes() == strip(pool[n:]).tobytes()
    assert e.seed_points(bad, hypotheses=3) == 0
    e.close()


def test_perturbed_points():
    """every point moved by 0.1 scene units along the ray to its own view: held to bit-equality only"""
    sc = cached_scene(3, 96, 64, 30.0)
    pts, rays = [], []
    for v in range(3):
        p = sc.points[v, 2::4, 2::4].reshape(-1, 3)
        pts.append(p)
        rays.append(p - sc.centers[v].astype(np.float32))
    pts, rays = np.concatenate(pts).astype(np.float64), np.concatenate(rays).astype(np.float64)
    sign = np.where(np.arange(pts.shape[0]) % 2 == 0, 0.1, -0.1)[:, None]
    moved = (pts + sign * rays / np.linalg.norm(rays, axis=1, keepdims=True)).astype(np.float32)
    assert np.isfinite(moved).all()
    _case(sc, PLAIN, K=3, pts=moved, min_kept=0)


def _engine(monkeypatch=None, grid=None, **kw):
    sc = cached_scene(3, 96, 64, 30.0)
    if grid:
        monkeypatch.setenv("MVS_SWEEP_GRID", grid)
    e = engine.Engine(3, enable_check=0, **{**PLAIN, **kw})
    e.set_scene(sc)
    return e, sc, _points(sc, 4)


def test_determinism_chunks_and_sweep_grid(monkeypatch):
    """a second call appends the same records again; MVS_SEED_POINTS_CHUNK = 256 (five chunks, the last one short) gives the pool bytes of
    the default, and so does an engine under MVS_SWEEP_GRID, which sizes the sweep's grid and nothing here"""
    pools = []
    for grid, chunk in ((None, None), (None, "256"), ("7", None), (None, "1000")):
        if chunk:
            monkeypatch.setenv("MVS_SEED_POINTS_CHUNK", chunk)
        else:
            monkeypatch.delenv("MVS_SEED_POINTS_CHUNK", raising=False)
        e, sc, pts = _engine(monkeypatch, grid)
        n = e.seed_points(pts)
        assert n > 500 and e.seed_points(pts) == n
        pools.append(e.patches())
        assert pools[-1].shape[0] == 2 * n
        assert strip(pools[-1][:n]).tobytes() == strip(pools[-1][n:]).tobytes()
        hyp = e.seed_points_hypotheses(pts)
        pools.append(hyp[0].tobytes() + hyp[1].tobytes())  # the window streams in chunks too
        e.close()
        monkeypatch.delenv("MVS_SWEEP_GRID", raising=False)
    assert pools[0].tobytes() == pools[2].tobytes() == pools[4].tobytes() == pools[6].tobytes()
    assert pools[1] == pools[3] == pools[5] == pools[7]


def test_capacity():
    e, sc, pts = _engine()
    n = e.seed_points(pts)
    e.close()
    seeds = synth.make_seeds(sc, stride=16)
    assert n > 100 and seeds.shape[0] > 0
    e, sc, pts = _engine(max_patches=seeds.shape[0] + n - 1)
    e.upload_patches(seeds)
    before = e.patches()
    with pytest.raises(engine.EngineError) as err:
        e.seed_points(pts)
    assert err.value.status == -4 and "max_patches" in str(err.value)  # MVS_ERR_CAPACITY
    assert e.patches().tobytes() == before.tobytes()
    e.close()
    e, sc, pts = _engine(max_patches=seeds.shape[0] + n)  # exactly enough
    e.upload_patches(seeds)
    assert e.seed_points(pts) == n
    e.close()


def test_state_and_empty():
    e, sc, pts = _engine()
    assert e.seed_points(np.zeros((0, 3), np.float32)) == 0 and e.num_patches() == 0
    hyp, count = e.seed_points_hypotheses(np.zeros((0, 3), np.float32))
    assert hyp.shape[0] == 0 and count.shape[0] == 0
    lo, hi, cnt = e.depth_ranges(np.zeros((0, 3), np.float32))
    assert not lo.any() and not hi.any() and not cnt.any()
    e.upload_patches(synth.make_seeds(sc, stride=8))
    e.engine_pass(0, 0)  # staged, not committed
    with pytest.raises(engine.EngineError) as err:
        e.seed_points(pts)
    assert err.value.status == -2  # MVS_ERR_STATE
    e.commit_local()
    assert e.seed_points(pts) > 0
    e.close()
    e = engine.Engine(3, enable_check=0, **PLAIN)  # no views
    for call in (e.seed_points, e.seed_points_hypotheses, e.depth_ranges):
        with pytest.raises(engine.EngineError) as err:
            call(pts)
        assert err.value.status == -2
    e.close()


# ---- steps 1 and 2 against a float64 reading
def _reading(sc, pts, level, sizes, masks, off_arc=False):
    """float64: per (point, view) the gate, the depth, the squared camera distance, the sum of the depth's term magnitudes, and whether
    the pair keeps the margins inside which the float32 gate must agree: the projection more than 1e-3 pixel from a rounding boundary
    (image and mask edges are such boundaries), the depth more than 1e-3 of its magnitude from zero.  off_arc: the margin in pixels is
    maps_reading.margins' with the pair's own kappa, max(|X|_inf, |C|_inf) / |depth|: 48 kappa 2^-24 max(w, h) where that exceeds 1e-3"""
    X = pts.astype(np.float64)
    n, nv = X.shape[0], sc.nviews
    ok, safe = np.zeros((n, nv), bool), np.zeros((n, nv), bool)
    depth, dist, mag = np.zeros((n, nv)), np.zeros((n, nv)), np.zeros((n, nv))
    centers = []
    for v in range(nv):
        P32 = np.ascontiguousarray(sc.P[v], dtype=np.float32)
        P = P32.astype(np.float64).copy()
        P[:2] /= 2.0 ** level
        w, h = sizes[v][0] >> level, sizes[v][1] >> level
        o = oaxis64(P32)
        depth[:, v] = X @ o[:3] + o[3]
        mag[:, v] = np.abs(X * o[:3]).sum(axis=1) + abs(o[3])
        x = X @ P[:, :3].T + P[:, 3]
        with np.errstate(divide="ignore", invalid="ignore"):
            px, py = x[:, 0] / x[:, 2] + 0.5, x[:, 1] / x[:, 2] + 0.5
        fx, fy = np.floor(px), np.floor(py)
        inside = (x[:, 2] > 0) & (fx >= 0) & (fx < w) & (fy >= 0) & (fy < h)
        fg = np.ones(n, bool)
        if masks is not None and masks[v] is not None:
            m = mask_at(masks[v], sizes[v], level)
            fg = m[np.clip(fy, 0, h - 1).astype(int), np.clip(fx, 0, w - 1).astype(int)]
        ok[:, v] = inside & fg & (depth[:, v] > 0)
        edge = np.minimum(np.abs(px - np.rint(px)), np.abs(py - np.rint(py)))
        c = center64(P32)
        px_margin = 1e-3
        if off_arc:
            big = np.maximum(np.abs(X).max(axis=1), np.abs(c).max())
            px_margin = np.maximum(1e-3, 48.0 * U * max(w, h) * big / np.maximum(np.abs(depth[:, v]), 1e-30))
        safe[:, v] = (edge > px_margin) & (np.abs(depth[:, v]) > 1e-3 * mag[:, v]) & (np.abs(x[:, 2]) > 1e-3 * (np.abs(X * P[2, :3]).sum(axis=1) + abs(P[2, 3])))
        centers.append(c)
        dist[:, v] = ((c - X) ** 2).sum(axis=1)
    return ok, safe, depth, dist, mag, np.array(centers)


def _probe_points(sc, stride):
    """the scene's points, and copies pushed sideways and towards / beyond the cameras so that views drop out for every reason"""
    base = _points(sc, stride)
    side = base + np.array([1.2, 0.4, 0.0], np.float32)
    target = np.asarray(sc.meta.get("target", (0.0, 0.0, 0.0)), np.float32)  # (0, 0, 0) on the arc: the same bits as without it
    near = (base - target) * np.float32(0.3) + np.array([0.0, 0.0, 2.5], np.float32) + target
    far = base + np.array([0.0, 0.0, 6.0], np.float32)
    return np.ascontiguousarray(np.concatenate([base, side, near, far]), dtype=np.float32)


HYP_CASES = {
    "masked_level1": dict(scene=(3, 192, 128, 30.0), level=1, K=2, stride=8, band=(41, 89)),
    "twenty_views": dict(scene=(20, 48, 32, 60.0), level=0, K=20, stride=4, band=None),
    "three_of_twenty": dict(scene=(20, 48, 32, 60.0), level=0, K=3, stride=4, band=None),
    # cameras off the arc (camera_scenes.py): 4 views of 96 x 64 of the plane, `mixed` at (12, -8, 16)
    "intrinsics": dict(scene="intrinsics", level=0, K=4, stride=4, band=None),
    "mixed": dict(scene="mixed", level=0, K=4, stride=4, band=None),
}


def _hyp_setup(name):
    cs = HYP_CASES[name]
    off_arc = isinstance(cs["scene"], str)
    sc = cams_off_arc.family_scene(cs["scene"], 4, 96, 64, 30.0, "plane") if off_arc else cached_scene(*cs["scene"])
    masks = None
    if cs["band"]:
        band = np.full((sc.H, sc.W), 255, np.uint8)
        band[:, cs["band"][0]:cs["band"][1]] = 0
        masks = [band] + [None] * (sc.nviews - 1)
    e = engine.Engine(sc.nviews, enable_check=0, level=cs["level"], csize=2, minImageNum=2, depth=0)
    e.set_scene(sc, masks=masks)
    pts = _probe_points(sc, cs["stride"])
    sizes = [(sc.W, sc.H)] * sc.nviews
    ok, safe, depth, dist, mag, centers = _reading(sc, pts, cs["level"], sizes, masks, off_arc)
    # the points of the test: every (point, view) pair inside the margins, camera distances more than 1e-4 apart (relative)
    sd = np.sort(dist, axis=1)
    apart = ((sd[:, 1:] - sd[:, :-1]) > 1e-4 * sd[:, 1:]).all(axis=1)
    sel = safe.all(axis=1) & apart
    assert sel.mean() > 0.8, sel.mean()
    return e, sc, cs, pts[sel], ok[sel], depth[sel], dist[sel], mag[sel], centers


@pytest.mark.parametrize("name", list(HYP_CASES))
def test_hypotheses_against_float64(name):
    e, sc, cs, pts, ok, depth, dist, mag, centers = _hyp_setup(name)
    K, n = cs["K"], pts.shape[0]
    hyp, count = e.seed_points_hypotheses(pts, hypotheses=K)
    again = e.seed_points_hypotheses(pts, hypotheses=K)
    assert hyp.tobytes() == again[0].tobytes() and (count == again[1]).all()
    e.close()
    nq = ok.sum(axis=1)
    print(f"{name}: {n} points, qualifying views min {nq.min()} max {nq.max()}, none for {(nq == 0).sum()}")
    assert (nq == 0).any() and (nq == sc.nviews).any() and ((nq > 0) & (nq < sc.nviews)).any()  # every kind of point is there
    assert (count == np.minimum(nq, K)).all()
    order = np.argsort(np.where(ok, dist, np.inf), axis=1, kind="stable")[:, :K]  # ascending distance, the lower view first among equals
    h = hyp.reshape(n, K)
    live = np.arange(K)[None, :] < count[:, None]
    assert not h[~live].view(np.uint8).any()
    assert (h["images"][:, :, 0][live] == order[live]).all()
    r = h[live]
    assert (r["nimages"] == 1).all() and not r["images"][:, 1:].any() and not r["vimages"].any() and (r["nvimages"] == 0).all()
    assert (r["ncc"] == -1).all() and (r["flags"] == 1).all() and not r["dscale"].any() and not r["ascale"].any() and not r["tmp"].any()
    assert (h["id"][live] == np.broadcast_to(np.arange(K), (n, K))[live]).all()
    src = np.broadcast_to(pts[:, None, :], (n, K, 3))[live]
    assert r["coord"][:, :3].tobytes() == np.ascontiguousarray(src).tobytes() and (r["coord"][:, 3] == 1).all()  # the input bits
    # the normal: the unit vector to the reference camera.  In float32 it passes a subtraction (half an ulp of the component), the norm's
    # fma chain, a correctly rounded square root and reciprocal (together under 2.5 ulp on the common factor) and one product (half an
    # ulp): within 4 ulp of every component of the float64 value
    X = src.astype(np.float64)
    t = centers[order[live]] - X
    want = t / np.linalg.norm(t, axis=1, keepdims=True)
    got = r["normal"][:, :3].astype(np.float64)
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    err = np.abs(got - want) / ulp
    print(f"{name}: normal error at most {err.max():.2f} ulp")
    assert (err <= 4).all(), err.max()
    # normal.w = -coord . n of the record's own n: three products and two sums in float32, each within half an ulp of a partial sum no
    # larger than sum |coord_j n_j|: within 4 ulp of that magnitude
    m = np.abs(X * got).sum(axis=1)
    werr = np.abs(r["normal"][:, 3].astype(np.float64) + (X * got).sum(axis=1)) / np.spacing(m.astype(np.float32)).astype(np.float64)
    print(f"{name}: normal.w error at most {werr.max():.2f} ulp of sum |coord_j n_j|")
    assert (werr <= 4).all(), werr.max()


@pytest.mark.parametrize("name", ["masked_level1", "twenty_views", "intrinsics", "mixed"])
def test_depth_ranges(name):
    e, sc, cs, pts, ok, depth, dist, mag, centers = _hyp_setup(name)
    before = (e.patches().tobytes(), e.thresholds())
    margin = 0.1
    lo, hi, cnt = e.depth_ranges(pts, margin=margin)
    lo0, hi0, cnt0 = e.depth_ranges(pts, margin=0.0)
    again = e.depth_ranges(pts, margin=margin)
    assert lo.dtype == np.float32 and hi.dtype == np.float32
    assert all(a.tobytes() == b.tobytes() for a, b in zip((lo, hi, cnt), again))  # the same bits, whatever the order of the atomics
    assert (cnt == ok.sum(axis=0)).all() and (cnt0 == cnt).all() and (cnt > 0).all()
    # the widening is the host's: one float32 division / product by 1 + margin
    w = np.float32(1) + np.float32(margin)
    assert (lo == lo0 / w).all() and (hi == hi0 * w).all()
    # the extremes against float64: a four-term float32 dot product in any order is within 4 u (sum |o_j X_j| + |o_w|) of the exact one,
    # doubled for the rounding of the axis itself and of the widening that is undone here; the sum is taken at its largest over the
    # view's qualifying points, since the float32 extreme may sit on another point than the float64 one
    worst = 0.0
    for v in range(sc.nviews):
        d = depth[ok[:, v], v]
        bound = 8 * U * mag[ok[:, v], v].max()
        for got, want in ((float(lo[v]) * float(w), d.min()), (float(hi[v]) / float(w), d.max()), (float(lo0[v]), d.min()), (float(hi0[v]), d.max())):
            worst = max(worst, abs(got - want) / bound)
            assert abs(got - want) <= bound, (v, got, want, bound)
    print(f"{name}: depth extremes within {worst:.3f} of the bound")
    # margin 0 returns the exact extremes: those of the depths the same call gives one point at a time
    sub = np.arange(0, pts.shape[0], max(pts.shape[0] // 48, 1))
    one = [e.depth_ranges(pts[i:i + 1], margin=0.0) for i in sub]
    assert all((a == b).all() for a, b, c in one)  # one point: min = max
    d1 = np.array([a for a, b, c in one])
    c1 = np.array([c for a, b, c in one])
    assert ((c1 == 1) == ok[sub]).all()
    los, his, cs_ = e.depth_ranges(pts[sub], margin=0.0)
    for v in range(sc.nviews):
        q = c1[:, v] == 1
        assert cs_[v] == q.sum()
        if q.any():
            assert los[v] == d1[q, v].min() and his[v] == d1[q, v].max()
        else:
            assert los[v] == 0 and his[v] == 0
    assert (e.patches().tobytes(), e.thresholds()) == before and e.num_patches() == 0
    e.close()


def test_depth_ranges_of_a_fully_masked_view():
    sc = cached_scene(3, 96, 64, 30.0)
    e = engine.Engine(3, enable_check=0, **PLAIN)
    e.set_scene(sc, masks=[np.zeros((sc.H, sc.W), np.uint8), None, None])
    pts = _points(sc, 4)
    lo, hi, cnt = e.depth_ranges(pts)
    assert cnt[0] == 0 and lo[0] == 0 and hi[0] == 0 and (cnt[1:] > 1000).all() and (lo[1:] > 0).all() and (hi[1:] > lo[1:]).all()
    with pytest.raises(engine.EngineError) as err:
        e.seed_random(lo, hi)  # the cold start refuses the empty range
    assert err.value.status == -1
    e.close()


# ---- end to end
def test_warm_then_cold_then_propagate():
    """seed_points, then depth_ranges of the same points fed straight into seed_random, which takes them and appends; one Propagate::run
    from that pool in a fresh engine and in the oracle: counters exact, records to 1e-3"""
    e, sc, pts = _engine()
    n = e.seed_points(pts)
    assert n > 500
    lo, hi, cnt = e.depth_ranges(pts)
    assert (cnt > 0).all()
    m = e.seed_random(lo, hi, hypotheses=4)
    print(f"warm start {n} patches, cold start over the points' ranges {m} more")
    assert m > 0
    pool = e.patches()
    assert pool.shape[0] == n + m
    e.close()
    o, e2 = pair(sc, minImageNum=2, seed=7)
    o.add_patches(pool)
    e2.upload_patches(pool)
    co, ce = o.propagate(0), e2.propagate(0)
    assert ce["patches"] > 500
    for k in COUNTERS:
        assert co[k] == ce[k], (k, co, ce)
    po, pe = o.patches(), e2.patches()
    assert po.shape == pe.shape
    np.testing.assert_array_equal(po["nimages"], pe["nimages"])
    np.testing.assert_array_equal(po["images"], pe["images"])
    np.testing.assert_allclose(pe["coord"], po["coord"], rtol=REL_TOL, atol=1e-6)
    np.testing.assert_allclose(pe["normal"], po["normal"], rtol=0, atol=REL_TOL)
    np.testing.assert_allclose(pe["ncc"], po["ncc"], rtol=REL_TOL, atol=1e-6)
    o.close()
    e2.close()
