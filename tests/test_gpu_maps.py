"""Dense per-view maps and their fusion on the GPU: mvs_engine_render_maps / mvs_engine_fused_points against a float64 numpy reading.

The pool of every case: synth.make_seeds uploaded, then propagate(0) once -- the patches carry real m_ncc, lists and some noise.  The
yardstick (_render64, _agree64, _fused64) works on e.patches() and float64 copies of the float32 cameras, read at level L as tests/test_gpu_seed_points.py
reads them (P[:2] /= 2**L, _oaxis64, _center64).  Every decision of the feature is integer-exact against code from before it (the ids of
mvs_engine_depth_normal_map) or lies outside a stated margin, so float64 never disagrees on one: a pair (pixel of v, view u) whose
projection lies within 1e-3 pixel of a rounding boundary (image edges are such boundaries), whose | |s - 1| - depth_tol | is below 1e-5 or
whose |n.n_q - normal_cos| is below 1e-5 is left out (the GPU may set or clear its bit), and a pixel with such a pair is left out of the
fused-point comparison.  Every case asserts that the reading leaves out fewer than 5 % of the valid pixels and finds at least 10 % of them
with no agreeing view and at least 10 % with all other views agreeing: a vacuous or one-sided case fails.

Depth bound: the reading is about 30 float32 operations at unit roundoff 2^-24 divided by the cosine between the normal and the ray, about
2e-6 / cos; the bound 2e-5 / |cos| relative keeps a tenfold margin."""
import ctypes as C

import numpy as np
import pytest

from mvskit_amd import engine, synth
from test_gpu_seed_points import _center64, _oaxis64
from test_gpu_seed_random import _mask_at, _scene

pytestmark = pytest.mark.gpu
DEPTH_TOL, NORMAL_COS = 0.004, 0.98
MVS_ERR_STATE, MVS_ERR_CAPACITY = -2, -4


def _cams(sc, level, sizes):
    """per view the float64 copies of the float32 camera at `level`: P, the inverse of its 3x3 block, the centre, oaxis, W, H"""
    cams = []
    for v in range(sc.nviews):
        P32 = np.ascontiguousarray(sc.P[v], dtype=np.float32)
        P = P32.astype(np.float64).copy()
        P[:2] /= 2.0 ** level
        cams.append(dict(P=P, Minv=np.linalg.inv(P[:, :3]), C=_center64(P32), o=_oaxis64(P32), W=sizes[v][0] >> level, H=sizes[v][1] >> level))
    return cams


def _expected_ids(src, v, kind, csize, cam, mask):
    """the ids grid of depth_normal_map(v, kind) repeated over each cell's pixels, -1 on the mask's background"""
    grid = src.depth_normal_map(v, kind)[2]
    px = np.repeat(np.repeat(grid, csize, axis=0), csize, axis=1)[:cam["H"], :cam["W"]].copy()
    assert px.shape == (cam["H"], cam["W"])
    if mask is not None:
        px[~mask] = -1
    return px


def _render64(pat, ids, cam):
    """step 2 in float64 over one view's id map -> depth, the point, |cos(n, dir)|, t (NaN where ids < 0)"""
    H, W = ids.shape
    y, x = np.mgrid[0:H, 0:W]
    sel = np.maximum(ids, 0)
    n = pat["normal"][sel][..., :3].astype(np.float64)
    X0 = pat["coord"][sel][..., :3].astype(np.float64)
    d = np.stack([x, y, np.ones_like(x)], axis=-1).astype(np.float64) @ cam["Minv"].T
    nd = (n * d).sum(-1)
    t = (n * (X0 - cam["C"])).sum(-1) / nd
    X = cam["C"] + t[..., None] * d
    depth = X @ cam["o"][:3] + cam["o"][3]
    cos = np.abs(nd) / (np.linalg.norm(n, axis=-1) * np.linalg.norm(d, axis=-1))
    hole = ids < 0
    depth[hole], X[hole], cos[hole], t[hole] = np.nan, np.nan, np.nan, np.nan
    return depth, X, cos, t


def _agree64(pat, ids, X, cams, v, tol, ncos):
    """step 3 in float64 for view v -> (bits, unsure): uint64 maps, bit u of `unsure` = the pair (pixel, u) lies inside a margin"""
    bits, unsure = np.zeros(ids[v].shape, np.uint64), np.zeros(ids[v].shape, np.uint64)
    ok = ids[v] >= 0
    Xv = X[v][ok]
    n = pat["normal"][ids[v][ok]][:, :3].astype(np.float64)
    for u, cu in enumerate(cams):
        if u == v:
            continue
        h = Xv @ cu["P"][:, :3].T + cu["P"][:, 3]
        assert (h[:, 2] > 0.1).all()  # every point lies well in front of every camera in these scenes
        px, py = h[:, 0] / h[:, 2] + 0.5, h[:, 1] / h[:, 2] + 0.5
        edge = np.minimum(np.abs(px - np.rint(px)), np.abs(py - np.rint(py))) <= 1e-3
        fx, fy = np.floor(px).astype(int), np.floor(py).astype(int)
        inside = (fx >= 0) & (fx < cu["W"]) & (fy >= 0) & (fy < cu["H"])
        idq = np.where(inside, ids[u][np.clip(fy, 0, cu["H"] - 1), np.clip(fx, 0, cu["W"] - 1)], -1)
        met = idq >= 0
        q = pat[np.maximum(idq, 0)]
        nq, X0q = q["normal"][:, :3].astype(np.float64), q["coord"][:, :3].astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            ds = np.abs((nq * (X0q - cu["C"])).sum(1) / (nq * (Xv - cu["C"])).sum(1) - 1.0)
        nn = (n * nq).sum(1)
        with np.errstate(invalid="ignore"):
            bit = met & (ds <= tol) & ((nn >= ncos) if ncos > -1 else True)
            margin = edge | (met & ((np.abs(ds - tol) < 1e-5) | ((np.abs(nn - ncos) < 1e-5) if ncos > -1 else False)))
        b, m = np.zeros(ids[v].shape, np.uint64), np.zeros(ids[v].shape, np.uint64)
        b[ok], m[ok] = bit.astype(np.uint64) << np.uint64(u), margin.astype(np.uint64) << np.uint64(u)
        bits |= b
        unsure |= m
    return bits, unsure


def _popcount(a):
    return np.unpackbits(np.ascontiguousarray(a).view(np.uint8).reshape(a.shape + (8,)), axis=-1).sum(-1)


def _fused64(ids, bits, unsure, min_consistent, dedupe):
    """step 4 over the reading -> per view the (emit, sure) masks"""
    out = []
    for v in range(len(ids)):
        emit = (ids[v] >= 0) & (_popcount(bits[v]) >= min_consistent)
        if dedupe:
            emit &= (bits[v] & np.uint64((1 << v) - 1)) == 0
        out.append((emit, unsure[v] == 0))
    return out


def _engine(sc, ekw, masks, sizes, list_cap, seeds):
    """a pool of 2^16 records unless the case sizes its own: the default, four per cell, does not hold a seed in every cell plus what one
    iteration adds where a view is a crop or csize is 3"""
    e = engine.Engine(sc.nviews, list_cap=list_cap, enable_check=0, seed=3, **{"max_patches": 1 << 16, **ekw})
    e.set_scene(sc, masks=masks, sizes=sizes)
    if seeds is not None and seeds.shape[0]:
        e.upload_patches(seeds)
        e.propagate(0)
    return e


def _check_fused(e, pts, maps, cams, want, source, dedupe):
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
        assert np.abs(px - x).max() < 1e-3 and np.abs(py - y).max() < 1e-3, "xyz does not project onto its pixel"
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


def _case(sc, ekw, source=0, masks=None, sizes=None, list_cap=None, seeds=None, twin=True):
    level, csize = ekw["level"], ekw["csize"]
    sizes = sizes or [(sc.W, sc.H)] * sc.nviews
    seeds = synth.make_seeds(sc, level, csize, stride=1) if seeds is None else seeds
    e = _engine(sc, ekw, masks, sizes, list_cap, seeds)
    alive = e.patches()
    assert alive.shape[0] > 0 and np.unique(alive["id"]).shape[0] == alive.shape[0] and (alive["id"] >= 0).all()
    pat = np.zeros(int(alive["id"].max()) + 1, alive.dtype)  # the records by pool index, which is what the maps' ids are
    pat[alive["id"]] = alive
    thr = e.thresholds()
    cams = _cams(sc, level, sizes)
    lmasks = [None if masks is None or masks[v] is None else _mask_at(masks[v], sizes[v], level) for v in range(sc.nviews)]
    maps = e.render_maps(source=source, depth_tol=DEPTH_TOL, normal_cos=NORMAL_COS)
    assert (e.valid_pixels(source=source) == [int((m["ids"] >= 0).sum()) for m in maps]).all()
    # ids, normal, conf: exact; depth within the bound
    ids, X, worst = [], [], 0.0
    for v, cam in enumerate(cams):
        m = maps[v]
        want_ids = _expected_ids(e, v, 1 if source == 0 else 0, csize, cam, lmasks[v])
        depth, Xv, cos, t = _render64(pat, want_ids, cam)
        have = want_ids >= 0
        assert (cos[have] > 0.3).all() and (t[have] > 0).all() and (depth[have] > 0).all(), "the scene has a grazing or back-facing selection"
        assert (m["ids"] == want_ids).all(), f"view {v}: ids differ from depth_normal_map's"
        assert m["normal"][have].tobytes() == pat["normal"][want_ids[have]][:, :3].tobytes()
        assert m["conf"][have].tobytes() == pat["ncc"][want_ids[have]].tobytes()
        for k in ("depth", "normal", "conf"):
            assert np.isnan(m[k][~have]).all() and not np.isnan(m[k][have]).any()
        assert (m["agree"][~have] == 0).all()
        ratio = np.abs(m["depth"][have].astype(np.float64) - depth[have]) / np.abs(depth[have]) / (2e-5 / cos[have])
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
        b, u = _agree64(pat, ids, X, cams, v, DEPTH_TOL, NORMAL_COS)
        got = maps[v]["agree"]
        assert (((got >> np.uint64(v)) & np.uint64(1)) == 0).all(), f"view {v}: its own bit is set"
        assert ((got >> np.uint64(sc.nviews)) == 0).all(), f"view {v}: a bit beyond the last view is set"
        assert ((got ^ b) & ~u == 0).all(), f"view {v}: an agree bit outside the margins differs from the float64 reading"
        have = ids[v] >= 0
        pc = _popcount(b)[have]
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
    deduped = _check_fused(e, pts, maps, cams, _fused64(ids, bits, unsure, 1, True), source, True)
    all_pts = e.fused_points(source=source, min_consistent=1, depth_tol=DEPTH_TOL, normal_cos=NORMAL_COS, dedupe=False)
    everyone = _check_fused(e, all_pts, maps, cams, _fused64(ids, bits, unsure, 1, False), source, False)
    assert deduped <= everyone and len(everyone) > len(deduped), "dedupe = 0 does not emit a superset"
    print(f"maps: {pts.shape[0]} fused points, {all_pts.shape[0]} without dedupe")
    # nothing of the engine's state moved: the pool, the thresholds, and the pass that follows against a twin that never rendered
    assert e.patches().tobytes() == alive.tobytes() and e.thresholds() == thr
    if twin:
        t = _engine(sc, ekw, masks, sizes, list_cap, seeds)
        assert t.patches().tobytes() == alive.tobytes()
        assert e.propagate(1) == t.propagate(1)
        assert e.patches().tobytes() == t.patches().tobytes()
        t.close()
    e.close()
    return maps, pts


PLAIN = dict(level=0, csize=2, minImageNum=2, depth=0)


@pytest.mark.parametrize("source", [0, 1])
def test_plain(source):
    """3 views of 96 x 64, csize 2, level 0: the plain path, both selections"""
    _case(_scene(3, 96, 64, 30.0), PLAIN, source=source)


def test_ragged_grid():
    """4 views of 97 x 63, csize 3: the last cell column is one pixel wide, the tiles overhang the image"""
    _case(_scene(4, 97, 63, 30.0), dict(level=0, csize=3, minImageNum=2, depth=0, max_patches=4 * 33 * 21 * 2 * 9))


def test_level_one():
    """3 views of 192 x 128 at level 1: P_L, Minv and the mask of a level above 0"""
    sc = _scene(3, 192, 128, 30.0)
    band = np.full((sc.H, sc.W), 255, np.uint8)
    band[:, 150:171] = 0
    _case(sc, dict(level=1, csize=2, minImageNum=2, depth=0), masks=[None, band, None])


def test_unequal_views():
    """views of 96 x 64 and 80 x 56: per-view sizes in the agreement gather"""
    _case(_scene(2, 96, 64, 15.0), PLAIN, sizes=[(96, 64), (80, 56)])


def test_mask_band():
    """view 0 with a background band: holes in its maps, and the other views' pixels that project into the band agree with nothing there"""
    sc = _scene(3, 96, 64, 30.0)
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
    sc = _scene(40, 48, 32, 1.0)
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
    sc = _scene(3, 96, 64, 30.0)
    e = _engine(sc, PLAIN, None, None, None, None)
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

    sc = _scene(3, 96, 64, 30.0)
    e = _engine(sc, PLAIN, None, None, None, synth.make_seeds(sc, 0, 2, stride=1))
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
