"""The cold start on the GPU: mvs_engine_seed_random against code from before it, mvs_engine_probe's ops 1, 0, 2 and 3.

The yardstick chain (_yardstick): the hypotheses of every cell (mvs_engine_seed_random_hypotheses) go through MVS_PROBE_PREPROCESS and
MVS_PROBE_NCC; numpy picks each cell's winner -- the highest score strictly above min_ncc, the lowest k among equals, among the
hypotheses whose preProcess flag is 0, in the cells the mask gate lets through; the winner of cell c sits at batch index c of a batch of
gw * gh records (a valid record in the other slots), so that MVS_PROBE_REFINE's key (0, 0, i, 0) is the kernel's; then
MVS_PROBE_REFINE and MVS_PROBE_POSTPROCESS, and the records with flag 0 are kept, in (view, cell) order.  What seed_random appended
must be that list byte for byte, `id` and `flags` aside.

Against a vacuous pass every parity case (the wide one aside) draws its depths from the true scene depth of each view -2 % / +2 % with
max_tilt 10 degrees, and the chain itself must keep a patch in at least half of the cells the mask gate lets through."""
import functools
import math

import numpy as np
import pytest

import oracle_binding as ob
from mvskit_amd import engine, synth
from test_gpu_parity import _pair

pytestmark = pytest.mark.gpu
TILT10 = math.radians(10.0)
COUNTERS = ("candidates", "prefiltered", "patches", "fail0", "fail1", "inserted", "replaced", "evals", "view_evals", "trimmed")


@functools.lru_cache(maxsize=None)
def _scene(nviews, W, H, arc, kind="plane"):
    return synth.make_scene(nviews=nviews, W=W, H=H, arc_deg=arc, radius=4.0, kind=kind)


def _sizes(sc, sizes):
    return sizes or [(sc.W, sc.H)] * sc.nviews


def _true_depths(sc, sizes=None):
    """per view the smallest and largest true depth along the optical axis (the third row of P = K [R | t] is (R_z, t_z), K's being
    (0, 0, 1)) over the view's pixels"""
    lo, hi = [], []
    for v, (w, h) in enumerate(_sizes(sc, sizes)):
        X = sc.points[v, :h, :w].reshape(-1, 3).astype(np.float64)
        X = X[np.isfinite(X).all(axis=1)]
        P = sc.P[v].astype(np.float64)
        z = (X @ P[2, :3] + P[2, 3]) / np.linalg.norm(P[2, :3])
        lo.append(z.min())
        hi.append(z.max())
    return np.array(lo), np.array(hi)


def _ranges(sc, sizes=None, lo=0.98, hi=1.02):
    a, b = _true_depths(sc, sizes)
    return (a * lo).astype(np.float32), (b * hi).astype(np.float32)


def _mask_at(mask, size, level):
    """the view's mask at `level` as the engine builds it: > 127 at level 0, then 2 x 2 blocks (clamped at the border), foreground
    where any of the four is"""
    m = np.asarray(mask)[:size[1], :size[0]] > 127
    for _ in range(level):
        ys = 2 * np.arange(max(m.shape[0] >> 1, 1))[:, None] + np.arange(2)
        xs = 2 * np.arange(max(m.shape[1] >> 1, 1))[:, None] + np.arange(2)
        ys, xs = np.minimum(ys, m.shape[0] - 1), np.minimum(xs, m.shape[1] - 1)
        m = m[ys[:, None, :, None], xs[None, :, None, :]].any(axis=(2, 3))
    return m


def _gate(e, v, size, masks, level, csize):
    """the mask gate of every cell of view v: the cell centre's pixel at `level` inside the image and on the foreground of the mask at
    that level, if the view has one"""
    gw, gh = e.grid_dims(v)
    w, h = size[0] >> level, size[1] >> level
    cy, cx = np.divmod(np.arange(gw * gh), gw)
    px = np.floor(np.float32(csize * (2 * cx + 1) - 1) / np.float32(2) + np.float32(0.5)).astype(int)
    py = np.floor(np.float32(csize * (2 * cy + 1) - 1) / np.float32(2) + np.float32(0.5)).astype(int)
    ok = (px >= 0) & (px < w) & (py >= 0) & (py < h)
    if masks is not None and masks[v] is not None:
        m = _mask_at(masks[v], size, level)
        assert m.shape == (h, w)
        ok &= m[np.clip(py, 0, h - 1), np.clip(px, 0, w - 1)]
    return ok


def _yardstick(e, sc, lo, hi, K, seed, tilt, masks, sizes, level, csize, min_ncc=None):
    """-> (the records the chain keeps, in (view, cell) order; the number of cells the gate lets through)"""
    thr = np.float32(e.thresholds()[1] if min_ncc is None else min_ncc)
    kept, gated = [], 0
    for v in range(sc.nviews):
        gw, gh = e.grid_dims(v)
        n = gw * gh
        hyp = e.seed_random_hypotheses(v, np.arange(n), lo, hi, hypotheses=K, seed=seed, max_tilt=tilt, min_ncc=min_ncc)
        assert hyp.shape[0] == n * K
        pre, _, flag = e.probe(engine.PROBE_PREPROCESS, hyp)
        _, ncc, _ = e.probe(engine.PROBE_NCC, pre)
        gate = _gate(e, v, _sizes(sc, sizes)[v], masks, level, csize)
        gated += int(gate.sum())
        best = np.full(n, thr, np.float32)
        win = np.full(n, -1)
        for k in range(K):  # ascending k and a strict comparison: the lowest k among equals; a NaN never wins
            s = ncc[k::K]
            with np.errstate(invalid="ignore"):
                take = gate & (flag[k::K] == 0) & (s > best)
            best[take] = s[take]
            win[take] = k
        cells = np.nonzero(win >= 0)[0]
        if cells.size == 0:
            continue
        first = cells[0] * K + win[cells[0]]
        batch = np.repeat(pre[first:first + 1], n)
        batch[cells] = pre[cells * K + win[cells]]
        ref, _, _ = e.probe(engine.PROBE_REFINE, batch)
        post, _, pflag = e.probe(engine.PROBE_POSTPROCESS, ref)
        kept.append(post[cells[pflag[cells] == 0]])
    return (np.concatenate(kept) if kept else np.zeros(0, e.dtype)), gated


def _strip(recs):
    r = recs.copy()
    r["id"] = 0
    r["flags"] = 0
    return r


def _case(sc, ekw, K, tilt=TILT10, wide=False, seed=1, masks=None, sizes=None, list_cap=None, seeds=None, refiner=None, min_kept=0.5):
    """seed_random on an engine (over `seeds`, if any, which must come through untouched), then the yardstick chain on the same engine
    with the pool put back to the seeds; asserts equality and the floor on what the chain keeps.  -> the appended records"""
    level, csize = ekw["level"], ekw["csize"]
    lo, hi = _ranges(sc, sizes, 0.5, 2.0) if wide else _ranges(sc, sizes)
    e = engine.Engine(sc.nviews, list_cap=list_cap, enable_check=0, **ekw)
    e.set_scene(sc, masks=masks, sizes=sizes)
    if refiner:
        e.set_refiner(**refiner)
    if seeds is not None:
        e.upload_patches(seeds)
    before = e.patches()
    added = e.seed_random(lo, hi, hypotheses=K, seed=seed, max_tilt=tilt)
    after = e.patches()
    assert after.shape[0] == before.shape[0] + added
    assert after[:before.shape[0]].tobytes() == before.tobytes(), "seed_random modified an existing record"
    got = after[before.shape[0]:]
    assert (got["flags"] == 1).all() and (after["id"] == np.arange(after.shape[0])).all()
    e.clear_patches()
    if seeds is not None:
        e.upload_patches(seeds)
    want, gated = _yardstick(e, sc, lo, hi, K, seed, tilt, masks, sizes, level, csize)
    e.close()
    print(f"seed_random: {added} appended, chain keeps {want.shape[0]} of {gated} gated cells ({want.shape[0] / max(gated, 1):.3f})")
    assert got.shape[0] == want.shape[0], (got.shape[0], want.shape[0])
    assert _strip(got).tobytes() == _strip(want).tobytes()
    if min_kept:
        assert want.shape[0] >= min_kept * gated, f"the yardstick chain keeps {want.shape[0]} patches in {gated} cells: the case shows too little"
    return got


PLAIN = dict(level=0, csize=2, minImageNum=2, depth=0)


def test_plain():
    """3 views of 96 x 64, csize 2, level 0, K 4, depth 0: 1536 cells per view"""
    sc = _scene(3, 96, 64, 30.0)
    got = _case(sc, PLAIN, K=4)
    assert (got["nvimages"] == 0).all()


def test_wide_range():
    """0.5 x to 2 x the true depth and tilts up to pi / 3: held to bit-equality only"""
    _case(_scene(3, 96, 64, 30.0), PLAIN, K=4, tilt=math.pi / 3, wide=True, min_kept=0)


def test_level_and_depth():
    """level 1 and depth 1 over a few uploaded patches: postProcess reads the depth maps of the pool as it was at entry, and the
    uploaded records (m_ncc = -1, which an index build would score) stay as they are"""
    sc = _scene(3, 192, 128, 30.0)
    seeds = synth.make_seeds(sc, level=1, csize=2, stride=8)
    assert 10 < seeds.shape[0] < 200
    got = _case(sc, dict(level=1, csize=2, minImageNum=2, depth=1), K=4, seeds=seeds)
    assert (got["nvimages"] >= 0).all()


def test_ragged_grids():
    """97 x 63 and csize 3: 33 x 21 cells, the last column's centre pixel (97) lies outside the image and gives nothing"""
    sc = _scene(3, 97, 63, 30.0)
    cells = 3 * 33 * 21
    _case(sc, dict(level=0, csize=3, minImageNum=2, depth=0, max_patches=cells * 2 * 9), K=4)


def test_unequal_views():
    sc = _scene(2, 96, 64, 15.0)
    _case(sc, PLAIN, K=4, sizes=[(96, 64), (80, 56)])


def test_mask_band():
    """view 0 with a background band, views 1 and 2 without a mask: the band's cells of view 0 give nothing"""
    sc = _scene(3, 96, 64, 30.0)
    band = np.full((sc.H, sc.W), 255, np.uint8)
    band[:, 20:31] = 0
    got = _case(sc, PLAIN, K=4, masks=[band, None, None])
    P = sc.P[0].astype(np.float64)
    mine = got[got["images"][:, 0] == 0]
    x = mine["coord"][:, :3].astype(np.float64) @ P[:, :3].T + P[:, 3]
    px = np.floor(x[:, 0] / x[:, 2] + 0.5)
    assert mine.shape[0] > 0 and not ((px >= 20) & (px <= 30)).any()  # postProcess' own mask test: no patch on the band


def test_mask_level1():
    """a masked view at level 1: the gate reads the mask of that level (48 columns of level 0 are background, 24 of level 1), indexed
    with that level's width"""
    sc = _scene(3, 192, 128, 30.0)
    band = np.full((sc.H, sc.W), 255, np.uint8)
    band[:, 41:89] = 0  # odd start: column 20 of level 1 keeps a foreground pixel (40) and stays foreground, 21..43 are background
    masks = [band, None, None]
    assert (~_mask_at(band, (192, 128), 1)).sum() == 23 * 64
    got = _case(sc, dict(level=1, csize=2, minImageNum=2, depth=0), K=4, masks=masks)
    assert (got["images"][:, 0] == 0).any()


@pytest.mark.parametrize("K", [1, 64])
def test_k_extremes(K):
    """a 24 x 16 grid: 96 x 64 at csize 4"""
    _case(_scene(3, 96, 64, 30.0), dict(level=0, csize=4, minImageNum=2, depth=0), K=K)


def test_converged_refiner():
    _case(_scene(3, 96, 64, 30.0), PLAIN, K=4, refiner=dict(mode="converged", max_evals=200, xtol=1e-3))


@pytest.mark.parametrize("list_cap", [16, 64])
def test_many_views(list_cap):
    """20 views of 48 x 32: the 16-view library cuts the lists, the 64-view library (192-byte records) holds them"""
    sc = _scene(20, 48, 32, 60.0)
    got = _case(sc, dict(level=0, csize=2, minImageNum=3, depth=0), K=8, list_cap=list_cap)  # K 8: the call's default
    print("longest list", got["nimages"].max())
    assert got["nimages"].max() == 16 if list_cap == 16 else got["nimages"].max() > 16


def test_hypotheses_alone():
    sc = _scene(3, 96, 64, 30.0)
    level, csize, K = 0, 2, 8
    e = engine.Engine(3, enable_check=0, **PLAIN)
    e.set_scene(sc)
    lo, hi = _ranges(sc)
    tilt = math.pi / 3
    for v in range(3):
        gw, gh = e.grid_dims(v)
        cells = np.arange(gw * gh)
        h = e.seed_random_hypotheses(v, cells, lo, hi, hypotheses=K, seed=5, max_tilt=tilt)
        assert h.tobytes() == e.seed_random_hypotheses(v, cells, lo, hi, hypotheses=K, seed=5, max_tilt=tilt).tobytes()
        other = e.seed_random_hypotheses(v, cells, lo, hi, hypotheses=K, seed=6, max_tilt=tilt)
        assert (other["coord"] != h["coord"]).any(axis=1).mean() > 0.99
        # a sub-list gives the same records: a hypothesis depends on (view, cell, k) alone
        sub = e.seed_random_hypotheses(v, cells[5::7], lo, hi, hypotheses=K, seed=5, max_tilt=tilt)
        assert sub.tobytes() == h.reshape(-1, K)[5::7].tobytes()
        assert (h["nimages"] == 1).all() and (h["images"][:, 0] == v).all() and not h["images"][:, 1:].any() and not h["vimages"].any()
        assert (h["nvimages"] == 0).all() and (h["ncc"] == -1).all() and (h["flags"] == 1).all()
        assert not h["dscale"].any() and not h["ascale"].any() and not h["tmp"].any()
        assert (h["id"].reshape(-1, K) == np.arange(K)).all() and (h["coord"][:, 3] == 1).all()
        X = h["coord"][:, :3].astype(np.float64)
        n = h["normal"][:, :3].astype(np.float64)
        P = sc.P[v].astype(np.float64)
        x = X @ P[:, :3].T + P[:, 3]
        # every pixel in its own cell (PatchManager's rule floor(p + 0.5) / csize), to the 1e-4 pixels the float32 round trip through
        # unproject and this float64 projection can move a pixel that sits on a cell edge (ulp(96) = 7.6e-6, a few operations)
        cy, cx = np.divmod(np.repeat(cells, K), gw)
        for p, c in ((x[:, 0] / x[:, 2], cx), (x[:, 1] / x[:, 2], cy)):
            assert ((p + 0.5 >= csize * c - 1e-4) & (p + 0.5 < csize * (c + 1) + 1e-4)).all()
        z = x[:, 2] / np.linalg.norm(P[2, :3])
        assert (z >= lo[v] - 4 * np.spacing(lo[v])).all() and (z <= hi[v] + 4 * np.spacing(hi[v])).all(), (z.min(), z.max(), lo[v], hi[v])
        assert z.max() - z.min() > 0.9 * (hi[v] - lo[v])  # the range is used
        assert np.abs(np.linalg.norm(n, axis=1) - 1).max() <= 1e-6
        r = sc.centers[v] - X
        r /= np.linalg.norm(r, axis=1, keepdims=True)
        ang = np.arccos(np.clip((r * n).sum(axis=1), -1, 1))
        assert ang.max() <= tilt + 1e-5 and ang.max() > 0.9 * tilt, ang.max()
        # normal.w = -coord . n: three float32 products and sums of magnitude <= |coord|_1
        err = np.abs(h["normal"][:, 3] + (X * n).sum(axis=1))
        assert (err <= 4 * np.finfo(np.float32).eps * np.abs(X).sum(axis=1).clip(1)).all(), err.max()
    e.close()


def _seeded_pool(monkeypatch=None, grid=None, **kw):
    sc = _scene(3, 96, 64, 30.0)
    if grid:
        monkeypatch.setenv("MVS_SWEEP_GRID", grid)
    e = engine.Engine(3, enable_check=0, **{**PLAIN, **kw})
    e.set_scene(sc)
    lo, hi = _ranges(sc)
    return e, sc, lo, hi


def test_determinism(monkeypatch):
    """two engines, the same arguments: the same pool bytes -- also under MVS_SWEEP_GRID, which sizes the sweep's grid and nothing here"""
    pools = []
    for grid in (None, None, "7"):
        e, sc, lo, hi = _seeded_pool(monkeypatch, grid)
        n = e.seed_random(lo, hi, hypotheses=4, max_tilt=TILT10)
        assert n > 0 and e.seed_random(lo, hi, hypotheses=4, max_tilt=TILT10) == n  # a second call appends again
        pools.append(e.patches())
        assert pools[-1].shape[0] == 2 * n
        assert _strip(pools[-1][:n]).tobytes() == _strip(pools[-1][n:]).tobytes()
        e.close()
    assert pools[0].tobytes() == pools[1].tobytes() == pools[2].tobytes()


def test_capacity():
    e, sc, lo, hi = _seeded_pool()
    n = e.seed_random(lo, hi, hypotheses=4, max_tilt=TILT10)
    e.close()
    seeds = synth.make_seeds(sc, stride=16)
    assert n > 100 and seeds.shape[0] > 0
    e, sc, lo, hi = _seeded_pool(max_patches=seeds.shape[0] + n - 1)
    e.upload_patches(seeds)
    before = e.patches()
    with pytest.raises(engine.EngineError) as err:
        e.seed_random(lo, hi, hypotheses=4, max_tilt=TILT10)
    assert err.value.status == -4 and "max_patches" in str(err.value)  # MVS_ERR_CAPACITY
    assert e.patches().tobytes() == before.tobytes()
    e.close()
    e, sc, lo, hi = _seeded_pool(max_patches=seeds.shape[0] + n)  # exactly enough
    e.upload_patches(seeds)
    assert e.seed_random(lo, hi, hypotheses=4, max_tilt=TILT10) == n
    e.close()


def test_state():
    e, sc, lo, hi = _seeded_pool()
    e.upload_patches(synth.make_seeds(sc, stride=8))
    e.engine_pass(0, 0)  # staged, not committed
    with pytest.raises(engine.EngineError) as err:
        e.seed_random(lo, hi, hypotheses=4, max_tilt=TILT10)
    assert err.value.status == -2  # MVS_ERR_STATE
    e.commit_local()
    assert e.seed_random(lo, hi, hypotheses=4, max_tilt=TILT10) > 0
    e.close()
    e = engine.Engine(3, enable_check=0, **PLAIN)  # no views
    with pytest.raises(engine.EngineError) as err:
        e.seed_random(lo, hi)
    assert err.value.status == -2
    with pytest.raises(engine.EngineError) as err:
        e.seed_random(lo, np.array([5.0, np.inf, 5.0], np.float32))
    assert err.value.status == -1  # MVS_ERR_ARG: a range that is not finite
    with pytest.raises(engine.EngineError) as err:
        e.seed_random(hi, lo)
    assert err.value.status == -1  # not ordered
    e.close()


def test_usable_seeds():
    """the seeded pool, downloaded, starts the oracle and a fresh engine alike: one Propagate::run gives equal counters"""
    e, sc, lo, hi = _seeded_pool()
    assert e.seed_random(lo, hi, hypotheses=4, max_tilt=TILT10) > 500
    pool = e.patches()
    e.close()
    o, e2 = _pair(sc, minImageNum=2, seed=7)
    o.add_patches(pool)
    e2.upload_patches(pool)
    co, ce = o.propagate(0), e2.propagate(0)
    assert ce["patches"] > 500
    for k in COUNTERS:
        assert co[k] == ce[k], (k, co, ce)
    o.close()
    e2.close()
