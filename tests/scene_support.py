"""Scenes, seeds and small engines of the seeding and output tests (a helper module like oracle_binding.py): the cached plane
scenes, masks and depth ranges as the engine sees them, the two yardstick chains of the cold and the warm start (mvs_engine_probe's
ops on the hypotheses), the engine with a propagated pool of the maps and mesh tests with their lattice, and a grid mesh."""
import functools

import numpy as np

from mvskit_amd import engine, synth

PLAIN = dict(level=0, csize=2, minImageNum=2, depth=0)
DIMS, SHIFT, TRUNC_VOXELS = (24, 20, 12), (0.31, 0.17, 0.43), 4


@functools.lru_cache(maxsize=None)
def cached_scene(nviews, W, H, arc, kind="plane"):
    return synth.make_scene(nviews=nviews, W=W, H=H, arc_deg=arc, radius=4.0, kind=kind)


def view_sizes(sc, sizes):
    return sizes or [(sc.W, sc.H)] * sc.nviews


def true_depths(sc, sizes=None):
    """per view the smallest and largest true depth along the optical axis (the third row of P = K [R | t] is (R_z, t_z), K's being
    (0, 0, 1)) over the view's pixels"""
    lo, hi = [], []
    for v, (w, h) in enumerate(view_sizes(sc, sizes)):
        X = sc.points[v, :h, :w].reshape(-1, 3).astype(np.float64)
        X = X[np.isfinite(X).all(axis=1)]
        P = sc.P[v].astype(np.float64)
        z = (X @ P[2, :3] + P[2, 3]) / np.linalg.norm(P[2, :3])
        lo.append(z.min())
        hi.append(z.max())
    return np.array(lo), np.array(hi)


def ranges(sc, sizes=None, lo=0.98, hi=1.02):
    a, b = true_depths(sc, sizes)
    return (a * lo).astype(np.float32), (b * hi).astype(np.float32)


def mask_at(mask, size, level):
    """the view's mask at `level` as the engine builds it: > 127 at level 0, then 2 x 2 blocks (clamped at the border), foreground
    where any of the four is"""
    m = np.asarray(mask)[:size[1], :size[0]] > 127
    for _ in range(level):
        ys = 2 * np.arange(max(m.shape[0] >> 1, 1))[:, None] + np.arange(2)
        xs = 2 * np.arange(max(m.shape[1] >> 1, 1))[:, None] + np.arange(2)
        ys, xs = np.minimum(ys, m.shape[0] - 1), np.minimum(xs, m.shape[1] - 1)
        m = m[ys[:, None, :, None], xs[None, :, None, :]].any(axis=(2, 3))
    return m


def mask_gate(e, v, size, masks, level, csize):
    """the mask gate of every cell of view v: the cell centre's pixel at `level` inside the image and on the foreground of the mask at
    that level, if the view has one"""
    gw, gh = e.grid_dims(v)
    w, h = size[0] >> level, size[1] >> level
    cy, cx = np.divmod(np.arange(gw * gh), gw)
    px = np.floor(np.float32(csize * (2 * cx + 1) - 1) / np.float32(2) + np.float32(0.5)).astype(int)
    py = np.floor(np.float32(csize * (2 * cy + 1) - 1) / np.float32(2) + np.float32(0.5)).astype(int)
    ok = (px >= 0) & (px < w) & (py >= 0) & (py < h)
    if masks is not None and masks[v] is not None:
        m = mask_at(masks[v], size, level)
        assert m.shape == (h, w), f"the mask at level {level} is {m.shape}, the view {(h, w)}"
        ok &= m[np.clip(py, 0, h - 1), np.clip(px, 0, w - 1)]
    return ok


def random_yardstick(e, sc, lo, hi, K, seed, tilt, masks, sizes, level, csize, min_ncc=None):
    """-> (the records the chain keeps, in (view, cell) order; the number of cells the gate lets through)"""
    thr = np.float32(e.thresholds()[1] if min_ncc is None else min_ncc)
    kept, gated = [], 0
    for v in range(sc.nviews):
        gw, gh = e.grid_dims(v)
        n = gw * gh
        hyp = e.seed_random_hypotheses(v, np.arange(n), lo, hi, hypotheses=K, seed=seed, max_tilt=tilt, min_ncc=min_ncc)
        assert hyp.shape[0] == n * K, f"view {v}: {hyp.shape[0]} hypotheses for {n} cells of {K}"
        pre, _, flag = e.probe(engine.PROBE_PREPROCESS, hyp)
        _, ncc, _ = e.probe(engine.PROBE_NCC, pre)
        gate = mask_gate(e, v, view_sizes(sc, sizes)[v], masks, level, csize)
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


def strip(recs):
    r = recs.copy()
    r["id"] = 0
    r["flags"] = 0
    return r


def points_yardstick(e, pts, K, min_images, min_ncc=None):
    """-> (the records the chain keeps, in point order; the number of points that at least min_images views qualify for)"""
    thr = np.float32(e.thresholds()[1] if min_ncc is None else min_ncc)
    n = pts.shape[0]
    if n == 0:
        return np.zeros(0, e.dtype), 0
    hyp, count = e.seed_points_hypotheses(pts, hypotheses=K, min_ncc=min_ncc)
    assert hyp.shape[0] == n * K and count.shape[0] == n, f"{hyp.shape[0]} hypotheses and {count.shape[0]} counts for {n} points of {K}"
    _, views = e.seed_points_hypotheses(pts, hypotheses=e.cfg.nviews)
    denom = int((views >= min_images).sum())
    assert (count == np.minimum(views, K)).all(), f"counts {count} are not min(qualifying views {views}, {K})"
    slot = (np.arange(K)[None, :] < count[:, None]).ravel()
    assert not hyp[~slot].view(np.uint8).any(), "a slot behind count[i] is not zero bytes"
    idx = np.nonzero(slot)[0]
    if idx.size == 0:
        return np.zeros(0, e.dtype), denom
    p, _, f = e.probe(engine.PROBE_PREPROCESS, hyp[idx])
    _, s, _ = e.probe(engine.PROBE_NCC, p)
    pre = np.zeros(n * K, e.dtype)
    flag = np.ones(n * K, np.int32)
    ncc = np.full(n * K, np.nan, np.float32)
    pre[idx], flag[idx], ncc[idx] = p, f, s
    best = np.full(n, thr, np.float32)
    win = np.full(n, -1)
    for k in range(K):  # ascending k and a strict comparison: the lowest k among equals; a NaN never wins
        with np.errstate(invalid="ignore"):
            take = slot[k::K] & (flag[k::K] == 0) & (ncc[k::K] > best)
        best[take] = ncc[k::K][take]
        win[take] = k
    who = np.nonzero(win >= 0)[0]
    if who.size == 0:
        return np.zeros(0, e.dtype), denom
    first = who[0] * K + win[who[0]]
    batch = np.repeat(pre[first:first + 1], n)
    batch[who] = pre[who * K + win[who]]
    ref, _, _ = e.probe(engine.PROBE_REFINE, batch)
    post, _, pflag = e.probe(engine.PROBE_POSTPROCESS, ref)
    return post[who[pflag[who] == 0]], denom


def engine_with_pool(sc, ekw, masks, sizes, list_cap, seeds):
    """a pool of 2^16 records unless the case sizes its own: the default, four per cell, does not hold a seed in every cell plus what one
    iteration adds where a view is a crop or csize is 3"""
    e = engine.Engine(sc.nviews, list_cap=list_cap, enable_check=0, seed=3, **{"max_patches": 1 << 16, **ekw})
    e.set_scene(sc, masks=masks, sizes=sizes)
    if seeds is not None and seeds.shape[0]:
        e.upload_patches(seeds)
        e.propagate(0)
    return e


def lattice(sc, level, min_count=1):
    """the case's mvs_volume: 1.5 pixel footprints at the scene's radius of 4 (with the scene's focal: the largest where the views'
    differ, so the smallest footprint), around the scene's target"""
    focal = float(np.max(sc.meta.get("focal", 765.702941895 * sc.W / 640.0)))
    target = sc.meta.get("target", (0.0, 0.0, 0.0))
    foot = 4.0 / (focal / 2 ** level)
    voxel = 1.5 * foot
    origin = [target[c] + (-DIMS[c] / 2 + SHIFT[c]) * voxel for c in range(3)]
    return engine.make_volume(origin, voxel, DIMS, TRUNC_VOXELS * voxel, min_count)


def many_view_seeds(sc):
    """one seed per cell, exact to 2 % of a pixel footprint and half a degree (the left half of test_gpu_maps.test_many_views' seeds): the
    rough half of that test leaves pixels with no or one agreeing view, whose usability then rests on one pair, and every lattice point
    behind such a pixel would be left out (11 % of the reached points on the CPU oracle's pool)"""
    return synth.make_seeds(sc, 0, 2, stride=1, depth_noise=0.02, normal_noise_deg=0.5)


def grid_mesh(nx, ny, z=None):
    """nx x ny vertices at integer (x, y) and height z[y, x] (default 0), two counter-clockwise triangles a cell: normals towards +z"""
    y, x = np.mgrid[0:ny, 0:nx]
    zz = np.zeros((ny, nx)) if z is None else z
    verts = np.stack([x, y, zz], axis=-1).reshape(-1, 3).astype(np.float32)
    p = (y[:-1, :-1] * nx + x[:-1, :-1]).ravel()
    tris = np.concatenate([np.stack([p, p + 1, p + nx + 1], 1), np.stack([p, p + nx + 1, p + nx], 1)]).astype(np.int32)
    return verts, tris
