"""Scenes for the inputs synth.make_scene never produces (numpy only, no GPU; a helper module like mesh_reading.py).

patchwork_scene: a make_scene plane scene without noise whose views are repainted, as a function of the surface point (X, Y) of
every pixel (Scene.points), with regions a band-limited texture never gives -- exactly constant, saturated, striped, nearly flat,
one varying channel, flat in one view only -- so that all views stay consistent.  mixed_scale_scene: the views of one scene at
the scales 1, 1/2, 1/4, 1/8 (the oracle's own pyramid levels, P's rows 0 and 1 scaled alike), which drives Optim::getTex's level
pick (optim.cpp:799-811) through every value and both clamps.  wanted_level: that pick, unclamped, by the second reading.

The last section holds what tests/test_edge_scenes.py (CPU), tests/test_gpu_photometric_edges.py (GPU) and
tests/golden/make_edge_reading.py share: the groups of seeds, the level table, the recorded second reading and its bound."""
import functools
import os

import numpy as np

import oracle_binding as ob
from mvskit_amd import synth
from second_reading import RefCam, ref_compute_incc, ref_cost_func, ref_get_paxes, ref_project

F = np.float32

TEXTURED, CONST, SATURATED, STRIPES, RAMP, RED_ONLY, FLAT_ONE_VIEW, BLACK = range(8)
CLASS_NAMES = {TEXTURED: "textured", CONST: "a", SATURATED: "b", STRIPES: "c", RAMP: "d", RED_ONLY: "e", FLAT_ONE_VIEW: "f", BLACK: "a0"}
#: the classes whose windows have a variance far from zero in every view: what a float32 restatement in another order can be held to
WELL_CONDITIONED = (TEXTURED, SATURATED, STRIPES, RED_ONLY)
FLAT_VIEW = 1       # the view class (f) is flat in
TILE = 0.62         # world units: 47 pixels of a 256-wide view at radius 4, 45 under the foreshortening of the outer views
#: rows (Y) x columns (X) of tiles centred on the origin; everything outside stays textured
LAYOUT = ((CONST, STRIPES, SATURATED),
          (BLACK, FLAT_ONE_VIEW, TEXTURED),
          (RAMP, TEXTURED, RED_ONLY))


def _classes(X, Y):
    """class of every surface point"""
    cls = np.zeros(X.shape, np.int8)
    ix = np.floor(X / TILE + 1.5).astype(int)
    iy = np.floor(Y / TILE + 1.5).astype(int)
    with np.errstate(invalid="ignore"):
        inside = (ix >= 0) & (ix < 3) & (iy >= 0) & (iy < 3) & np.isfinite(X) & np.isfinite(Y)
    lay = np.asarray(LAYOUT, np.int8)
    cls[inside] = lay[iy[inside], ix[inside]]
    return cls


def patchwork_scene(nviews=4, W=256, H=192, arc_deg=30.0, kind="plane", noise_sigma=2.0, tex_seed=12345, flat_sphere=False):
    """-> (scene, classes): classes[v] is the H x W int8 class of every pixel of view v (TEXTURED .. FLAT_ONE_VIEW).

    (a) CONST: 200 in every channel.  A bilinear blend of four equal texels in float32 (image.cpp:452-470) is NOT that texel again
    -- the four weights are rounded products and their sum is not 1 -- so a window of this class has an ssd of about 1e-9, not 0, and
    1 / msd of about 2e5; (a0) BLACK: 0 in every channel, the one value whose blend is exact, so ssd == 0 and msd -> 1 in every view.
    (b) SATURATED: bars of 255 and 0, 5 pixels of X each, so that every 7x7 window holds a step edge.  (c) STRIPES: a sinusoid in X
    with a period of 6 pixels, the same in every channel.  (d) RAMP: one grey level per 8 pixels of X.  (e) RED_ONLY: the texture's
    red channel, green and blue 90.  (f) FLAT_ONE_VIEW: 150 in view FLAT_VIEW, the texture elsewhere.  Sensor noise (make_scene's own
    draw) is added only where the texture is left.  flat_sphere (kind "multi"): no tiles; every pixel that sees the sphere is 200."""
    sc = synth.make_scene(nviews=nviews, W=W, H=H, arc_deg=arc_deg, radius=4.0, kind=kind, noise_sigma=0.0, tex_seed=tex_seed)
    px = sc.meta["radius"] / sc.meta["focal"]  # world units per pixel at the scene's distance
    classes = np.zeros((nviews, H, W), np.int8)
    for v in range(nviews):
        X, Y, Z = (sc.points[v][..., k].astype(np.float64) for k in range(3))
        img = sc.images[v]
        if flat_sphere:
            with np.errstate(invalid="ignore"):  # default_objects' sphere: centre (0, 0, 0.55), radius 0.5
                cls = np.where(np.abs(np.sqrt(X * X + Y * Y + (Z - 0.55) ** 2) - 0.5) < 1e-3, CONST, TEXTURED).astype(np.int8)
            img[cls == CONST] = 200
        else:
            cls = _classes(X, Y)
            img[cls == CONST] = 200
            m = cls == SATURATED
            img[m] = np.where(np.floor(X[m] / (5.0 * px)).astype(int) % 2 == 0, 255, 0)[:, None]
            img[cls == BLACK] = 0
            m = cls == STRIPES
            img[m] = np.rint(128.0 + 100.0 * np.sin(2.0 * np.pi * X[m] / (6.0 * px)))[:, None]
            m = cls == RAMP
            img[m] = (100.0 + np.floor(X[m] / (8.0 * px) + 1e-9))[:, None]
            m = cls == RED_ONLY
            img[m, 1:] = 90
            if v == FLAT_VIEW:
                img[cls == FLAT_ONE_VIEW] = 150
        classes[v] = cls
        noisy = (cls == TEXTURED) | ((cls == FLAT_ONE_VIEW) & (v != FLAT_VIEW))
        if noise_sigma > 0:
            nz = np.random.RandomState(tex_seed + 1000 + v).normal(0.0, noise_sigma, size=img.shape)
            img[noisy] = np.clip(np.rint(img[noisy].astype(np.float64) + nz[noisy]), 0, 255).astype(np.uint8)
    return sc, classes


def seed_classes(sc, classes, seeds, half=5, sizes=None):
    """class of every seed: the class that fills the (2 half + 1)^2 pixels around its projection in EVERY listed view (so that
    whole 7x7 windows, one pixel per sample plus the bilinear tap and the rounding, lie inside it), -1 where they do not agree."""
    out = np.full(seeds.shape[0], -1, np.int64)
    P = sc.P.astype(np.float64)
    X = seeds["coord"].astype(np.float64)
    ok = np.ones(seeds.shape[0], bool)
    for k in range(int(seeds["nimages"].max())):
        for v in range(sc.nviews):
            sel = (k < seeds["nimages"]) & (seeds["images"][:, k] == v)
            if not sel.any():
                continue
            w, h = (sc.W, sc.H) if sizes is None else sizes[v]
            x = X[sel] @ P[v].T
            u, t = np.rint(x[:, 0] / x[:, 2]).astype(int), np.rint(x[:, 1] / x[:, 2]).astype(int)
            inside = (u - half >= 0) & (u + half < w) & (t - half >= 0) & (t + half < h)
            u, t = np.clip(u, half, w - 1 - half), np.clip(t, half, h - 1 - half)
            lo = np.full(u.shape, 127, np.int64)
            hi = np.full(u.shape, -1, np.int64)
            for dy in (-half, 0, half):
                for dx in (-half, 0, half):  # the regions are axis-aligned in X, Y and convex in every view: nine taps of the box decide
                    c = classes[v][t + dy, u + dx]
                    lo, hi = np.minimum(lo, c), np.maximum(hi, c)
            rows = np.nonzero(sel)[0]
            ok[rows] &= inside & (lo == hi)
            if k == 0:
                out[rows] = lo
            else:
                ok[rows] &= out[rows] == lo
    out[~ok] = -1
    return out


# ------------------------------------------------------------------ views of mixed scale
def mixed_scale_scene(scales=(0, 1, 2, 3), W=512, H=384, arc_deg=30.0, kind="plane", level=0, csize=2, stride=2, seed=5):
    """-> (scene, sizes, seeds, base): view v of `scene` is pyramid level scales[v] of view v of the full-size scene `base` as the
    oracle builds it (Image::buildImagePyramid), top-left in an H x W array; sizes[v] = (W >> k, H >> k); rows 0 and 1 of P[v] are
    scaled by 2^-k (Camera::updateProjection's own rule).  seeds: make_seeds of `base`, every view the reference view of its own
    share, relisted for the scaled views by parity_support.seeds_for_sizes' rule (a view is listed if the point projects at
    least 8 pixels inside its own image; a seed whose reference view is not is dropped).

    A 64 x 48 view is accepted at working level 1 as well (mvs_engine_set_views refuses level-0 sizes below 8 only; the levels
    below it, down to 8 x 6 at level 3, only ever reject windows), so no view has to be dropped there."""
    n = len(scales)
    base = synth.make_scene(nviews=n, W=W, H=H, arc_deg=arc_deg, radius=4.0, kind=kind)
    o = ob.Oracle(n, level=max(0, max(scales) - 2), csize=2, wsize=7, minImageNum=2, schedule=ob.SCHEDULE_ENGINE, sum_mode=ob.SUM_SEQ, nthreads=1)
    o.set_scene(base)
    images = np.zeros_like(base.images)
    P = base.P.copy()
    sizes = []
    for v, k in enumerate(scales):
        img = base.images[v] if k == 0 else o.pyramid(v, k)
        assert img.shape == (H >> k, W >> k, 3)
        images[v, : H >> k, : W >> k] = img
        P[v, :2] = (P[v, :2] / F(1 << k)).astype(F)
        sizes.append((W >> k, H >> k))
    o.close()
    sc = synth.Scene(W=W, H=H, P=P, images=images, centers=base.centers, points=None, normals=None, meta=dict(base.meta, scales=tuple(scales)))
    seeds = synth.make_seeds(base, level=level, csize=csize, stride=stride, seed=seed)
    return sc, sizes, seeds_for_sizes(sc, seeds, sizes), base


def seeds_for_sizes(sc, seeds, sizes):
    """parity_support.seeds_for_sizes' rule over whole arrays (tens of thousands of seeds here)"""
    P = sc.P.astype(np.float64)
    X = seeds["coord"].astype(np.float64)
    out = seeds.copy()
    out["images"][:] = 0
    cnt = np.zeros(seeds.shape[0], np.int64)
    alive = np.ones(seeds.shape[0], bool)
    rows = np.arange(seeds.shape[0])
    for k in range(int(seeds["nimages"].max())):
        v = seeds["images"][:, k].astype(np.int64)
        listed = k < seeds["nimages"]
        x = np.einsum("nij,nj->ni", P[v], X)
        with np.errstate(divide="ignore", invalid="ignore"):
            u, w = x[:, 0] / x[:, 2], x[:, 1] / x[:, 2]
        sw = np.array([sizes[i][0] for i in range(sc.nviews)])[v]
        sh = np.array([sizes[i][1] for i in range(sc.nviews)])[v]
        keep = listed & (x[:, 2] > 0) & (u >= 8) & (u < sw - 8) & (w >= 8) & (w < sh - 8)
        if k == 0:
            alive &= keep
        sel = keep & alive
        out["images"][rows[sel], cnt[sel]] = v[sel]
        cnt[sel] += 1
    out["nimages"] = cnt
    out = out[alive & (cnt >= 2)]
    out["id"] = np.arange(out.shape[0])
    return np.ascontiguousarray(out)


def ratio_of(cams, seed, view, level):
    """Optim::getTex's ratio (optim.cpp:799-807) of `seed` in `view`, by the second reading: the mean length, in pixels of `view`
    at `level`, of the reference view's two patch axes."""
    X, N = seed["coord"].astype(F), seed["normal"].astype(F)
    px, py = ref_get_paxes(cams[int(seed["images"][0])], X, N, level)
    Pv = cams[int(view)].P[level]
    c = ref_project(Pv, X)
    dx = (ref_project(Pv, (X + px).astype(F)) - c).astype(F)
    dy = (ref_project(Pv, (X + py).astype(F)) - c).astype(F)
    return float((np.linalg.norm(dx).astype(F) + np.linalg.norm(dy).astype(F)) / F(2))


def wanted_level(cams, seed, view, level):
    """The unclamped floor(log2(ratio) + .5) of optim.cpp:808 (the reference then clamps it to [-level, 2])."""
    return int(np.floor(np.log(ratio_of(cams, seed, view, level)) / np.log(2.0) + 0.5))


def near_level_threshold(ratio, rel=1e-3):
    """is `ratio` within `rel` (relative) of a threshold 2^(k - .5) of the level pick"""
    t = 2.0 ** (np.floor(np.log2(ratio) + 0.5) - 0.5)  # the threshold just below ...
    return min(abs(ratio - t) / t, abs(ratio - 2.0 * t) / (2.0 * t)) < rel  # ... and the one above


def hostile_records(sc, ref=0, other=1):
    """Finite records no scene produces, each listed as [ref, other]: a point behind the reference camera, a point 1e4 units away,
    a normal facing away from the cameras, a normal perpendicular to the reference view's ray, and a normal within 1e-4 of the
    reference camera's x axis (Optim::getPAxes crosses the normal with that axis, optim.cpp:71-74)."""
    cam = RefCam(sc.P[ref], 0)
    C0 = cam.center[:3].astype(np.float64)
    z = cam.zaxis.astype(np.float64)
    xa = cam.xaxis.astype(np.float64) / np.linalg.norm(cam.xaxis.astype(np.float64))
    ray = -C0 / np.linalg.norm(C0)  # towards the origin, where the plane is
    perp = np.cross(ray, [0.0, 1.0, 0.0])
    perp /= np.linalg.norm(perp)
    tilt = xa + 1e-4 * z
    tilt /= np.linalg.norm(tilt)
    cases = [(C0 - 2.0 * z, (0.0, 0.0, 1.0)),          # behind the reference camera
             (C0 + 1e4 * ray, (0.0, 0.0, 1.0)),        # 1e4 units away
             ((0.0, 0.0, 0.0), (0.0, 0.0, -1.0)),      # the normal faces away
             ((0.1, 0.05, 0.0), tuple(perp)),          # perpendicular to the ray
             ((0.1, 0.05, 0.0), tuple(tilt)),          # 1e-4 off the camera's x axis
             ((0.1, 0.05, 0.0), tuple(-tilt))]
    recs = np.zeros(len(cases), dtype=synth.PATCH_DTYPE)
    for i, (X, N) in enumerate(cases):
        recs["coord"][i] = (X[0], X[1], X[2], 1.0)
        recs["normal"][i, :3] = N
    recs["ncc"] = -1.0
    recs["flags"] = 1
    recs["nimages"] = 2
    recs["images"][:, 0] = ref
    recs["images"][:, 1] = other
    recs["dscale"] = 0.01
    recs["ascale"] = 0.1
    recs["id"] = np.arange(len(cases))
    return recs


def border_seeds(sc, sizes, ref, target, n_along=40, depth=14.0):
    """Patches on the plane z = 0 whose centres walk across the first and the last `depth` pixels of the columns of view `target`
    (its own, scaled pixels) in steps of depth / n_along, listed as [ref, target]: in and out of the window test of `target` at
    whatever level it is sampled at (test_gpu_ragged_shapes._border_seeds, for views with their own sizes)."""
    P = sc.P.astype(np.float64)
    M = P[target][:, :3]
    C = sc.centers[target]
    w, h = sizes[target]
    uv = []
    for k, t in enumerate(np.linspace(0.0, depth, n_along)):
        y = 0.25 * h + (k * 37) % max(1, h // 2)
        uv.append((t, y))
        uv.append((w - 1.0 - t, y))
    recs = np.zeros(len(uv), dtype=synth.PATCH_DTYPE)
    for i, (u, v) in enumerate(uv):
        d = np.linalg.solve(M, np.array([u, v, 1.0]))
        X = C + (-C[2] / d[2]) * d
        recs["coord"][i] = (X[0], X[1], 0.0, 1.0)
    recs["normal"][:, 2] = 1.0
    recs["ncc"] = -1.0
    recs["flags"] = 1
    recs["nimages"] = 2
    recs["images"][:, 0] = ref
    recs["images"][:, 1] = target
    recs["id"] = np.arange(len(uv))
    return recs


# ------------------------------------------------------------------ what the tests share (built once per process, never written to)
MIXED_SCALES = (3, 2, 1, 0, 3)  # 1/8, 1/4, 1/2, 1 and a second 1/8 at the other end of the arc: a pair of equal scale for a wanted level of 0


@functools.lru_cache(maxsize=None)
def patchwork(stride=1, seed=5):
    """-> (scene, classes, seeds, class of every seed) of the default patchwork scene; one seed per `stride`^2 cells of every view"""
    sc, classes = patchwork_scene()
    seeds = synth.make_seeds(sc, stride=stride, seed=seed)
    return sc, classes, seeds, seed_classes(sc, classes, seeds)


def class_seeds(cls, count=240):
    """`count` seeds of class `cls`, spread evenly over the class (all of them if it has fewer)"""
    _, _, seeds, k = patchwork()
    s = seeds[k == cls]
    return s if s.shape[0] <= count else s[np.linspace(0, s.shape[0] - 1, count).astype(int)]


@functools.lru_cache(maxsize=None)
def mixed(level):
    """-> (scene, sizes, grid seeds, border seeds) of the mixed-scale scene for working level `level`: the grid seeds are what the
    loop may be fed (every listed view sees the point 8 pixels inside its image), the border seeds go through the probes only"""
    sc, sizes, seeds, _ = mixed_scale_scene(scales=MIXED_SCALES, level=level, stride=8 >> level)
    n = sc.nviews
    border = np.concatenate([border_seeds(sc, sizes, r, t) for r in range(n) for t in range(n) if r != t])
    border["id"] = np.arange(border.shape[0])
    return sc, sizes, seeds, border


# ------------------------------------------------------------------ what the tests of the scenes share
COS_THR = F(np.cos(F(60.0 * np.pi / 180.0)))
SECOND_READING_BOUND = 4 * 5.59e-5  # times max(1, |expected|): four times the worst of WORST_MEASURED
#: worst |oracle - second reading| when the bound was set: (computeINCC plain, computeINCC robust, cost_func) per group
WORST_MEASURED = {"textured": (9.8e-6, 8.0e-6, 8.2e-6), "b": (5.59e-5, 2.4e-5, 2.4e-5), "c": (1.4e-5, 1.1e-5, 1.1e-5), "e": (8.6e-6, 7.6e-6, 7.9e-6),
                  "mixed scale, level 0": (5.22e-5, 1.4e-5, 1.3e-5), "mixed scale, level 1": (2.4e-5, 5.8e-6, 5.3e-6)}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "edge_second_reading.npz")
GROUPS = list(WELL_CONDITIONED) + [("mixed", 0), ("mixed", 1)]
CLASS_SEEDS = 600  # seeds per well-conditioned class; the mixed-scale groups take every grid and border seed


def oracle_for(sc, level=0, sizes=None, wsize=7, **kw):
    o = ob.Oracle(sc.nviews, level=level, csize=2, wsize=wsize, minImageNum=2, schedule=ob.SCHEDULE_ENGINE, sum_mode=ob.SUM_TREE64, nthreads=8, **kw)
    o.set_scene(sc, sizes=sizes)
    return o


def windows(o, s):
    """raw textures of every listed view of seed s -> [(view, flag, tex)]"""
    X, N = s["coord"], s["normal"]
    px, py = o.get_paxes(int(s["images"][0]), X, N)
    return [(int(v),) + o.get_tex(X, px, py, N, int(v)) for v in s["images"][: s["nimages"]]]


@functools.lru_cache(maxsize=None)
def level_table(level):
    """Every (seed, non-reference view) pair of the mixed-scale seeds (grid, then border) -> a structured array: seed (index into
    the concatenation), view, wanted (unclamped level difference), ratio, ref_ok / ok (the oracle's window test of the reference
    view / of the view), and per seed the oracle's preProcess flag."""
    sc, sizes, grid, border = mixed(level)
    seeds = np.concatenate([grid, border])
    o = oracle_for(sc, level, sizes)
    cams = [RefCam(sc.P[v], level) for v in range(sc.nviews)]
    rows = []
    flags = np.zeros(seeds.shape[0], np.int32)
    for i, s in enumerate(seeds):
        w = windows(o, s)
        for v, flag, _ in w[1:]:
            r = ratio_of(cams, s, v, level)
            rows.append((i, v, int(np.floor(np.log(r) / np.log(2.0) + 0.5)), r, w[0][1] == 0, flag == 0))
        flags[i] = o.preprocess(s)[0]
    o.close()
    tab = np.array(rows, dtype=[("seed", "i4"), ("view", "i4"), ("wanted", "i4"), ("ratio", "f8"), ("ref_ok", "?"), ("ok", "?")])
    return seeds, tab, flags


def level_counts(tab, level):
    """-> {name: (accepted, rejected while the reference view passes)} per unclamped value and per clamp reached at `level`"""
    groups = {"0": tab["wanted"] == 0, "+1": tab["wanted"] == 1, "+2": tab["wanted"] == 2, "upper clamp (>= 3)": tab["wanted"] >= 3}
    if level == 0:
        groups["lower clamp (<= -1 at level 0)"] = tab["wanted"] <= -1
    else:
        groups["-1"] = tab["wanted"] == -1
    return {k: (int((m & tab["ok"]).sum()), int((m & tab["ref_ok"] & ~tab["ok"]).sum())) for k, m in groups.items()}


def group_name(g):
    return f"mixed scale, level {g[1]}" if isinstance(g, tuple) else "class " + CLASS_NAMES[g]


def group_seeds(group):
    """-> (scene, level, sizes, seeds): ("mixed", level): ALL grid and border seeds of that level; a class: CLASS_SEEDS seeds of it"""
    if isinstance(group, tuple):
        sc, sizes, grid, border = mixed(group[1])
        return sc, group[1], sizes, np.concatenate([grid, border])
    return patchwork()[0], 0, None, class_seeds(group, CLASS_SEEDS)


def compute_reading(group, which=None):
    """The second reading and the oracle over the seeds `which` (indexes; default all) of a group -> dict of arrays, one row per seed:
    near (pairs within 1e-3 of a level threshold; such a seed is left out), pairs, incc / oracle_incc (n x 2: computeINCC plain and
    robust), kept (the oracle's preProcess keeps it and its kept pairs are not near a threshold), recs (preProcess' output), x
    (encode of it), cost / oracle_cost (cost_func at x); NaN where a value does not apply.  The reading's side (incc, cost) is what
    tests/golden/make_edge_reading.py records: numpy over 49 samples per view takes minutes for the full sets."""
    sc, level, sizes, seeds = group_seeds(group)
    which = np.arange(seeds.shape[0]) if which is None else np.asarray(which)
    o = oracle_for(sc, level, sizes)
    cams = [RefCam(sc.P[v], level) for v in range(sc.nviews)]
    pyrs = [[o.pyramid(v, l) for l in range(level + 3)] for v in range(sc.nviews)]
    tau = min(2 * 2, sc.nviews)  # m_tau, pmmvps.cpp:32
    near = lambda s, idx: sum(bool(near_level_threshold(ratio_of(cams, s, v, level))) for v in idx[1:])
    n = which.shape[0]
    out = dict(near=np.zeros(n, np.int64), pairs=np.zeros(n, np.int64), incc=np.full((n, 2), np.nan), oracle_incc=np.full((n, 2), np.nan),
               kept=np.zeros(n, bool), recs=np.zeros(n, ob.PATCH_DTYPE), x=np.full((n, 3), np.nan), cost=np.full(n, np.nan),
               oracle_cost=np.full(n, np.nan))
    for j, s in enumerate(seeds[which]):
        idx = [int(i) for i in s["images"][: s["nimages"]]]
        out["pairs"][j] = len(idx) - 1
        out["near"][j] = near(s, idx)
        if out["near"][j]:
            continue
        X, N = s["coord"].astype(F), s["normal"].astype(F)
        for robust in (0, 1):
            out["oracle_incc"][j, robust] = o.compute_incc(s, robust=robust)
            out["incc"][j, robust] = ref_compute_incc(cams, pyrs, X, N, idx, level, 7, tau, robust, COS_THR)
        f, rec = o.preprocess(s)
        if f != 0:
            continue
        idx = [int(i) for i in rec["images"][: rec["nimages"]]]
        if near(rec, idx):
            continue
        Xr = rec["coord"].astype(F)
        ray = (Xr - cams[idx[0]].center).astype(F)
        ray = (ray / np.linalg.norm(ray).astype(F)).astype(F)
        x = o.encode(rec)
        out["kept"][j], out["recs"][j], out["x"][j] = True, rec, x
        out["oracle_cost"][j] = o.cost(rec, x)
        out["cost"][j] = ref_cost_func(cams, pyrs, Xr, ray, rec["dscale"], idx, x, level, 7, tau, 2, COS_THR)
    o.close()
    return out


@functools.lru_cache(maxsize=None)
def second_reading(group):
    """What tests/test_gpu_photometric_edges.py shares: the group's seeds that are compared (none of their pairs near a threshold),
    the recorded reading of them (incc n x 2), the records preProcess keeps of them and the recorded reading's cost of those."""
    sc, level, sizes, seeds = group_seeds(group)
    with np.load(GOLDEN) as z:
        incc, cost = z[group_name(group) + "/incc"], z[group_name(group) + "/cost"]
    assert incc.shape == (seeds.shape[0], 2) and cost.shape == (seeds.shape[0],), "tests/golden/make_edge_reading.py has to be run again"
    used, kept = ~np.isnan(incc[:, 0]), ~np.isnan(cost)
    o = oracle_for(sc, level, sizes)
    pre = [o.preprocess(s) for s in seeds[kept]]
    o.close()
    assert all(f == 0 for f, _ in pre), f"preProcess flags {[f for f, _ in pre if f != 0]} among the kept seeds"
    return dict(seeds=seeds[used], incc=incc[used], recs=np.array([r for _, r in pre], dtype=ob.PATCH_DTYPE), cost=cost[kept])


def within_bound(got, exp):
    """-> (all within SECOND_READING_BOUND * max(1, |exp|), the worst absolute deviation)"""
    got, exp = np.asarray(got, np.float64), np.asarray(exp, np.float64)
    d = np.abs(got - exp)
    return bool((d <= SECOND_READING_BOUND * np.maximum(1.0, np.abs(exp))).all()), float(d.max()) if d.size else 0.0
