"""Scenes for the inputs synth.make_scene never produces (numpy only, no GPU; a helper module like mesh_reading.py).

patchwork_scene: a make_scene plane scene without noise whose views are repainted, as a function of the surface point (X, Y) of
every pixel (Scene.points), with regions a band-limited texture never gives -- exactly constant, saturated, striped, nearly flat,
one varying channel, flat in one view only -- so that all views stay consistent.  mixed_scale_scene: the views of one scene at
the scales 1, 1/2, 1/4, 1/8 (the oracle's own pyramid levels, P's rows 0 and 1 scaled alike), which drives Optim::getTex's level
pick (optim.cpp:799-811) through every value and both clamps.  wanted_level: that pick, unclamped, by the second reading."""
import functools

import numpy as np

import oracle_binding as ob
from mvskit_amd import synth
from test_oracle_second_reading import RefCam, ref_get_paxes, ref_project

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
    share, relisted for the scaled views by test_gpu_ragged_shapes._seeds_for_sizes' rule (a view is listed if the point projects at
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
    """test_gpu_ragged_shapes._seeds_for_sizes' rule over whole arrays (tens of thousands of seeds here)"""
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
