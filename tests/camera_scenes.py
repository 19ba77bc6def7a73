"""Scenes whose cameras leave the arc of synth.make_cameras (a helper module like scene_support.py): rolled about the optical axis,
with unequal intrinsics and distances per view, and in a world far from the origin.  Every family starts from the arc cameras (radius
4, elev 0.15, f0 = 765.702941895 * W / 640) and cycles its per-view tuples by view index:

  roll        R <- Rz(roll_v) R with rolls (0, 90, 180, 37) degrees: a patch's x-axis no longer runs along image rows
  intrinsics  fx_v = f0 * (1, 1.25, 0.85, 1.1), fy = 1.07 fx, skew 0.02 fx, principal point off centre by (0, 0), (9.5, -6.25),
              (-12, 4), (3, 3) pixels at W = 160 (scaled with W), camera distance x (1, 1.2, 0.85, 1.1)
  far         cameras, target and objects translated by T (default (300, -150, 500): |X| / depth of about 150)
  mixed       the roll and the intrinsics together, translated by T (default (12, -8, 16))

The third row of every P is (R_z, t_z) with K's last row (0, 0, 1): of unit norm in its first three entries, the precondition of
mvs_view_desc (include/mvskit_engine.h), asserted here to 2^-22 on the float32 matrices."""
import functools
import math

import numpy as np

from mvskit_amd import synth

FAMILIES = ("roll", "intrinsics", "far", "mixed")
ROLLS_DEG = (0.0, 90.0, 180.0, 37.0)
FX_FACTORS = (1.0, 1.25, 0.85, 1.1)
FY_OVER_FX, SKEW_OVER_FX = 1.07, 0.02
PP_OFFSETS = ((0.0, 0.0), (9.5, -6.25), (-12.0, 4.0), (3.0, 3.0))  # pixels at W = 160
DISTANCES = (1.0, 1.2, 0.85, 1.1)
T_FAR, T_NEAR = (300.0, -150.0, 500.0), (12.0, -8.0, 16.0)
# The float64 readings of the maps, the volume and the colours leave out what lies inside margins that grow with kappa
# (maps_reading.margins).  On the CPU oracle's pool at T_NEAR (kappa 5.7 and 7.0) they left out 4.2 % and 6.0 % of the volume's reached
# points and 5.5 % and 5.3 % of the caller's vertices on `far` and `mixed`, past the cases' cap of 5 %; at half of it (kappa 3.4 and
# 4.3) 2.2 % and 4.2 %, 2.9 % and 3.0 %.  The cap stays, the translation shrinks.
T_READING = (6.0, -4.0, 8.0)
RADIUS, ELEV = 4.0, 0.15
PORTRAIT = (98, 130)  # W < H: the roll family's second shape


def _f0(W):
    return 765.702941895 * W / 640.0


def _moved(objects, T):
    out = []
    for ob in objects:
        if isinstance(ob, synth.Plane):
            b = ob.bounds
            out.append(synth.Plane(ob.n, ob.d + float(np.dot(ob.n, T)), bounds=(b[0] + T[0], b[1] + T[0], b[2] + T[1], b[3] + T[1])))
        else:
            out.append(synth.Sphere(tuple(np.asarray(ob.c, dtype=np.float64) + T), ob.r))
    return out


def family_cameras(name, nviews, W, H, arc, T):
    """-> (P [n, 3, 4] float32, C [n, 3] float64, K [n, 3, 3] float64) of the family"""
    rolled = name in ("roll", "mixed")
    intr = name in ("intrinsics", "mixed")
    f0 = _f0(W)
    T = np.asarray(T, dtype=np.float64)
    P = np.zeros((nviews, 3, 4))
    C = np.zeros((nviews, 3))
    K = np.zeros((nviews, 3, 3))
    for v in range(nviews):
        k = v % 4
        a = 0.0 if nviews == 1 else math.radians(-arc / 2.0 + arc * v / (nviews - 1))
        c = RADIUS * np.array([math.sin(a), ELEV, math.cos(a)])
        fx, fy, skew, cx, cy = f0, f0, 0.0, W / 2.0, H / 2.0
        if intr:
            c = c * DISTANCES[k]
            fx = f0 * FX_FACTORS[k]
            fy, skew = FY_OVER_FX * fx, SKEW_OVER_FX * fx
            cx, cy = cx + PP_OFFSETS[k][0] * W / 160.0, cy + PP_OFFSETS[k][1] * W / 160.0
        c = c + T
        R, t = synth.look_at(c, T)
        if rolled:
            r = math.radians(ROLLS_DEG[k])
            Rz = np.array([[math.cos(r), -math.sin(r), 0.0], [math.sin(r), math.cos(r), 0.0], [0.0, 0.0, 1.0]])
            R, t = Rz @ R, Rz @ t
        K[v] = [[fx, skew, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]]
        P[v] = K[v] @ np.concatenate([R, t[:, None]], axis=1)
        C[v] = c
    return P.astype(np.float32), C, K


@functools.lru_cache(maxsize=None)
def family_scene(name, nviews, W, H, arc, kind, T=None):
    """the family's synth.Scene; meta["K"] holds the intrinsics the cameras were built from, meta["focal"] one number or, where the
    views' intrinsics differ, (fx + fy) / 2 per view; meta["target"] = T"""
    assert name in FAMILIES, name
    if T is None:
        T = {"far": T_FAR, "mixed": T_NEAR}.get(name, (0.0, 0.0, 0.0))
    P, C, K = family_cameras(name, nviews, W, H, arc, T)
    row = np.linalg.norm(P.astype(np.float64)[:, 2, :3], axis=1)
    assert (np.abs(row - 1.0) <= 2.0 ** -22).all(), f"{name}: |P[v, 2, :3]| = {row}"
    focal = (K[:, 0, 0] + K[:, 1, 1]) / 2.0 if name in ("intrinsics", "mixed") else _f0(W)
    sc = synth.make_scene(nviews=nviews, W=W, H=H, arc_deg=arc, radius=RADIUS, kind=kind, cameras=(P, C),
                          objects=_moved(synth.default_objects(kind), np.asarray(T, dtype=np.float64)), focal=focal, target=T)
    sc.meta["K"] = K
    sc.meta["family"] = name
    return sc


def reading_scene(name):
    """the family on 3 views of 96 x 64 of the plane, as the tests against a float64 reading take it: `far` and `mixed` at T_READING"""
    return family_scene(name, 3, 96, 64, 30.0, "plane", T_READING if name in ("far", "mixed") else None)


def portrait_roll_scene(nviews, arc, kind):
    """the roll family in a portrait image (W < H): a footprint turned by 90 degrees where the image is narrower than tall"""
    return family_scene("roll", nviews, PORTRAIT[0], PORTRAIT[1], arc, kind)


def kappa(sc):
    """how much larger the world's coordinates are than its depths: the largest |coordinate| over camera centres and surface points
    over the smallest true depth, never below 1.  Every float32 rounding of a projection P X is relative to |P[:, :3]| |X| + |P[:, 3]|
    while the result is compared relative to the depth: absolute errors grow by this factor."""
    big = float(np.abs(sc.centers).max())
    depth = np.inf
    for v in range(sc.nviews):
        X = sc.points[v].reshape(-1, 3).astype(np.float64)
        X = X[np.isfinite(X).all(axis=1)]
        if X.shape[0] == 0:
            continue
        big = max(big, float(np.abs(X).max()))
        P = sc.P[v].astype(np.float64)
        depth = min(depth, float((X @ P[2, :3] + P[2, 3]).min()))
    return max(1.0, big / depth)
