"""A float64 numpy reading of the dense maps (mvs_engine_render_maps / mvs_engine_fused_points): the cameras at a level, the
rendering of an id map, the agreement of the views with its margins (`unsure`), and the fusion on top of them.  numpy only, no GPU:
tests/test_gpu_maps.py holds the device to it, and mesh_reading.py and mesh_attr_reading.py build the TSDF and the colours on it."""
import numpy as np

DEPTH_TOL, NORMAL_COS = 0.004, 0.98
EDGE_PX, S_MARGIN, COS_MARGIN = 1e-3, 1e-5, 1e-5  # the margins where the world lies about as far from the origin as from the cameras
U = 2.0 ** -24  # float32 unit roundoff


def margins(kappa, W, H):
    """The margins of the float64 readings for a world whose coordinates are `kappa` times its depths (camera_scenes.kappa), images of
    W x H: dict(edge=pixels, s=, cos=), never below the module's defaults.
    edge: the device projects in float32, px = (P0 . X + p03) / (P2 . X + p23) + 0.5.  Each sum has four terms, three products and three
    additions: its error is at most 4 U of the sum of the terms' magnitudes.  For the numerator that sum is at most
    2 sqrt(3) (fx + |skew| + cx) |X|_inf (p03 = -P0 . C is as large as P0 . X), with fx + |skew| + cx <= (1.5 + 0.6) max(W, H) in the
    scenes of camera_scenes.py (fx <= 1.25 * 1.196 W, cx <= 0.575 W), and |X|_inf <= kappa w: 4 U * 7.3 kappa max(W, H) = 29 U kappa max(W, H) pixels after
    the division by w.  For the denominator it is 2 sqrt(3) |X|_inf: relative 4 U * 3.5 kappa = 14 U kappa, times |px| <= max(W, H).
    The division and the addition of 0.5 add 2 U max(W, H).  In all (29 + 14 + 2) U kappa max(W, H): c = 48 with the sum rounded up.
    s: s = n_q . (X0q - C) / n_q . (X - C).  Each difference rounds relative to |X|_inf, U kappa of the depth, each dot product of three
    terms adds 3 U kappa: 8 U kappa for the quotient; X itself comes from the rendering, about 30 float32 operations (the depth
    bound of tests/test_gpu_maps.py), 30 U kappa.  All of it over |cos(n_q, ray)| > 0.3, which the cases assert: 38 / 0.3 = 127,
    c = 128.  With kappa = 1 that is 7.6e-6, inside the default 1e-5.
    cos: n . n_q is a sum of three products of numbers both sides read exactly, 3 U |n| |n_q| = 1.8e-7 whatever the world's offset: the
    default stays."""
    return dict(edge=max(EDGE_PX, 48.0 * kappa * U * max(W, H)), s=max(S_MARGIN, 128.0 * kappa * U), cos=COS_MARGIN)


def cameras64(sc, level, sizes):
    """per view the float64 copies of the float32 camera at `level`: P, the inverse of its 3x3 block, the centre, oaxis, W, H"""
    cams = []
    for v in range(sc.nviews):
        P32 = np.ascontiguousarray(sc.P[v], dtype=np.float32)
        P = P32.astype(np.float64).copy()
        P[:2] /= 2.0 ** level
        cams.append(dict(P=P, Minv=np.linalg.inv(P[:, :3]), C=center64(P32), o=oaxis64(P32), W=sizes[v][0] >> level, H=sizes[v][1] >> level))
    return cams


def expected_ids(src, v, kind, csize, cam, mask):
    """the ids grid of depth_normal_map(v, kind) repeated over each cell's pixels, -1 on the mask's background"""
    grid = src.depth_normal_map(v, kind)[2]
    px = np.repeat(np.repeat(grid, csize, axis=0), csize, axis=1)[:cam["H"], :cam["W"]].copy()
    assert px.shape == (cam["H"], cam["W"]), f"the cells' pixels are {px.shape}, the view {(cam['H'], cam['W'])}"
    if mask is not None:
        px[~mask] = -1
    return px


def render64(pat, ids, cam):
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


def agree64(pat, ids, X, cams, v, tol, ncos, edge_px=EDGE_PX, s_margin=S_MARGIN, cos_margin=COS_MARGIN):
    """step 3 in float64 for view v -> (bits, unsure): uint64 maps, bit u of `unsure` = the pair (pixel, u) lies inside a margin (of
    edge_px pixels around a rounding boundary, s_margin around depth_tol, cos_margin around normal_cos: margins())"""
    bits, unsure = np.zeros(ids[v].shape, np.uint64), np.zeros(ids[v].shape, np.uint64)
    ok = ids[v] >= 0
    Xv = X[v][ok]
    n = pat["normal"][ids[v][ok]][:, :3].astype(np.float64)
    for u, cu in enumerate(cams):
        if u == v:
            continue
        h = Xv @ cu["P"][:, :3].T + cu["P"][:, 3]
        assert (h[:, 2] > 0.1).all(), f"view {u}: smallest w {h[:, 2].min()}"  # every point lies well in front of every camera in these scenes
        px, py = h[:, 0] / h[:, 2] + 0.5, h[:, 1] / h[:, 2] + 0.5
        edge = np.minimum(np.abs(px - np.rint(px)), np.abs(py - np.rint(py))) <= edge_px
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
            margin = edge | (met & ((np.abs(ds - tol) < s_margin) | ((np.abs(nn - ncos) < cos_margin) if ncos > -1 else False)))
        b, m = np.zeros(ids[v].shape, np.uint64), np.zeros(ids[v].shape, np.uint64)
        b[ok], m[ok] = bit.astype(np.uint64) << np.uint64(u), margin.astype(np.uint64) << np.uint64(u)
        bits |= b
        unsure |= m
    return bits, unsure


def render_agree64(pat, ids, cams, tol=DEPTH_TOL, ncos=NORMAL_COS, edge_px=EDGE_PX, s_margin=S_MARGIN, cos_margin=COS_MARGIN):
    """steps 2 and 3 over every view: render each id map, then agree each view against the others -> (bits, unsure), one map per view"""
    X = [render64(pat, ids[v], cams[v])[1] for v in range(len(cams))]
    bits, unsure = zip(*[agree64(pat, ids, X, cams, v, tol, ncos, edge_px, s_margin, cos_margin) for v in range(len(cams))])
    return bits, unsure


def popcount(a):
    return np.unpackbits(np.ascontiguousarray(a).view(np.uint8).reshape(a.shape + (8,)), axis=-1).sum(-1)


def fused64(ids, bits, unsure, min_consistent, dedupe):
    """step 4 over the reading -> per view the (emit, sure) masks"""
    out = []
    for v in range(len(ids)):
        emit = (ids[v] >= 0) & (popcount(bits[v]) >= min_consistent)
        if dedupe:
            emit &= (bits[v] & np.uint64((1 << v) - 1)) == 0
        out.append((emit, unsure[v] == 0))
    return out


def center64(P32):
    """the camera centre as the engine derives it from the level-0 projection: in double, in this order, rounded to float32"""
    P = P32.astype(np.float64)
    a, b, c, d, ee, f, g, h, i = P[0, 0], P[0, 1], P[0, 2], P[1, 0], P[1, 1], P[1, 2], P[2, 0], P[2, 1], P[2, 2]
    A, B, C = ee * i - f * h, -(d * i - f * g), d * h - ee * g
    det = a * A + b * B + c * C
    inv = [A, -(b * i - c * h), b * f - c * ee, B, a * i - c * g, -(a * f - c * d), C, -(a * h - b * g), a * ee - b * d]
    q = P[:, 3]
    return np.array([-(inv[3 * r] * q[0] + inv[3 * r + 1] * q[1] + inv[3 * r + 2] * q[2]) / det for r in range(3)]).astype(np.float32).astype(np.float64)


def oaxis64(P32):
    """the optical axis row as the engine holds it: the third row of the projection over the float32 norm of its first three entries
    (the engine's norm can differ from this one in the last bit: one unit roundoff on every term of the depth)"""
    r = P32[2].astype(np.float64)
    n = np.float32(np.sqrt(np.float32((r[:3] ** 2).sum())))
    return (P32[2] / n).astype(np.float32).astype(np.float64)
