"""A numpy reading of the mesh render (include/mvskit_engine.h: mvs_engine_mesh_render, mvs_engine_mesh_visibility): the coverage in
int64, the depth as the contract's fp64 chain, the z-buffer as a minimum of 64-bit keys, vectorised over (triangle, pixel of its clipped
box) pairs.  It works from its own float64 projection (project64) or from a given (screen, vdepth) -- the device's own, which leaves
nothing but integer arithmetic and IEEE fp64 between the two, so the yardstick is equality of bytes.  numpy only, no GPU."""
import numpy as np

LIMIT = 1 << 24  # |sx|, |sy| of a usable vertex, in 1/256 pixel
U = 2.0 ** -24   # float32 unit roundoff
PAIRS = 1 << 21  # (triangle, pixel) pairs a pass


def camera64(P32, level):
    """the float64 copy of the float32 camera at `level`"""
    P = np.ascontiguousarray(P32, dtype=np.float32).astype(np.float64).copy()
    P[:2] /= 2.0 ** level
    return P


def project64(P, verts):
    """the contract's VERTEX step in float64: (screen [n, 2] int64 = rint(256 x), rint(256 y), half to even; d [n] float64, not rounded
    to float32; xy [n, 2] the unsnapped position; mag [n] the summed magnitudes of the four terms of d)"""
    X = np.asarray(verts, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):  # a vertex may be NaN or infinite: so is what comes of it
        r = X @ P[:, :3].T + P[:, 3]
        xy = r[:, :2] / r[:, 2:3]
        mag = np.abs(X * P[2, :3]).sum(axis=1) + abs(P[2, 3])
    with np.errstate(invalid="ignore"):
        screen = np.rint(np.clip(np.nan_to_num(xy, nan=2.0 ** 31, posinf=2.0 ** 31, neginf=-2.0 ** 31), -2.0 ** 31, 2.0 ** 31) * 256.0).astype(np.int64)
    return screen, r[:, 2], xy, mag


def usable(screen, vdepth):
    s = np.asarray(screen, dtype=np.int64)
    d = np.asarray(vdepth)
    with np.errstate(invalid="ignore"):
        return (d > 0) & np.isfinite(d) & (np.abs(s) <= LIMIT).all(axis=1)


def boxes(screen, tris, W, H):
    """per triangle the pixels of its bounding box clipped to the image: (x0, y0, x1, y1), empty where x1 < x0 or y1 < y0"""
    s = np.asarray(screen, dtype=np.int64)[np.asarray(tris, dtype=np.int64)]  # [m, 3, 2]
    lo, hi = s.min(axis=1), s.max(axis=1)
    x0, y0 = np.maximum(0, (lo[:, 0] + 255) >> 8), np.maximum(0, (lo[:, 1] + 255) >> 8)
    x1, y1 = np.minimum(W - 1, hi[:, 0] >> 8), np.minimum(H - 1, hi[:, 1] >> 8)
    return x0, y0, x1, y1


def render(screen, vdepth, tris, W, H):
    """-> dict(depth [H, W] float32 (NaN: empty), tri [H, W] int32 (-1), covered, skipped, count [H, W] int64: the triangles that
    cover each pixel, keys [H, W] uint64).  vdepth is used as it comes: float32 from the device, float64 from project64."""
    s = np.asarray(screen, dtype=np.int64).reshape(-1, 2)
    d = np.asarray(vdepth).reshape(-1)
    t = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    keys = np.full(W * H, np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64)
    count = np.zeros(W * H, np.int64)
    ok = usable(s, d)
    live = ok[t].all(axis=1) if t.shape[0] else np.zeros(0, bool)
    skipped = int((~live).sum())
    rows = np.flatnonzero(live)
    t = t[rows]
    p = s[t]  # [m, 3, 2]
    area = (p[:, 1, 0] - p[:, 0, 0]) * (p[:, 2, 1] - p[:, 0, 1]) - (p[:, 1, 1] - p[:, 0, 1]) * (p[:, 2, 0] - p[:, 0, 0])
    flip = area < 0
    t[flip] = t[flip][:, [0, 2, 1]]
    p = s[t]
    area = np.abs(area)
    x0, y0, x1, y1 = boxes(s, t, W, H)
    keep = (area != 0) & (x1 >= x0) & (y1 >= y0)
    rows, t, p, area, x0, y0, x1, y1 = rows[keep], t[keep], p[keep], area[keep], x0[keep], y0[keep], x1[keep], y1[keep]
    bw, n = x1 - x0 + 1, (x1 - x0 + 1) * (y1 - y0 + 1)
    with np.errstate(divide="ignore"):
        w = 1.0 / d[t].astype(np.float64)  # [m, 3]
    start = 0
    while start < rows.shape[0]:
        stop = start + max(1, int(np.searchsorted(np.cumsum(n[start:]), PAIRS, side="right")))
        sl = slice(start, stop)
        start = stop
        k = np.repeat(np.arange(n[sl].shape[0]), n[sl])  # the pair's triangle, within the pass
        j = np.arange(k.shape[0]) - np.repeat(np.cumsum(n[sl]) - n[sl], n[sl])  # its pixel within the box
        px, py = x0[sl][k] + j % bw[sl][k], y0[sl][k] + j // bw[sl][k]
        qx, qy = 256 * px, 256 * py
        pk = p[sl][k]
        inside = np.ones(k.shape[0], bool)
        E = []
        for a, b in ((1, 2), (2, 0), (0, 1)):  # the edge opposite vertex 0, 1, 2
            dx, dy = pk[:, b, 0] - pk[:, a, 0], pk[:, b, 1] - pk[:, a, 1]
            e = dx * (qy - pk[:, a, 1]) - dy * (qx - pk[:, a, 0])
            inside &= (e > 0) | ((e == 0) & ((dy < 0) | ((dy == 0) & (dx > 0))))
            E.append(e)
        k, px, py = k[inside], px[inside], py[inside]
        E = [e[inside].astype(np.float64) for e in E]
        wk = w[sl][k]
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            inv = ((E[0] * wk[:, 0] + E[1] * wk[:, 1]) + E[2] * wk[:, 2]) / area[sl][k].astype(np.float64)
            depth = (1.0 / inv).astype(np.float32)
        pix = py * W + px
        np.add.at(count, pix, 1)
        fin = np.isfinite(depth)
        key = depth[fin].view(np.uint32).astype(np.uint64) << np.uint64(32) | rows[sl][k[fin]].astype(np.uint64)
        np.minimum.at(keys, pix[fin], key)
    have = keys != np.uint64(0xFFFFFFFFFFFFFFFF)
    depth = np.where(have, (keys >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(np.nan)).astype(np.float32)
    tri = np.where(have, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    return dict(depth=depth.reshape(H, W), tri=tri.reshape(H, W), covered=int(have.sum()), skipped=skipped, count=count.reshape(H, W),
                keys=keys.reshape(H, W))


def listed(screen, vdepth, tris, W, H, small_max=32):
    """the triangles that the device hands to the wave-per-triangle kernel: usable, with an area, a clipped box of more than small_max pixels"""
    s = np.asarray(screen, dtype=np.int64).reshape(-1, 2)
    t = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    if t.shape[0] == 0:
        return 0
    p = s[t]
    area = (p[:, 1, 0] - p[:, 0, 0]) * (p[:, 2, 1] - p[:, 0, 1]) - (p[:, 1, 1] - p[:, 0, 1]) * (p[:, 2, 0] - p[:, 0, 0])
    x0, y0, x1, y1 = boxes(s, t, W, H)
    n = np.maximum(x1 - x0 + 1, 0) * np.maximum(y1 - y0 + 1, 0)
    return int((usable(s, vdepth)[t].all(axis=1) & (area != 0) & (n > small_max)).sum())


def visibility(screens, vdepths, depths, tol):
    """visible [n] uint64 from every view's (screen [n, 2], vdepth [n]) and rendered depth map [H, W]; tol as the float32 the call takes"""
    n = np.asarray(screens[0]).shape[0]
    vis = np.zeros(n, np.uint64)
    factor = 1.0 + float(np.float32(tol))
    for v, (s, d, z) in enumerate(zip(screens, vdepths, depths)):
        s = np.asarray(s, dtype=np.int64)
        H, W = z.shape
        px, py = (s[:, 0] + 128) >> 8, (s[:, 1] + 128) >> 8
        inside = usable(s, d) & (px >= 0) & (px < W) & (py >= 0) & (py < H)
        zz = z[np.clip(py, 0, H - 1), np.clip(px, 0, W - 1)].astype(np.float64)
        with np.errstate(invalid="ignore"):
            seen = inside & (np.isnan(zz) | (np.asarray(d).astype(np.float64) <= zz * factor))
        vis |= seen.astype(np.uint64) << np.uint64(v)
    return vis
