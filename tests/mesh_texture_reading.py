"""A numpy reading of the textured mesh (include/mvskit_texture.h: mvs_engine_mesh_face_views, mvs_engine_mesh_texture): the candidate
gates and the largest |area| in int64, the atlas layout from a cumulative sum, every texel as the contract's fp64 chain, vectorised over
the texels of the atlas.  It works from a given (screen, vdepth) per view -- its own float64 projection (mesh_render_reading.project64)
or the device's own, which leaves nothing but integer arithmetic and IEEE fp64 between the two, so the yardstick is equality of bytes --
and from the views' images at the engine's level.  numpy only, no GPU."""
import numpy as np

from mesh_render_reading import usable


def front_sign(P):
    """f_v of the camera P [3, 4] (float64 of the float32 camera at the level): the sign of a triangle's area when its face vector
    points to the camera centre, -sign(det M)"""
    det = np.linalg.det(np.asarray(P, dtype=np.float64)[:, :3])
    return -1 if det > 0 else (1 if det < 0 else 0)


def signed_area(screen, tris):
    p = np.asarray(screen, dtype=np.int64).reshape(-1, 2)[np.asarray(tris, dtype=np.int64).reshape(-1, 3)]  # [m, 3, 2]
    return (p[:, 1, 0] - p[:, 0, 0]) * (p[:, 2, 1] - p[:, 0, 1]) - (p[:, 1, 1] - p[:, 0, 1]) * (p[:, 2, 0] - p[:, 0, 0])


def face_views(screens, vdepths, tris, sizes, signs, visible=None, front_only=True):
    """-> (label [m] int32, area [m] int64, n_faces [nviews] int64) from every view's (screen [n, 2], vdepth [n]), its (W, H) and f_v"""
    t = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    m, nviews = t.shape[0], len(screens)
    best, label = np.zeros(m, np.int64), np.full(m, -1, np.int32)
    for v in range(nviews):
        if m == 0 or (front_only and signs[v] == 0):
            continue
        s = np.asarray(screens[v], dtype=np.int64).reshape(-1, 2)
        W, H = sizes[v]
        ok = usable(s, vdepths[v])
        window = (s[:, 0] >= 0) & (s[:, 0] <= 256 * (W - 1) - 1) & (s[:, 1] >= 0) & (s[:, 1] <= 256 * (H - 1) - 1)
        gate = ok & window
        if visible is not None:
            gate &= ((np.asarray(visible, dtype=np.uint64) >> np.uint64(v)) & np.uint64(1)).astype(bool)
        area = signed_area(s, t)
        cand = gate[t].all(axis=1) & (area != 0)
        if front_only:
            cand &= np.sign(area) == signs[v]
        take = cand & (np.abs(area) > best)  # ascending views and a strict comparison: the lowest view among equals
        best[take] = np.abs(area)[take]
        label[take] = v
    faces = np.array([(label == v).sum() for v in range(nviews)], dtype=np.int64)
    return label, best, faces


def honoured(screens, vdepths, tris, label):
    """[m] bool: the triangle's label names a view in which its three vertices are usable and it has an area"""
    t = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    label = np.asarray(label, dtype=np.int64).reshape(-1)
    out = np.zeros(t.shape[0], bool)
    for v in range(len(screens)):
        mine = label == v
        if mine.any():
            out |= mine & usable(screens[v], vdepths[v])[t].all(axis=1) & (signed_area(screens[v], t) != 0)
    return out


def layout(n_textured, res, width):
    """-> (B, cpr, n_cells, height)"""
    B = res + 3
    cpr = width // B
    n_cells = 1 + (n_textured + 1) // 2
    return B, cpr, n_cells, -(-n_cells // cpr) * B


def corners(flags, res, width):
    """uv [m, 3, 2] int32: the (column, row) of the corner texels; an untextured triangle gets the centre texel of cell 0"""
    flags = np.asarray(flags, dtype=bool)
    B, cpr, _, _ = layout(int(flags.sum()), res, width)
    k = np.cumsum(flags) - flags
    q = 1 + k // 2
    origin = np.stack([(q % cpr) * B, (q // cpr) * B], axis=1)[:, None, :]
    lower = np.array([[0, 0], [res, 0], [0, res]])
    upper = np.array([[res + 2, res + 2], [2, res + 2], [res + 2, 2]])
    uv = origin + np.where((k % 2 == 1)[:, None, None], upper, lower)
    uv[~flags] = B // 2
    return uv.astype(np.int32)


def owners(n_textured, res, width):
    """the atlas texel by texel -> (height, k [height, width] int64: the honoured triangle that owns the texel or -1, n1, n2 [height,
    width] int64: its integer weights there)"""
    B, cpr, n_cells, height = layout(n_textured, res, width)
    row, col = np.mgrid[0:height, 0:width]
    cy, j, cx, i = row // B, row % B, col // B, col % B
    q = cy * cpr + cx
    upper = i + j >= res + 3
    k = 2 * (q - 1) + upper
    owned = (cx < cpr) & (q >= 1) & (q < n_cells) & (k < n_textured)
    n1, n2 = np.where(upper, res + 2 - i, i), np.where(upper, res + 2 - j, j)
    return height, np.where(owned, k, -1), n1, n2


def texture(screens, vdepths, tris, label, images, res, width):
    """-> dict(atlas [height, width, 3] uint8, uv [m, 3, 2] int32, height, n_textured, flags [m] bool, owner [height, width] the
    triangle row that owns each texel or -1, xy [height, width, 2] float64 the unclamped position in the labelled view, NaN where grey).
    images[v]: [H, W, 3] uint8, the view at the engine's level"""
    t = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    label = np.asarray(label, dtype=np.int64).reshape(-1)
    flags = honoured(screens, vdepths, t, label) if t.shape[0] else np.zeros(0, bool)
    rows = np.flatnonzero(flags)
    nt = rows.shape[0]
    height, k, n1, n2 = owners(nt, res, width)
    atlas = np.full((height, width, 3), 128, np.uint8)
    owner = np.where(k >= 0, rows[np.maximum(k, 0)] if nt else -1, -1)
    xy = np.full((height, width, 2), np.nan)
    if nt:
        # the nine numbers of every honoured triangle in its own view
        sx, sy, d = np.zeros((nt, 3)), np.zeros((nt, 3)), np.ones((nt, 3))
        Wt, Ht = np.zeros(nt, np.int64), np.zeros(nt, np.int64)
        for v in range(len(screens)):
            mine = label[rows] == v
            if mine.any():
                s = np.asarray(screens[v], dtype=np.int64).reshape(-1, 2)
                ids = t[rows[mine]]
                sx[mine], sy[mine] = s[ids, 0].astype(np.float64), s[ids, 1].astype(np.float64)
                d[mine] = np.asarray(vdepths[v])[ids].astype(np.float64)
                Wt[mine], Ht[mine] = images[v].shape[1], images[v].shape[0]
        yy, xx = np.nonzero(k >= 0)
        kk = k[yy, xx]
        a1n, a2n = n1[yy, xx].astype(np.float64), n2[yy, xx].astype(np.float64)
        a0n = (res - n1[yy, xx] - n2[yy, xx]).astype(np.float64)
        w = d[kk]  # a point of the triangle in space: the weights of its homogeneous image are n_m d_m
        a0, a1, a2 = a0n * w[:, 0], a1n * w[:, 1], a2n * w[:, 2]
        den = a0 + a1 + a2
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            xs = (a0 * sx[kk, 0] + a1 * sx[kk, 1] + a2 * sx[kk, 2]) / den
            ys = (a0 * sy[kk, 0] + a1 * sy[kk, 1] + a2 * sy[kk, 2]) / den
            x, y = xs / 256.0, ys / 256.0
            W, H = Wt[kk], Ht[kk]
            good = (den > 0) & np.isfinite(den) & ~np.isnan(x) & ~np.isnan(y) & (W >= 2) & (H >= 2)
        yy, xx, kk, x, y, W, H = yy[good], xx[good], kk[good], x[good], y[good], W[good], H[good]
        xy[yy, xx, 0], xy[yy, xx, 1] = x, y
        x = np.minimum(np.maximum(x, 0.0), (W - 1).astype(np.float64) - 1.0 / 256)
        y = np.minimum(np.maximum(y, 0.0), (H - 1).astype(np.float64) - 1.0 / 256)
        fix, fiy = np.floor(x), np.floor(y)
        fx, fy = x - fix, y - fiy
        ix, iy = fix.astype(np.int64), fiy.astype(np.int64)
        out = np.zeros((yy.shape[0], 3), np.uint8)
        view = label[rows[kk]]
        for v in np.unique(view):
            mine = view == v
            img = np.asarray(images[v]).astype(np.float64)
            a, b, gx, gy = ix[mine], iy[mine], fx[mine][:, None], fy[mine][:, None]
            top = (1.0 - gx) * img[b, a] + gx * img[b, a + 1]
            bot = (1.0 - gx) * img[b + 1, a] + gx * img[b + 1, a + 1]
            out[mine] = np.floor((1.0 - gy) * top + gy * bot + 0.5).astype(np.uint8)
        atlas[yy, xx] = out
    return dict(atlas=atlas, uv=corners(flags, res, width), height=height, n_textured=nt, flags=flags, owner=owner, xy=xy)


def by_weights(result, res, width, t):
    """{(n1, n2): (r, g, b)} of the texels that triangle row t owns in a texture() result: what must not depend on where the triangle
    lies in the atlas (a lower half holds the diagonal n1 + n2 = res + 2 more than an upper one)"""
    _, _, n1, n2 = owners(result["n_textured"], res, width)
    yy, xx = np.nonzero(result["owner"] == t)
    return {(int(a), int(b)): tuple(int(c) for c in result["atlas"][y, x]) for y, x, a, b in zip(yy, xx, n1[yy, xx], n2[yy, xx])}
