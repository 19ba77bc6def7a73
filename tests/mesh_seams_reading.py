"""A numpy / pure-Python reading of the seam calls (include/mvskit_seams.h): the adjacency of triangles from the counts of the directed
edges, the quality table from the labelling's gates and areas in int64, the label smoothing as the header's loop over the triangles,
the seam samples as the contract's fp64 chain with integer sums, the offsets as the header's elimination in Python floats, and the
levelled atlas.  It builds on mesh_texture_reading.py and mesh_render_reading.py and works from a given (screen, vdepth) per view, the
device's own or a float64 projection: nothing but integer arithmetic and IEEE fp64 lies between it and the device, so the yardstick is
equality of bytes.  numpy only, no GPU."""
import math

import numpy as np

import mesh_fill_reading as fr
import mesh_texture_reading as tr
from mesh_render_reading import usable

LIMIT = 1 << 30


# ---- 1. adjacency
def adjacency(n_v, tris):
    """-> (nbr [m, 3] int32, n_irregular): nbr[t][k] = the row with the reverse of edge k of t when both directed edges occur once"""
    t = fr._tris(int(n_v), tris)
    m = t.shape[0]
    nbr = np.full((m, 3), -1, np.int32)
    if m == 0:
        return nbr, 0
    ok = (t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])
    rows = np.flatnonzero(ok)
    if rows.shape[0] == 0:
        return nbr, 0
    u = t[rows]
    a = np.stack([u[:, 0], u[:, 1], u[:, 2]], axis=1).reshape(-1)  # edge k of a row: a -> b
    b = np.stack([u[:, 1], u[:, 2], u[:, 0]], axis=1).reshape(-1)
    owner = np.repeat(rows, 3)
    key = a * LIMIT + b
    order = np.argsort(key, kind="stable")
    skey = key[order]
    ukey, first, f = np.unique(skey, return_index=True, return_counts=True)
    uowner = owner[order][first]  # the owner of a key that occurs once
    rkey = b * LIMIT + a
    own = np.searchsorted(ukey, key)
    pos = np.minimum(np.searchsorted(ukey, rkey), ukey.shape[0] - 1)
    r = np.where(ukey[pos] == rkey, f[pos], 0)
    pair = (f[own] == 1) & (r == 1)
    flat = np.full(3 * rows.shape[0], -1, np.int64)
    flat[pair] = uowner[pos[pair]]
    nbr[rows] = flat.reshape(-1, 3).astype(np.int32)
    # the irregular pairs, as mvs_engine_mesh_boundaries counts them: once per distinct directed edge
    ua, ub = ukey // LIMIT, ukey % LIMIT
    upos = np.minimum(np.searchsorted(ukey, ub * LIMIT + ua), ukey.shape[0] - 1)
    ur = np.where(ukey[upos] == ub * LIMIT + ua, f[upos], 0)
    irregular = ~((f == 1) & (ur == 0)) & ~((f == 1) & (ur == 1))
    return nbr, int((irregular & ((ua < ub) | (ur == 0))).sum())


# ---- 2. quality
def face_quality(screens, vdepths, tris, sizes, signs, visible=None, front_only=True):
    """-> quality [m, nviews] uint8: 0 for no candidate, else max(1, 255 |area_v| // best_t)"""
    t = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    m, nviews = t.shape[0], len(screens)
    area = np.zeros((m, nviews), np.int64)
    for v in range(nviews):
        if m == 0 or (front_only and signs[v] == 0):
            continue
        s = np.asarray(screens[v], dtype=np.int64).reshape(-1, 2)
        W, H = sizes[v]
        gate = usable(s, vdepths[v]) & (s[:, 0] >= 0) & (s[:, 0] <= 256 * (W - 1) - 1) & (s[:, 1] >= 0) & (s[:, 1] <= 256 * (H - 1) - 1)
        if visible is not None:
            gate &= ((np.asarray(visible, dtype=np.uint64) >> np.uint64(v)) & np.uint64(1)).astype(bool)
        a = tr.signed_area(s, t)
        cand = gate[t].all(axis=1) & (a != 0)
        if front_only:
            cand &= np.sign(a) == signs[v]
        area[:, v] = np.where(cand, np.abs(a), 0)
    best = area.max(axis=1, keepdims=True) if m else np.zeros((0, 1), np.int64)
    q = np.where(area > 0, np.maximum(1, 255 * area // np.maximum(best, 1)), 0)
    return q.astype(np.uint8)


# ---- 3. smoothing
def count_seams(nbr, label):
    """the adjacent pairs, counted once, whose labels are both >= 0 and differ"""
    nbr, label = np.asarray(nbr, np.int64), np.asarray(label, np.int64)
    if nbr.shape[0] == 0:
        return 0
    t = np.arange(nbr.shape[0])[:, None]
    lu = label[np.maximum(nbr, 0)]
    return int(((nbr > t) & (label[:, None] >= 0) & (lu >= 0) & (lu != label[:, None])).sum())


def proposals(nbr, quality, label, keep):
    """-> (proposal [m] int64, -1 for none; score [m] int64: (gain << 8) | quality of the proposal where the gain is above 0, else 0)"""
    m = nbr.shape[0]
    prop, score = np.full(m, -1, np.int64), np.zeros(m, np.int64)
    for t in range(m):
        own = int(label[t])
        if own < 0:
            continue
        ls = [int(label[u]) if u >= 0 else -1 for u in nbr[t]]
        best = None
        for l in ls:
            if l < 0 or l == own or int(quality[t, l]) < keep:
                continue
            cand = (ls.count(l), int(quality[t, l]), -l)
            if best is None or cand > best:
                best = cand
        if best is None:
            continue
        gain = best[0] - ls.count(own)
        prop[t] = -best[2]
        if gain > 0:
            score[t] = (gain << 8) | best[1]
    return prop, score


def smooth_labels(n_v, tris, quality, label, keep=192, iterations=64):
    """-> (label_out [m] int32, stats [4] int64 = seams before, seams after, moves, iterations that moved something)"""
    t = fr._tris(int(n_v), tris)
    quality = np.asarray(quality, np.uint8)  # [m, nviews_q]
    assert quality.ndim == 2 and quality.shape[0] == t.shape[0]
    lab = np.array(label, dtype=np.int64).reshape(-1)
    if lab.shape[0] and (lab.min() < -1 or lab.max() >= quality.shape[1]):
        raise fr.Refused("a label outside -1 .. nviews_q - 1")
    nbr, _ = adjacency(n_v, t)
    triple = [tuple(sorted(int(i) for i in row)) for row in t]
    before = count_seams(nbr, lab)
    moves = moved_its = 0
    for _ in range(int(iterations)):
        prop, score = proposals(nbr, quality, lab, int(keep))
        movers = []
        for x in np.flatnonzero(score > 0):
            wins = True
            for u in nbr[x]:
                if u < 0 or score[u] <= 0:
                    continue
                if not (score[x] > score[u] or (score[x] == score[u] and triple[x] < triple[u])):
                    wins = False
            if wins:
                movers.append(x)
        if not movers:
            break
        lab[movers] = prop[movers]
        moves += len(movers)
        moved_its += 1
    return lab.astype(np.int32), np.int64([before, count_seams(nbr, lab), moves, moved_its])


# ---- 4. levels
def _bilinear(images, view, x, y):
    """TEXEL's c before rounding, [n, 3] float64, at the unclamped positions (x, y) in images[view[i]]; every view at least 2 x 2 here"""
    c = np.zeros((x.shape[0], 3))
    for v in np.unique(view):
        mine = view == v
        img = np.asarray(images[v]).astype(np.float64)
        H, W = img.shape[:2]
        xv = np.minimum(np.maximum(x[mine], 0.0), float(W - 1) - 1.0 / 256)
        yv = np.minimum(np.maximum(y[mine], 0.0), float(H - 1) - 1.0 / 256)
        fix, fiy = np.floor(xv), np.floor(yv)
        gx, gy = (xv - fix)[:, None], (yv - fiy)[:, None]
        a, b = fix.astype(np.int64), fiy.astype(np.int64)
        top = (1.0 - gx) * img[b, a] + gx * img[b, a + 1]
        bot = (1.0 - gx) * img[b + 1, a] + gx * img[b + 1, a + 1]
        c[mine] = (1.0 - gy) * top + gy * bot
    return c


def seam_edges(n_v, tris, flags, label):
    """-> (t, k, u) int64 arrays: the seam edges, each from the side whose directed edge p -> q has p < q"""
    t = fr._tris(int(n_v), tris)
    nbr, _ = adjacency(n_v, t)
    label = np.asarray(label, np.int64).reshape(-1)
    flags = np.asarray(flags, bool)
    tt, kk = np.nonzero(nbr >= 0)
    uu = nbr[tt, kk].astype(np.int64)
    p, q = t[tt, kk], t[tt, (kk + 1) % 3]
    take = flags[tt] & flags[uu] & (label[tt] != label[uu]) & (p < q)
    return tt[take], kk[take], uu[take]


def seam_pairs(screens, vdepths, tris, label, images, samples=4):
    """-> (pairs [nviews, nviews, 4] int64, n_seam_edges)"""
    nviews = len(screens)
    t = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    label = np.asarray(label, np.int64).reshape(-1)
    n_v = np.asarray(vdepths[0]).shape[0] if nviews else 0
    pairs = np.zeros((nviews, nviews, 4), np.int64)
    if t.shape[0] == 0:
        return pairs, 0
    flags = tr.honoured(screens, vdepths, t, label)
    tt, kk, uu = seam_edges(n_v, t, flags, label)
    if tt.shape[0] == 0:
        return pairs, 0
    p, q = t[tt, kk], t[tt, (kk + 1) % 3]
    la, lb = label[tt], label[uu]
    S = np.stack([np.asarray(s, dtype=np.int64).reshape(-1, 2) for s in screens])  # [nviews, n, 2]
    D = np.stack([np.asarray(d, dtype=np.float32) for d in vdepths])
    small = np.array([im.shape[0] < 2 or im.shape[1] < 2 for im in images])
    for k in range(samples + 1):
        L, good = [], np.ones(tt.shape[0], bool)
        for view in (la, lb):
            ap = float(samples - k) * D[view, p].astype(np.float64)
            aq = float(k) * D[view, q].astype(np.float64)
            den = ap + aq
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                xs = (ap * S[view, p, 0].astype(np.float64) + aq * S[view, q, 0].astype(np.float64)) / den
                ys = (ap * S[view, p, 1].astype(np.float64) + aq * S[view, q, 1].astype(np.float64)) / den
                x, y = xs / 256.0, ys / 256.0
                ok = (den > 0) & np.isfinite(den) & ~np.isnan(x) & ~np.isnan(y) & ~small[view]
            good &= ok
            c = np.zeros((tt.shape[0], 3))
            if ok.any():
                c[ok] = _bilinear(images, view[ok], x[ok], y[ok])
            L.append(np.floor(c * 16.0 + 0.5).astype(np.int64))
        d = (L[0] - L[1])[good]
        a, b = la[good], lb[good]
        lo, hi, sign = np.minimum(a, b), np.maximum(a, b), np.where(a < b, 1, -1)
        np.add.at(pairs[:, :, 0], (lo, hi), 1)
        for ch in range(3):
            np.add.at(pairs[:, :, 1 + ch], (lo, hi), sign * d[:, ch])
    for a in range(nviews):
        for b in range(a + 1, nviews):
            pairs[b, a, 0] = pairs[a, b, 0]
            pairs[b, a, 1:] = -pairs[a, b, 1:]
    return pairs, int(tt.shape[0])


def offsets(pairs, max_shift=32):
    """-> offset [nviews, 3] int32 in 1/16 grey level: the header's elimination, a Python float loop"""
    pairs = np.asarray(pairs, np.int64)
    n = pairs.shape[0]
    out = np.zeros((n, 3), np.int32)
    lim = 16.0 * float(max_shift)
    for ch in range(3):
        A = [[0.0] * n for _ in range(n)]
        rhs = [0.0] * n
        for a in range(n):
            diag, s = 1.0, 0.0
            for b in range(n):
                if b == a:
                    continue
                diag = diag + float(pairs[a, b, 0])
                s = s + float(pairs[a, b, 1 + ch])
                A[a][b] = -float(pairs[a, b, 0])
            A[a][a] = diag
            rhs[a] = -s
        for i in range(n):
            for r in range(i + 1, n):
                f = A[r][i] / A[i][i]
                for c in range(i, n):
                    A[r][c] = A[r][c] - f * A[i][c]
                rhs[r] = rhs[r] - f * rhs[i]
        g = [0.0] * n
        for i in range(n - 1, -1, -1):
            s = rhs[i]
            for c in range(i + 1, n):
                s = s - A[i][c] * g[c]
            g[i] = s / A[i][i]
        for a in range(n):
            out[a, ch] = int(math.floor(min(max(g[a], -lim), lim) + 0.5))
    return out


def seam_levels(screens, vdepths, tris, label, images, max_shift=32, samples=4):
    """-> (offset [nviews, 3] int32, pairs [nviews, nviews, 4] int64, n_seam_edges)"""
    pairs, n = seam_pairs(screens, vdepths, tris, label, images, samples)
    return offsets(pairs, max_shift), pairs, n


# ---- 5. the levelled atlas
def texture_levelled(screens, vdepths, tris, label, images, offset, res, width):
    """mesh_texture_reading.texture with the byte clamp(floor(c + offset[v][ch] / 16.0 + 0.5), 0, 255); offset None: all zeros"""
    r = tr.texture(screens, vdepths, tris, label, images, res, width)
    if offset is None:
        return r
    offset = np.asarray(offset, np.int32).reshape(len(screens), 3)
    label = np.asarray(label, np.int64).reshape(-1)
    yy, xx = np.nonzero(~np.isnan(r["xy"][..., 0]))
    if yy.shape[0]:
        view = label[r["owner"][yy, xx]]
        c = _bilinear(images, view, r["xy"][yy, xx, 0], r["xy"][yy, xx, 1])
        byte = np.floor(c + offset[view].astype(np.float64) / 16.0 + 0.5)
        atlas = r["atlas"].copy()
        atlas[yy, xx] = np.minimum(np.maximum(byte, 0.0), 255.0).astype(np.uint8)
        r = dict(r, atlas=atlas)
    return r
