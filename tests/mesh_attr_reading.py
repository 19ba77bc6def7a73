"""The yardstick of the mesh attribute calls (include/mvskit_engine.h, "Vertex normals and colours"), a second reading in numpy.

normals_exact() restates mvs_engine_mesh_normals operation by operation: float32 face vectors, the power-of-two scale from the largest
component, int64 sums, float64 normalisation, the cast.  Equality of bytes is the yardstick.
colours64() restates mvs_engine_mesh_colours in float64 on render64 / agree64 of tests/maps_reading.py (their bits and `unsure`
masks), as mesh_reading.tsdf64 does for the volume, and says which vertices have a (vertex, view) pair inside a margin."""
import numpy as np

from maps_reading import COS_MARGIN, EDGE_PX, S_MARGIN, popcount


def normals_exact(verts, tris):
    """-> [n, 3] float32, the bytes mvs_engine_mesh_normals gives"""
    v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(tris, np.int64).reshape(-1, 3)
    out = np.zeros((v.shape[0], 3), np.float32)
    if t.shape[0] == 0 or v.shape[0] == 0:
        return out
    with np.errstate(over="ignore", invalid="ignore"):
        a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
        e1, e2 = b - a, c - a  # float32
        f = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
    assert f.dtype == np.float32
    ok = np.isfinite(f).all(axis=1)
    M = float(np.abs(f[ok]).max()) if ok.any() else 0.0
    if M == 0.0:
        return out
    E = int(np.frexp(M)[1]) - 1  # floor(log2 M)
    S = float(np.ldexp(1.0, 30 - E))
    prod = f[ok].astype(np.float64) * S
    assert (np.abs(prod) < 2.0 ** 31).all()
    q = np.rint(prod).astype(np.int64)  # round-half-even
    A = np.zeros((v.shape[0], 3), np.int64)
    for k in range(3):
        np.add.at(A, t[ok][:, k], q)
    ad = A.astype(np.float64)
    length = np.sqrt(ad[:, 0] * ad[:, 0] + ad[:, 1] * ad[:, 1] + ad[:, 2] * ad[:, 2])
    have = length > 0
    out[have] = (ad[have] / length[have, None]).astype(np.float32)
    return out


def _bilinear64(img, x, y):
    """ply_colour's sample in float64: img [H, W, 3] uint8, (x, y) inside [0, W-1) x [0, H-1)"""
    lx, ly = np.floor(x).astype(int), np.floor(y).astype(int)
    dx1, dy1 = (x - lx)[:, None], (y - ly)[:, None]
    dx0, dy0 = 1.0 - dx1, 1.0 - dy1
    im = img.astype(np.float64)
    return (im[ly, lx] * (dx0 * dy0) + im[ly + 1, lx] * (dx0 * dy1)) + (im[ly, lx + 1] * (dx1 * dy0) + im[ly + 1, lx + 1] * (dx1 * dy1))


def colours64(pat, ids, bits, unsure, cams, images, masks, verts, normals, min_consistent=1, occl_tol=0.01, min_cos=0.1, edge_px=EDGE_PX,
              s_margin=S_MARGIN, cos_margin=COS_MARGIN):
    """mvs_engine_mesh_colours in float64.  pat: the records by pool index; ids[v], bits[v], unsure[v]: view v's id map and the agree
    words of agree64 with their margins; cams: cameras64 of tests/maps_reading.py; images[v]: the level-L pyramid [H, W, 3] uint8; masks[v]:
    the level-L mask as booleans, or None; normals: [n, 3] or None; edge_px, s_margin, cos_margin: maps_reading.margins().
    -> dict of per-vertex arrays: mean [n, 3] (the unrounded weighted mean; NaN with no view), used (uint8), sure (no pair of the vertex
    lies inside a margin), reached (some view has the vertex in its sampling window), confirmed (the confirmed tier was chosen)"""
    X = np.asarray(verts, np.float64).reshape(-1, 3)
    N = X.shape[0]
    nrm = None if normals is None else np.asarray(normals, np.float64).reshape(-1, 3)
    facing = np.zeros(N, bool) if nrm is None else ~(nrm == 0).all(axis=1)
    sw, sc, cnt = np.zeros((2, N)), np.zeros((2, N, 3)), np.zeros((2, N), np.int64)
    sure, reached = np.ones(N, bool), np.zeros(N, bool)
    for v, cam in enumerate(cams if len(pat) else []):  # a pool without a patch: no view counts
        W, H = cam["W"], cam["H"]
        h = X @ cam["P"][:, :3].T + cam["P"][:, 3]
        with np.errstate(divide="ignore", invalid="ignore"):
            x, y = h[:, 0] / h[:, 2], h[:, 1] / h[:, 2]
            front = h[:, 2] > 0
            win = front & (x >= 0) & (y >= 0) & (x < W - 1) & (y < H - 1)
            # within 1e-3 pixel of the window's edge, on either side of it
            near_win = front & (x > -edge_px) & (y > -edge_px) & (x < W - 1 + edge_px) & (y < H - 1 + edge_px)
            edge_win = near_win & ((np.abs(x) <= edge_px) | (np.abs(y) <= edge_px) | (np.abs(x - (W - 1)) <= edge_px) | (np.abs(y - (H - 1)) <= edge_px))
        sure &= ~edge_win
        reached |= win
        xs, ys = np.where(win, x, 0.0), np.where(win, y, 0.0)
        fx, fy = np.floor(xs + 0.5).astype(int), np.floor(ys + 0.5).astype(int)
        valid = ids[v] >= 0
        use = valid & (popcount(bits[v]) >= min_consistent)
        use_lo = valid & (popcount(bits[v] & ~unsure[v]) >= min_consistent)
        use_hi = valid & (popcount(bits[v] | unsure[v]) >= min_consistent)
        fg = np.ones((H, W), bool) if masks is None or masks[v] is None else np.asarray(masks[v], bool)
        # what the surface test meets at a pixel: background -2, not usable -1, else the patch
        state = np.where(fg, np.where(use, ids[v], -1), -2)
        # a projection within 1e-3 pixel of a rounding boundary across which that differs
        differs = np.zeros(N, bool)
        for yy in (np.floor(ys + 0.5 - edge_px).astype(int), np.floor(ys + 0.5 + edge_px).astype(int)):
            for xx in (np.floor(xs + 0.5 - edge_px).astype(int), np.floor(xs + 0.5 + edge_px).astype(int)):
                cy, cx = np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)
                differs |= (state[cy, cx] != state[fy, fx]) | (use_lo != use_hi)[cy, cx]
        sure &= ~(win & differs)
        ok = win & fg[fy, fx]
        # the pixel's usability rests on an unsure agree pair
        sure &= ~(ok & (use_lo != use_hi)[fy, fx])
        d = cam["C"] - X
        w = np.ones(N)
        if nrm is not None:
            with np.errstate(divide="ignore", invalid="ignore"):
                wf = (nrm * d).sum(1) / np.sqrt((d * d).sum(1))
            w = np.where(facing, wf, 1.0)
            sure &= ~(ok & facing & (np.abs(wf - min_cos) < cos_margin))
            with np.errstate(invalid="ignore"):
                ok &= ~facing | (wf >= min_cos)
        usable = ok & use[fy, fx]
        q = pat[np.maximum(ids[v][fy, fx], 0)]
        nq, X0q = q["normal"][:, :3].astype(np.float64), q["coord"][:, :3].astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            den = (nq * (X - cam["C"])).sum(1)
            s = (nq * (X0q - cam["C"])).sum(1) / den
            good = np.isfinite(den) & (den != 0) & (np.abs(s - 1.0) <= occl_tol)
            sure &= ~(usable & (np.abs(np.abs(s - 1.0) - occl_tol) < s_margin))
        conf = usable & good
        unconf = ok & ~use[fy, fx]
        sample = _bilinear64(images[v], xs, ys)
        for tier, sel in ((0, conf), (1, unconf)):
            sw[tier][sel] += w[sel]
            sc[tier][sel] += w[sel, None] * sample[sel]
            cnt[tier][sel] += 1
    confirmed = cnt[0] > 0
    tier = np.where(confirmed, 0, 1)
    idx = np.arange(N)
    n_used = cnt[tier, idx]
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = np.where((n_used > 0)[:, None], sc[tier, idx] / sw[tier, idx][:, None], np.nan)
    used = np.where(n_used > 0, n_used | np.where(confirmed, 0x80, 0), 0).astype(np.uint8)
    return dict(mean=mean, used=used, sure=sure, reached=reached, confirmed=confirmed & (n_used > 0))
