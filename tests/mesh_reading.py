"""The yardstick of the mesh calls (include/mvskit_engine.h, "Triangle mesh"): marching tetrahedra in numpy float32, written from the rule
text in the stated operation order, and a float64 reading of the TSDF on top of render64 / agree64 of tests/maps_reading.py.

extract() restates mvs_engine_extract_mesh: equality is the yardstick (vertex count, order and bits; the triangle list).  The orientation
of a triangle is not read from a table here: it is decided on the tetrahedron's ideal geometry -- the crossings at the edge midpoints,
the normal against the direction from the centroid of the inside corners to that of the outside ones -- which is the rule's own words.
tsdf64() restates mvs_engine_tsdf in float64 and says which (point, view) pairs lie inside a margin."""
import numpy as np

from maps_reading import EDGE_PX, S_MARGIN, popcount

#: the Kuhn split of a cube along its main diagonal, as corner tuples (corner c = dx + 2 dy + 4 dz)
TETS = ((0, 1, 3, 7), (0, 1, 5, 7), (0, 2, 3, 7), (0, 2, 6, 7), (0, 4, 5, 7), (0, 4, 6, 7))


def _corner(c):
    return np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1], np.int64)


def tet_triangles(tet, inside):
    """the triangles of one tetrahedron as tuples of edges (pairs of cube corners, lower first), oriented; inside: four booleans in the
    order of `tet`"""
    ins = [k for k in range(4) if inside[k]]
    out = [k for k in range(4) if not inside[k]]
    if not ins or not out:
        return []
    if len(ins) == 2:
        a, b = ins
        c, d = out
        q = [(a, c), (a, d), (b, d), (b, c)]
        tris = [(q[0], q[1], q[2]), (q[0], q[2], q[3])]
    else:
        a = ins[0] if len(ins) == 1 else out[0]
        b, c, d = [k for k in range(4) if k != a]
        tris = [((a, b), (a, c), (a, d))]
    pos = [_corner(c).astype(np.float64) for c in tet]
    toward = np.mean([pos[k] for k in out], axis=0) - np.mean([pos[k] for k in ins], axis=0)
    res = []
    for tri in tris:
        m = [(pos[x] + pos[y]) / 2 for x, y in tri]
        s = float(np.dot(np.cross(m[1] - m[0], m[2] - m[0]), toward))
        assert s != 0.0
        if s < 0:
            tri = (tri[0], tri[2], tri[1])
        res.append(tuple((min(tet[x], tet[y]), max(tet[x], tet[y])) for x, y in tri))
    return res


_CASES = {(t, m): tet_triangles(TETS[t], [(m >> k) & 1 for k in range(4)]) for t in range(6) for m in range(16)}


def lattice_positions(origin, voxel, dims):
    """[nz, ny, nx, 3] float32: origin[c] + (float)idx[c] * voxel, one multiplication and one addition"""
    nx, ny, nz = dims
    o, h = np.asarray(origin, np.float32), np.float32(voxel)
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return np.stack([o[0] + i.astype(np.float32) * h, o[1] + j.astype(np.float32) * h, o[2] + k.astype(np.float32) * h], axis=-1).astype(np.float32)


def observed(tsdf, count=None, min_count=1):
    obs = ~np.isnan(tsdf)
    if count is not None:
        obs &= count >= min_count
    return obs


def extract(origin, voxel, dims, tsdf, count=None, min_count=1):
    """-> (verts [n, 3] float32, tris [m, 3] int32) of the volume tsdf[nz, ny, nx] (count alike, or None)"""
    nx, ny, nz = dims
    F = np.asarray(tsdf, np.float32).reshape(nz, ny, nx)
    obs = observed(F, None if count is None else np.asarray(count).reshape(nz, ny, nx), min_count)
    with np.errstate(invalid="ignore"):
        ins = obs & (F < 0)
    pos = lattice_positions(origin, voxel, dims)
    mask = np.zeros((nz, ny, nx), np.uint8)
    for d in range(1, 8):
        dx, dy, dz = _corner(d)
        lo = (slice(0, nz - dz), slice(0, ny - dy), slice(0, nx - dx))
        hi = (slice(dz, nz), slice(dy, ny), slice(dx, nx))
        bit = obs[lo] & obs[hi] & (ins[lo] ^ ins[hi])
        mask[lo] |= bit.astype(np.uint8) << np.uint8(d - 1)
    flat = mask.ravel()
    bits = (flat[:, None] >> np.arange(7, dtype=np.uint8)) & 1  # [N, 7]: ascending (p, slot) in row-major order
    vbase = np.concatenate([[0], np.cumsum(bits.sum(1))]).astype(np.int64)
    p, slot = np.nonzero(bits)
    kk, jj, ii = np.unravel_index(p, (nz, ny, nx))
    d = slot + 1
    k2, j2, i2 = kk + ((d >> 2) & 1), jj + ((d >> 1) & 1), ii + (d & 1)
    Fa, Fb = F[kk, jj, ii], F[k2, j2, i2]
    pa, pb = pos[kk, jj, ii], pos[k2, j2, i2]
    t = (Fa / (Fa - Fb)).astype(np.float32)
    verts = (pa + (t[:, None] * (pb - pa)).astype(np.float32)).astype(np.float32)

    def edge(k, j, i, lo, hi):
        c = _corner(lo)
        q = ((k + c[2]) * ny + (j + c[1])) * nx + (i + c[0])
        s = hi - lo - 1
        assert (flat[q] >> s) & 1, "a triangle asks for a vertex that does not exist"
        return int(vbase[q]) + bin(int(flat[q]) & ((1 << s) - 1)).count("1")

    tris = []
    full = obs[:-1, :-1, :-1].copy()
    for c in range(1, 8):
        dx, dy, dz = _corner(c)
        full &= obs[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]
    for k, j, i in zip(*np.nonzero(full)):  # ascending linear index of corner 0
        cin = [bool(ins[k + ((c >> 2) & 1), j + ((c >> 1) & 1), i + (c & 1)]) for c in range(8)]
        for t_, tet in enumerate(TETS):
            m = sum(int(cin[c]) << n for n, c in enumerate(tet))
            for tri in _CASES[(t_, m)]:
                tris.append([edge(k, j, i, lo, hi) for lo, hi in tri])
    return verts.reshape(-1, 3), np.asarray(tris, np.int32).reshape(-1, 3)


def directed_edges(tris):
    e = np.concatenate([tris[:, [0, 1]], tris[:, [1, 2]], tris[:, [2, 0]]]).astype(np.int64)
    return e


def closed_and_oriented(tris):
    """every directed edge is met once and its reverse once"""
    e = directed_edges(tris)
    key = e[:, 0] * (1 << 32) + e[:, 1]
    rev = e[:, 1] * (1 << 32) + e[:, 0]
    return np.unique(key).shape[0] == key.shape[0] and np.array_equal(np.sort(key), np.sort(rev))


def euler(verts, tris):
    """V - E + F over the vertices that a triangle uses"""
    e = np.sort(directed_edges(tris), axis=1)
    return int(np.unique(tris).shape[0] - np.unique(e, axis=0).shape[0] + tris.shape[0])


def sphere_volume(dims, centers, radius, origin=(0.0, 0.0, 0.0), voxel=1.0):
    """min over the centres of |X - c| - radius on the lattice, float32 [nz, ny, nx]"""
    pos = lattice_positions(origin, voxel, dims).astype(np.float64)
    d = np.min([np.linalg.norm(pos - np.asarray(c, np.float64), axis=-1) - radius for c in centers], axis=0)
    return d.astype(np.float32)


def tsdf64(pat, ids, bits, unsure, cams, min_consistent, origin, voxel, dims, trunc, edge_px=EDGE_PX, s_margin=S_MARGIN):
    """mvs_engine_tsdf in float64.  pat: the records by pool index; ids[v], bits[v], unsure[v]: view v's id map and the agree words of
    agree64 with their margins; cams: cameras64 of tests/maps_reading.py; edge_px, s_margin: maps_reading.margins().
    -> dict of [nz, ny, nx] arrays: tsdf, count, sure (no pair of the point lies inside a margin), reached (some view takes the point to
    a usable pixel), bound (max over the contributing views of dz / (|cos(n_q, ray)| trunc))"""
    nx, ny, nz = dims
    X = lattice_positions(origin, voxel, dims).reshape(-1, 3).astype(np.float64)
    N = X.shape[0]
    total, cnt = np.zeros(N), np.zeros(N, np.int32)
    sure, reached, bound = np.ones(N, bool), np.zeros(N, bool), np.zeros(N)
    for v, cam in enumerate(cams):
        h = X @ cam["P"][:, :3].T + cam["P"][:, 3]
        assert (h[:, 2] > 0.1).all()
        px, py = h[:, 0] / h[:, 2] + 0.5, h[:, 1] / h[:, 2] + 0.5
        edge = np.minimum(np.abs(px - np.rint(px)), np.abs(py - np.rint(py))) <= edge_px
        fx, fy = np.floor(px).astype(int), np.floor(py).astype(int)
        inside = (fx >= 0) & (fx < cam["W"]) & (fy >= 0) & (fy < cam["H"])
        cy, cx = np.clip(fy, 0, cam["H"] - 1), np.clip(fx, 0, cam["W"] - 1)
        valid = ids[v] >= 0
        use_lo = valid & (popcount(bits[v] & ~unsure[v]) >= min_consistent)  # usable whatever the unsure pairs give
        use_hi = valid & (popcount(bits[v] | unsure[v]) >= min_consistent)   # usable if they all agree
        use = valid & (popcount(bits[v]) >= min_consistent)
        met = inside & use[cy, cx]
        # a pixel whose usability rests on an unsure agree pair
        sure &= ~(inside & (use_lo != use_hi)[cy, cx])
        # a projection within 1e-3 pixel of a rounding boundary may be taken to the pixel across it: that matters unless none of the
        # pixels it can be taken to could be usable
        any_use = np.zeros(N, bool)
        for yy in (np.floor(py - edge_px).astype(int), np.floor(py + edge_px).astype(int)):
            for xx in (np.floor(px - edge_px).astype(int), np.floor(px + edge_px).astype(int)):
                ok = (xx >= 0) & (xx < cam["W"]) & (yy >= 0) & (yy < cam["H"])
                any_use |= ok & use_hi[np.clip(yy, 0, cam["H"] - 1), np.clip(xx, 0, cam["W"] - 1)]
        sure &= ~(edge & any_use)
        q = pat[np.maximum(ids[v][cy, cx], 0)]
        nq, X0q = q["normal"][:, :3].astype(np.float64), q["coord"][:, :3].astype(np.float64)
        ray = X - cam["C"]
        with np.errstate(divide="ignore", invalid="ignore"):
            den = (nq * ray).sum(1)
            s = (nq * (X0q - cam["C"])).sum(1) / den
            dz = X @ cam["o"][:3] + cam["o"][3]
            sd = (s - 1.0) * dz
            cos = np.abs(den) / (np.linalg.norm(nq, axis=1) * np.linalg.norm(ray, axis=1))
        assert (dz > 0.1).all() and (cos[met] > 0.2).all(), "the scene has a grazing plane or a point behind a camera"
        sure &= ~(met & (np.abs(sd + trunc) < s_margin * dz))
        add = met & (sd >= -trunc)
        total[add] += np.minimum(sd[add] / trunc, 1.0)
        cnt[add] += 1
        reached |= met
        bound[add] = np.maximum(bound[add], dz[add] / (cos[add] * trunc))
    with np.errstate(invalid="ignore", divide="ignore"):
        tsdf = np.where(cnt > 0, total / np.maximum(cnt, 1), np.nan)
    shape = (nz, ny, nx)
    return dict(tsdf=tsdf.reshape(shape), count=cnt.reshape(shape), sure=sure.reshape(shape), reached=reached.reshape(shape),
                bound=bound.reshape(shape))
