"""The yardstick of mvs_engine_mesh_boundaries and mvs_engine_mesh_fill (include/mvskit_engine.h, "Mesh hole filling"), a second reading
in numpy written from the header: np.unique over the directed edges for their counts, a sorted search for the reverse of each, np.bincount
for out and in, repeated minimum-label propagation over the boundary half-edges for the components, cumsum for the rows of the new
triangles, and for the centroid the integer sum of the header -- int64 sums with np.add.at, np.rint, the division in float64 -- not
mean().  Every result is an integer, comes from an integer sum or is a copy of input bytes: equality of bytes is the yardstick."""
import numpy as np

LIMIT = 1 << 30


class Refused(ValueError):
    """what the two calls answer with MVS_ERR_ARG after their validating passes"""


def _tris(n_v, tris):
    t = np.ascontiguousarray(tris, np.int64).reshape(-1, 3)
    if t.shape[0] and (t.min() < 0 or t.max() >= n_v):
        raise Refused("a vertex index outside 0 .. n_v - 1")
    return t


def _analyse(n_v, t):
    """-> loop, length (int64), the three counts, nxt [n_v]: the end of the boundary half-edge that leaves a simple vertex (-1 elsewhere)"""
    loop = np.full(n_v, -1, np.int64)
    length = np.zeros(n_v, np.int64)
    nxt = np.full(n_v, -1, np.int64)
    # EDGES
    ok = (t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])
    u = t[ok]
    if u.shape[0] == 0:
        return loop, length, 0, 0, 0, nxt
    a = np.concatenate([u[:, 0], u[:, 1], u[:, 2]])
    b = np.concatenate([u[:, 1], u[:, 2], u[:, 0]])
    key, f = np.unique(a * LIMIT + b, return_counts=True)  # sorted: the distinct directed edges and cnt(a, b)
    a, b = key // LIMIT, key % LIMIT
    rkey = b * LIMIT + a
    pos = np.minimum(np.searchsorted(key, rkey), key.shape[0] - 1)
    r = np.where(key[pos] == rkey, f[pos], 0)
    boundary = (f == 1) & (r == 0)
    irregular = ~boundary & ~((f == 1) & (r == 1))
    n_irregular = int((irregular & ((a < b) | (r == 0))).sum())  # a pair with both directions present shows up twice
    cplx = np.zeros(n_v, bool)
    cplx[a[irregular]] = True
    cplx[b[irregular]] = True
    # VERTICES
    ha, hb = a[boundary], b[boundary]
    out, inn = np.bincount(ha, minlength=n_v), np.bincount(hb, minlength=n_v)
    on = (out + inn) > 0
    simple = (out == 1) & (inn == 1) & ~cplx
    # COMPONENTS
    label = np.arange(n_v, dtype=np.int64)
    while ha.shape[0]:
        m = np.minimum(label[ha], label[hb])
        new = label.copy()
        np.minimum.at(new, ha, m)
        np.minimum.at(new, hb, m)
        new = new[new]  # pointer jumping: a label is a vertex of the same component with a label no larger
        if (new == label).all():
            break
        label = new
    hedges = np.bincount(label[ha], minlength=n_v)
    bad = np.zeros(n_v, bool)
    bad[label[on & ~simple]] = True
    loop[on] = label[on]
    length[on] = np.where(bad[label[on]], -hedges[label[on]], hedges[label[on]])
    roots = on & (label == np.arange(n_v))
    n_loops, n_complex = int((roots & ~bad).sum()), int((roots & bad).sum())
    s = simple[ha]
    nxt[ha[s]] = hb[s]
    return loop, length, n_loops, n_complex, n_irregular, nxt


def boundaries(n_v, tris):
    """-> (loop [n_v] int32, length [n_v] int32, n_loops, n_complex, n_irregular)"""
    loop, length, n_loops, n_complex, n_irregular, _ = _analyse(int(n_v), _tris(int(n_v), tris))
    return loop.astype(np.int32), length.astype(np.int32), n_loops, n_complex, n_irregular


def closed(n_v, tris):
    """a closed edge-manifold: all three counts are 0"""
    return boundaries(n_v, tris)[2:] == (0, 0, 0)


def fill(verts, tris, max_edges=64):
    """-> (verts [n_v + new, 3] float32, tris [n_t + new, 3] int32, n_filled)"""
    v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    n_v = v.shape[0]
    if int(max_edges) < 3:
        raise Refused("max_edges < 3")
    t = _tris(n_v, tris)
    loop, length, _, _, _, nxt = _analyse(n_v, t)
    ids = np.arange(n_v)
    filled = (length >= 3) & (length <= int(max_edges))  # complex components carry a negative length
    if not np.isfinite(v[filled]).all():
        raise Refused("a loop vertex with a non-finite component")
    is_label = filled & (loop == ids)
    n_filled = int(is_label.sum())
    fan = filled & (length >= 4)
    # the new vertices, in ascending order of their loop's label
    centres = np.flatnonzero(fan & is_label)
    w = np.full(n_v, -1, np.int64)
    w[centres] = n_v + np.arange(centres.shape[0])
    new_v = np.zeros((centres.shape[0], 3), np.float32)  # M == 0: +0
    x = v[fan]
    M = float(np.abs(x).max()) if x.shape[0] else 0.0
    if M > 0.0:
        E = int(np.frexp(M)[1]) - 1  # floor(log2 M)
        prod = x.astype(np.float64) * float(np.ldexp(1.0, 30 - E))
        assert (np.abs(prod) < 2.0 ** 31).all()
        q = np.rint(prod).astype(np.int64)  # round-half-even
        A = np.zeros((n_v, 3), np.int64)
        np.add.at(A, loop[fan], q)
        p = (A[centres].astype(np.float64) * float(np.ldexp(1.0, E - 30))) / length[centres].astype(np.float64)[:, None]
        new_v = p.astype(np.float32)
    # the new triangles, in ascending order of their half-edge's origin
    origin = np.flatnonzero(fan | (is_label & (length == 3)))
    b = nxt[origin]
    third = np.where(length[origin] == 3, nxt[np.maximum(b, 0)], w[loop[origin]])
    new_t = np.stack([b, origin, third], axis=1).astype(np.int32).reshape(-1, 3)
    return np.concatenate([v, new_v]), np.concatenate([t.astype(np.int32), new_t]), n_filled
