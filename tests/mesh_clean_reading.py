"""The yardstick of the mesh clean-up calls (include/mvskit_engine.h, "Mesh clean-up"), a second reading in numpy.

components() labels by repeated minimum-label propagation over the edges, prune() works with boolean masks and cumsum, smooth_exact()
restates mvs_engine_mesh_smooth operation by operation: float32 terms, the power-of-two scale from the largest component, int64 sums
with np.add.at, the float64 update, the cast.  Every result is integer or an integer sum: equality of bytes is the yardstick."""
import numpy as np


def _mesh(verts, tris):
    v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(tris, np.int64).reshape(-1, 3)
    return v, t


def components(n_v, tris):
    """-> (label [n_v] int32: the smallest vertex id of the component; ntris [n_v] int32: the triangles of the component; n_components:
    the components with at least one triangle)"""
    t = np.ascontiguousarray(tris, np.int64).reshape(-1, 3)
    label = np.arange(n_v, dtype=np.int64)
    if t.shape[0]:
        assert t.min() >= 0 and t.max() < n_v
        a = np.concatenate([t[:, 0], t[:, 0]])
        b = np.concatenate([t[:, 1], t[:, 2]])
        while True:
            m = np.minimum(label[a], label[b])
            new = label.copy()
            np.minimum.at(new, a, m)
            np.minimum.at(new, b, m)
            new = new[new]  # pointer jumping: a label is a vertex of the same component with a label no larger
            if (new == label).all():
                break
            label = new
    count = np.zeros(n_v, np.int64)
    if t.shape[0]:
        np.add.at(count, label[t[:, 0]], 1)
    ntris = count[label]
    n_components = int(((label == np.arange(n_v)) & (count > 0)).sum())
    return label.astype(np.int32), ntris.astype(np.int32), n_components


def prune(verts, tris, min_triangles=1, largest_only=False):
    """-> (verts [n', 3] float32, tris [m', 3] int32, vmap [n] int32: the new id of every vertex, or -1)"""
    v, t = _mesh(verts, tris)
    n_v = v.shape[0]
    label, ntris, _ = components(n_v, t)
    keep_t = np.zeros(t.shape[0], bool)
    if t.shape[0]:
        keep_t = ntris[t[:, 0]] >= min_triangles
        if largest_only:
            roots = np.flatnonzero((label == np.arange(n_v)) & (ntris > 0))
            # the most triangles; among equals the smaller label
            best = roots[np.lexsort((roots, -ntris[roots].astype(np.int64)))[0]]
            keep_t &= label[t[:, 0]] == best
    keep_v = np.zeros(n_v, bool)
    keep_v[t[keep_t].reshape(-1)] = True
    new_id = np.cumsum(keep_v) - keep_v  # the exclusive scan of the flags
    vmap = np.where(keep_v, new_id, -1).astype(np.int32)
    return v[keep_v].copy(), vmap[t[keep_t]].astype(np.int32).reshape(-1, 3), vmap


def smooth_step(x, t, f):
    """one STEP with factor f: x [n, 3] float32, t [m, 3] int64 -> [n, 3] float32"""
    if t.shape[0] == 0 or x.shape[0] == 0:
        return x.copy()
    # per corner occurrence of vertex i in (i, j, k): the terms x_j - x_i and x_k - x_i
    i = np.concatenate([t[:, 0], t[:, 0], t[:, 1], t[:, 1], t[:, 2], t[:, 2]])
    j = np.concatenate([t[:, 1], t[:, 2], t[:, 2], t[:, 0], t[:, 0], t[:, 1]])
    with np.errstate(over="ignore", invalid="ignore"):
        term = x[j] - x[i]
    assert term.dtype == np.float32
    ok = np.isfinite(term).all(axis=1)
    M = float(np.abs(term[ok]).max()) if ok.any() else 0.0
    if M == 0.0:
        return x.copy()
    E = int(np.frexp(M)[1]) - 1  # floor(log2 M)
    S = float(np.ldexp(1.0, 30 - E))
    prod = term[ok].astype(np.float64) * S
    assert (np.abs(prod) < 2.0 ** 31).all()
    q = np.rint(prod).astype(np.int64)  # round-half-even
    A = np.zeros((x.shape[0], 3), np.int64)
    c = np.zeros(x.shape[0], np.int64)
    np.add.at(A, i[ok], q)
    np.add.at(c, i[ok], 1)
    have = c > 0
    u = (A[have].astype(np.float64) * float(np.ldexp(1.0, E - 30))) / c[have].astype(np.float64)[:, None]
    out = x.copy()
    with np.errstate(over="ignore"):
        out[have] = (x[have].astype(np.float64) + float(np.float32(f)) * u).astype(np.float32)
    return out


def smooth_exact(verts, tris, iterations=10, lam=0.5, mu=-0.53):
    """-> [n, 3] float32, the bytes mvs_engine_mesh_smooth gives"""
    x, t = _mesh(verts, tris)
    if t.shape[0]:
        assert t.min() >= 0 and t.max() < x.shape[0]
    x = x.copy()
    for _ in range(iterations):
        x = smooth_step(x, t, lam)
        if np.float32(mu) != 0:
            x = smooth_step(x, t, mu)
    return x
