"""The yardstick of mvs_engine_mesh_decimate (include/mvskit_engine.h, "Mesh decimation"), a second reading in numpy written from the
header: np.float32 arithmetic for the cell of a member and for the squared distance of placement 1, np.unique over the cell triples for
the clusters and over the sorted representatives for the duplicates, int64 sums with np.add.at, np.rint, the mean in float64.  Every
result is an integer, comes from an integer sum or is a copy of input bytes: equality of bytes is the yardstick."""
import numpy as np

GRID_MIN, GRID_MAX = -(1 << 20), (1 << 20) - 1


class Refused(ValueError):
    """what mvs_engine_mesh_decimate answers with MVS_ERR_ARG after its validating pass"""


def cells(verts, origin, cell):
    """[n, 3] float32: floorf((x - origin) / cell) per component in float32 (a NaN or an infinity where the position has one)"""
    v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    o, h = np.asarray(origin, np.float32).reshape(3), np.float32(cell)
    with np.errstate(over="ignore", invalid="ignore"):
        g = np.floor((v - o) / h)
    assert g.dtype == np.float32
    return g


def decimate(verts, tris, cell, origin=(0.0, 0.0, 0.0), placement="mean", stats=None):
    """-> (verts [n', 3] float32, tris [m', 3] int32, vmap [n] int32: the output id of every vertex's cluster, or -1).  stats, a dict,
    receives the numbers of collapsed and duplicate triangles dropped and of clusters."""
    v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(tris, np.int64).reshape(-1, 3)
    n_v = v.shape[0]
    mode = {"mean": 0, "member": 1}[placement]
    if not (np.isfinite(np.float32(cell)) and np.float32(cell) > 0) or not np.isfinite(np.asarray(origin, np.float32)).all():
        raise Refused("cell or origin")
    if t.shape[0] and (t.min() < 0 or t.max() >= n_v):
        raise Refused("a vertex index outside 0 .. n_v - 1")

    # MEMBERS
    member = np.zeros(n_v, bool)
    member[t.reshape(-1)] = True
    ids = np.flatnonzero(member)
    x = v[ids]
    if not np.isfinite(x).all():
        raise Refused("a member with a non-finite component")
    # CELL
    g = cells(x, origin, cell)
    if not (np.isfinite(g).all() and (g >= GRID_MIN).all() and (g <= GRID_MAX).all()):
        raise Refused("a member outside the grid")
    # CLUSTER: members arrive in ascending id, so the first member np.unique meets of a cell is the smallest
    rep = np.full(n_v, -1, np.int64)
    if ids.shape[0]:
        _, first, inverse = np.unique(g.astype(np.int64), axis=0, return_index=True, return_inverse=True)
        rep[ids] = ids[first[inverse.reshape(-1)]]
    # TRIANGLES
    r = rep[t]
    alive = (r[:, 0] != r[:, 1]) & (r[:, 1] != r[:, 2]) & (r[:, 0] != r[:, 2]) if t.shape[0] else np.zeros(0, bool)
    keep_t = np.zeros(t.shape[0], bool)
    idx = np.flatnonzero(alive)
    if idx.shape[0]:
        _, first = np.unique(np.sort(r[idx], axis=1), axis=0, return_index=True)  # the first occurrence: the smallest input index
        keep_t[idx[first]] = True
    # VERTICES
    keep_v = np.zeros(n_v, bool)
    keep_v[r[keep_t].reshape(-1)] = True
    new_id = np.cumsum(keep_v) - keep_v
    reps = np.flatnonzero(keep_v)
    vmap = np.where(rep >= 0, np.where(keep_v[np.maximum(rep, 0)], new_id[np.maximum(rep, 0)], -1), -1).astype(np.int32)
    out_t = new_id[r[keep_t]].astype(np.int32).reshape(-1, 3)
    if stats is not None:
        stats.update(collapsed=int((~alive).sum()), duplicates=int(alive.sum() - keep_t.sum()), clusters=int(np.unique(rep[ids]).shape[0]))

    # POSITION, placement 0
    out_v = v[reps].copy()  # one member, or M == 0: the representative's bytes
    M = float(np.abs(x).max()) if ids.shape[0] else 0.0
    n = np.zeros(n_v, np.int64)
    np.add.at(n, rep[ids], 1)
    if M > 0.0 and reps.shape[0]:
        E = int(np.frexp(M)[1]) - 1  # floor(log2 M)
        prod = x.astype(np.float64) * float(np.ldexp(1.0, 30 - E))
        assert (np.abs(prod) < 2.0 ** 31).all()
        q = np.rint(prod).astype(np.int64)  # round-half-even
        A = np.zeros((n_v, 3), np.int64)
        np.add.at(A, rep[ids], q)
        many = n[reps] > 1
        p = (A[reps].astype(np.float64) * float(np.ldexp(1.0, E - 30))) / n[reps].astype(np.float64)[:, None]
        out_v[many] = p[many].astype(np.float32)
    # POSITION, placement 1
    if mode == 1 and reps.shape[0]:
        in_out = keep_v[rep[ids]]
        mid, mx = ids[in_out], x[in_out]
        row = new_id[rep[mid]]
        with np.errstate(over="ignore"):
            d = mx - out_v[row]
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        assert d2.dtype == np.float32
        word = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | mid.astype(np.uint64)
        best = np.full(reps.shape[0], np.iinfo(np.uint64).max, np.uint64)
        np.minimum.at(best, row, word)
        out_v = v[(best & np.uint64(0xffffffff)).astype(np.int64)].copy()
    return out_v, out_t, vmap


def signed_volume(verts, tris):
    """the volume a closed, outward-oriented mesh encloses (float64)"""
    p = np.asarray(verts, np.float64)[np.asarray(tris, np.int64)]
    return float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)
