"""The meshes of the hole-filling tests (tests/test_mesh_fill_reading.py on the CPU, tests/test_gpu_mesh_fill.py on the GPU): the sphere of
the prune test with triangles taken out or put in, and a flat grid whose rim is longer than a block.  Built once per process."""
import functools

import numpy as np

import mesh_reading as mr
from scene_support import grid_mesh

CENTRE = np.array([8.3, 9.6, 10.2], np.float32)


@functools.lru_cache(maxsize=None)
def sphere():
    """2146 vertices, 4288 triangles, closed, valences 4 to 9"""
    dims = (24, 20, 20)
    verts, tris = mr.extract((0.0, 0.0, 0.0), 1.0, dims, mr.sphere_volume(dims, [tuple(float(c) for c in CENTRE)], 6.2))
    verts.setflags(write=False)
    tris.setflags(write=False)
    return verts, tris


def around(tris, v):
    """the rows of the triangles that name vertex v"""
    return (tris == v).any(axis=1)


def ring(tris, v):
    """the neighbours of v"""
    return np.setdiff1d(tris[around(tris, v)], [v])


def touching_vertex(tris, v):
    """the smallest k that is no neighbour of v and whose ring shares exactly one vertex with v's ring"""
    rv = ring(tris, v)
    for k in range(int(tris.max()) + 1):
        if k != v and k not in rv and np.intersect1d(ring(tris, k), rv).shape[0] == 1:
            return k
    raise AssertionError("no such vertex")


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (verts, tris, (n_loops, n_complex, n_irregular), the sorted lengths of the components (negative: complex), max_edges,
    (new vertices, new triangles, n_filled) of a fill with that max_edges)"""
    verts, tris = sphere()
    t0 = tris[0]
    first_neighbour = int(ring(tris, 500).min())
    k = touching_vertex(tris, 500)
    gv, gt = grid_mesh(70, 70)
    out = {
        "closed": (verts, tris, (0, 0, 0), [], 64, (0, 0, 0)),
        "one_triangle_out": (verts, np.delete(tris, 100, axis=0), (1, 0, 0), [3], 64, (0, 1, 1)),
        "two_rings_out": (verts, tris[~(around(tris, 500) | around(tris, 1500))], (2, 0, 0), [6, 6], 64, (2, 12, 2)),
        "two_adjacent_rings_out": (verts, tris[~(around(tris, 500) | around(tris, first_neighbour))], (1, 0, 0), [9], 64, (1, 9, 1)),
        "two_holes_meet_in_a_vertex": (verts, tris[~(around(tris, 500) | around(tris, k))], (0, 1, 0), [-12], 64, (0, 0, 0)),
        "first_triangle_twice": (verts, np.concatenate([tris, tris[:1]]), (0, 0, 3), [], 64, (0, 0, 0)),
        "fin": (verts, np.concatenate([tris, [[t0[0], t0[1], 2000]]]).astype(np.int32), (0, 1, 1), [-2], 64, (0, 0, 0)),
        "grid_rim_kept": (gv, gt, (1, 0, 0), [276], 275, (0, 0, 0)),
        "grid_rim_filled": (gv, gt, (1, 0, 0), [276], 276, (1, 276, 1)),
    }
    for c in out.values():
        c[0].setflags(write=False)
        c[1].setflags(write=False)
    return out


def component_lengths(loop, length):
    """the sorted lengths of the components, one entry each"""
    loop, length = np.asarray(loop), np.asarray(length)
    roots = np.flatnonzero(loop == np.arange(loop.shape[0]))
    return sorted(int(x) for x in length[roots])


def fan(n=20000):
    """the fan of the decimation test: around vertex 0, its rim wobbling between radius 0.7 and 1.3"""
    a = np.linspace(0.0, 2 * np.pi, n - 1, endpoint=False)
    r = 1.0 + 0.3 * np.sin(7 * a)
    rim = np.stack([r * np.cos(a), r * np.sin(a), 0.05 * np.cos(3 * a)], 1)
    verts = np.concatenate([[[0.0, 0.0, 0.0]], rim]).astype(np.float32)
    i = np.arange(1, n)
    tris = np.stack([np.zeros(n - 1, np.int64), i, np.where(i + 1 < n, i + 1, 1)], 1).astype(np.int32)
    return verts, tris
