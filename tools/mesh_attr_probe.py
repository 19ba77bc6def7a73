#!/usr/bin/env python3
"""tools/mesh_attr_probe.py [--out JSON] [--kernels-only] [--voxel V]: what the vertex normals and colours of a mesh cost
(mvs_engine_mesh_normals, mvs_engine_mesh_colours and Engine.coloured_mesh, include/mvskit_engine.h).

Input: the bench scene, pool and lattice of tools/mesh_probe.py -- 12 views 1920x1080 `multi`, ground-truth seeds (stride 2), then 3
iterations of Propagate::run, Filter::run, updateThreshold; the volume is engine.volume_around the fused points at --voxel world units
(default 0.01), trunc 4 voxels; the mesh is Engine.mesh of that volume.
1. Engine.mesh_normals (the mesh goes up, the normals come down), Engine.mesh_colours with those normals (the maps are rendered, the
   vertices go up, colours and `used` come down) and Engine.coloured_mesh (mesh with its size call, then the two): ms per call, the median
   of 5 after a warm-up call (host clock around the call, which ends in a synchronise); vertices, triangles, and how many vertices
   were coloured from confirmed views, from unconfirmed ones, and not at all.
2. --kernels-only: a warm-up and one call of each, for a run under `rocprofv3 --kernel-trace --stats -- python tools/mesh_attr_probe.py
   --kernels-only` (the k_mattr_* rows of the kernel statistics).
Without --out the result goes to profiles/r17_mesh_attr.json.  No time is gated."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
NCC0, DEPTH0 = 0.7, 1  # bench.py


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--voxel", type=float, default=0.01)
    a = ap.parse_args()
    from mvskit_amd import engine, synth

    t0 = time.perf_counter()
    sc = synth.make_scene(nviews=12, W=1920, H=1080, arc_deg=110.0, radius=4.0, kind="multi")
    res = {"views": sc.nviews, "width": sc.W, "height": sc.H, "voxel": a.voxel, "scene_s": round(time.perf_counter() - t0, 1)}
    e = engine.Engine(sc.nviews, level=0, csize=2, wsize=7, minImageNum=3, enable_check=1, seed=1, nccThreshold=NCC0, depth=DEPTH0)
    e.set_scene(sc)
    e.upload_patches(synth.make_seeds(sc, level=0, csize=2, stride=2, seed=777))
    for it in range(3):
        e.propagate(it)
        e.filter()
        e.update_threshold()
    res["pool"] = e.num_patches()
    pts = e.fused_points()
    vol = engine.volume_around(pts["xyz"], a.voxel)
    res["dims"] = list(vol.dims[:])
    res["lattice_points"] = int(np.prod(vol.dims[:], dtype=np.int64))
    del pts
    verts, tris = e.mesh(vol)
    res["vertices"], res["triangles"] = int(verts.shape[0]), int(tris.shape[0])
    normals = e.mesh_normals(verts, tris)  # warm-up, and the normals that mesh_colours takes
    rgb, used = e.mesh_colours(verts, normals)
    res["confirmed"], res["unconfirmed"], res["uncoloured"] = int((used >= 0x80).sum()), int(((used > 0) & (used < 0x80)).sum()), int((used == 0).sum())
    calls = {"mesh_normals": lambda: e.mesh_normals(verts, tris), "mesh_colours": lambda: e.mesh_colours(verts, normals),
             "coloured_mesh": lambda: e.coloured_mesh(vol)}
    calls["coloured_mesh"]()
    if a.kernels_only:
        for f in calls.values():
            f()
        print(json.dumps(res))
        return
    for k, f in calls.items():
        ms = []
        for _ in range(5):
            t = time.perf_counter()
            f()
            ms.append((time.perf_counter() - t) * 1e3)
        res[k + "_ms"] = float(np.median(ms))
        res[k + "_ms_all"] = [round(x, 1) for x in ms]
    e.close()
    print(json.dumps(res))
    out = a.out or os.path.join(ROOT, "profiles", "r17_mesh_attr.json")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
