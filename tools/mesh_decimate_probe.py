#!/usr/bin/env python3
"""tools/mesh_decimate_probe.py [--out JSON] [--kernels-only] [--voxel V] [--no-reading]: what vertex clustering makes of the bench mesh
and what it costs (mvs_engine_mesh_decimate, include/mvskit_engine.h).

Input: the bench scene, pool and lattice of tools/mesh_probe.py -- 12 views 1920x1080 `multi`, ground-truth seeds (stride 2), then 3
iterations of Propagate::run, Filter::run, updateThreshold; the volume is engine.volume_around the fused points at --voxel world units
(default 0.01), trunc 4 voxels; the mesh is Engine.mesh of that volume.
1. Engine.decimate_mesh at cells of 2, 4 and 8 voxels on the grid Engine.coloured_mesh uses (engine.decimation_origin), both placements:
   vertices and triangles out, collapsed and duplicate triangles dropped, ms per call (the size call and the full call together, as
   Engine.decimate_mesh makes them), the median of 5 after a warm-up call (host clock around the call, which ends in a synchronise).
2. Beside each the numpy reading of tests/mesh_decimate_reading.py on the same mesh, one run, and whether its bytes are the engine's
   (--no-reading leaves it out; the fields are then listed as not measured, and so are the dropped triangles, which the reading counts).
3. --kernels-only: a warm-up and one call of each, for a run under `rocprofv3 --kernel-trace --stats -- python
   tools/mesh_decimate_probe.py --kernels-only` (the k_mdec_* rows of the kernel statistics).
Without --out the result goes to profiles/r21_mesh_decimate.json.  No time is gated."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")]
NCC0, DEPTH0 = 0.7, 1  # bench.py


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--no-reading", action="store_true")
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
    del pts
    verts, tris = e.mesh(vol)
    res["vertices"], res["triangles"] = int(verts.shape[0]), int(tris.shape[0])
    origin = engine.decimation_origin(vol)
    res["origin"] = list(origin)
    cases = [(k, p) for k in (2, 4, 8) for p in ("mean", "member")]
    e.decimate_mesh(verts, tris, 2 * float(np.float32(vol.voxel)), origin)  # warm-up
    if a.kernels_only:
        for k, p in cases:
            e.decimate_mesh(verts, tris, k * float(np.float32(vol.voxel)), origin, p)
        print(json.dumps(res))
        return
    res["cases"] = []
    got = {}
    for k, p in cases:
        cell = k * float(np.float32(vol.voxel))
        ms = []
        for _ in range(5):
            t = time.perf_counter()
            got[k, p] = e.decimate_mesh(verts, tris, cell, origin, p)
            ms.append((time.perf_counter() - t) * 1e3)
        v, t, _ = got[k, p]
        res["cases"].append({"cell_voxels": k, "cell": cell, "placement": p, "vertices_out": int(v.shape[0]), "triangles_out": int(t.shape[0]),
                             "ms": float(np.median(ms)), "ms_all": [round(x, 1) for x in ms]})
    e.close()
    reading = ("collapsed", "duplicates", "reading_ms", "reading_same_bytes")
    if a.no_reading:
        res["not_measured"] = list(reading)
    else:
        import mesh_decimate_reading as dr

        for c in res["cases"]:
            st = {}
            t = time.perf_counter()
            want = dr.decimate(verts, tris, c["cell"], origin, c["placement"], stats=st)
            c["reading_ms"] = (time.perf_counter() - t) * 1e3
            c["collapsed"], c["duplicates"] = st["collapsed"], st["duplicates"]
            c["reading_same_bytes"] = bool(all(w.tobytes() == g.tobytes() for w, g in zip(want, got[c["cell_voxels"], c["placement"]])))
        res["not_measured"] = []
    print(json.dumps(res))
    out = a.out or os.path.join(ROOT, "profiles", "r21_mesh_decimate.json")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
