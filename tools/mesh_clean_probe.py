#!/usr/bin/env python3
"""tools/mesh_clean_probe.py [--out JSON] [--kernels-only] [--voxel V] [--no-reading]: what the clean-up of a mesh finds and costs
(mvs_engine_mesh_components, mvs_engine_mesh_prune, mvs_engine_mesh_smooth and Engine.coloured_mesh with clean-up on,
include/mvskit_engine.h).

Input: the bench scene, pool and lattice of tools/mesh_probe.py -- 12 views 1920x1080 `multi`, ground-truth seeds (stride 2), then 3
iterations of Propagate::run, Filter::run, updateThreshold; the volume is engine.volume_around the fused points at --voxel world units
(default 0.01), trunc 4 voxels; the mesh is Engine.mesh of that volume.
1. The components of that mesh: their number, the size of the largest, the histogram of the others' sizes (triangles, by powers of two),
   the unused vertices.
2. Engine.mesh_components, Engine.prune_mesh (largest_only, with its size call), Engine.smooth_mesh (10 default iterations) and
   Engine.coloured_mesh(largest_only=True, smooth_iterations=10): ms per call, the median of 5 after a warm-up call (host clock around
   the call, which ends in a synchronise).
3. Beside them the numpy reading of tests/mesh_clean_reading.py on the same mesh, one run each, and whether its bytes are the engine's
   (--no-reading leaves it out; the fields are then listed as not measured).
4. --kernels-only: a warm-up and one call of each, for a run under `rocprofv3 --kernel-trace --stats -- python tools/mesh_clean_probe.py
   --kernels-only` (the k_mclean_* and k_msmooth_* rows of the kernel statistics).
Without --out the result goes to profiles/r19_mesh_clean.json.  No time is gated."""
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
    n_v = verts.shape[0]
    res["vertices"], res["triangles"] = int(n_v), int(tris.shape[0])
    label, ntris, n_comp = e.mesh_components(n_v, tris)  # warm-up too
    roots = (label == np.arange(n_v)) & (ntris > 0)
    sizes = np.sort(ntris[roots])[::-1]
    res["components"], res["unused_vertices"] = int(n_comp), int((ntris == 0).sum())
    res["largest_triangles"] = int(sizes[0]) if sizes.size else 0
    rest = sizes[1:]
    # the others by size: [2^k, 2^(k+1)) triangles -> how many components
    res["rest_histogram"] = {f"{1 << k}..{(2 << k) - 1}": int(((rest >= 1 << k) & (rest < 2 << k)).sum()) for k in range(0, 31)
                             if ((rest >= 1 << k) & (rest < 2 << k)).any()}
    pv, pt, _ = e.prune_mesh(verts, tris, largest_only=True)
    res["pruned_vertices"], res["pruned_triangles"] = int(pv.shape[0]), int(pt.shape[0])
    sv = e.smooth_mesh(verts, tris)
    calls = {"mesh_components": lambda: e.mesh_components(n_v, tris), "prune_mesh": lambda: e.prune_mesh(verts, tris, largest_only=True),
             "smooth_mesh": lambda: e.smooth_mesh(verts, tris), "coloured_mesh_clean": lambda: e.coloured_mesh(vol, largest_only=True, smooth_iterations=10),
             "coloured_mesh_plain": lambda: e.coloured_mesh(vol)}
    calls["coloured_mesh_clean"]()
    calls["coloured_mesh_plain"]()
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
    reading = ("reading_components_ms", "reading_prune_ms", "reading_smooth_ms", "reading_same_bytes")
    if a.no_reading:
        res["not_measured"] = list(reading)
    else:
        import mesh_clean_reading as cr

        t = time.perf_counter()
        rl, rn, rc = cr.components(n_v, tris)
        res[reading[0]] = (time.perf_counter() - t) * 1e3
        t = time.perf_counter()
        rv, rt, _ = cr.prune(verts, tris, 1, True)
        res[reading[1]] = (time.perf_counter() - t) * 1e3
        t = time.perf_counter()
        rs = cr.smooth_exact(verts, tris)
        res[reading[2]] = (time.perf_counter() - t) * 1e3
        res[reading[3]] = bool(rl.tobytes() == label.tobytes() and rn.tobytes() == ntris.tobytes() and rc == n_comp and rv.tobytes() == pv.tobytes()
                               and rt.tobytes() == pt.tobytes() and rs.tobytes() == sv.tobytes())
        res["not_measured"] = []
    print(json.dumps(res))
    out = a.out or os.path.join(ROOT, "profiles", "r19_mesh_clean.json")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
