#!/usr/bin/env python3
"""tools/mesh_probe.py [--out JSON] [--kernels-only] [--voxel V]: what the triangle mesh costs (mvs_engine_tsdf, mvs_engine_extract_mesh
and mvs_engine_mesh, include/mvskit_engine.h).

Input: the bench scene and pool of tools/maps_probe.py -- 12 views 1920x1080 `multi`, ground-truth seeds (stride 2), then 3 iterations of
Propagate::run, Filter::run, updateThreshold.  The volume is engine.volume_around the fused points at --voxel world units (default 0.01,
about six pixel footprints: the scene then takes some 10^7 lattice points; the limit is 2^28), trunc 4 voxels.
1. Engine.tsdf (the volume into host arrays), Engine.extract_mesh on that volume (the volume goes back up, the size call, the mesh comes
   down), Engine.mesh (size call and full call: the volume stays on the device but both calls fuse it) and Engine.mesh with caps an
   eighth above the mesh (one call, one fusion): ms per call, the median of 5 after a warm-up call (host clock around the call, which
   ends in a synchronise); lattice points, observed points, vertices, triangles.
2. --kernels-only: a warm-up and one call of each, for a run under `rocprofv3 --kernel-trace --stats -- python tools/mesh_probe.py
   --kernels-only` (the k_mesh_* rows of the kernel statistics).
Without --out the result goes to profiles/rNN_mesh.json, NN = one more than the highest round number in profiles/.  No time is gated."""
import argparse
import glob
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
NCC0, DEPTH0 = 0.7, 1  # bench.py


def next_round():
    rounds = [int(m.group(1)) for p in glob.glob(os.path.join(ROOT, "profiles", "r*")) for m in [re.match(r"r(\d+)_", os.path.basename(p))] if m]
    return max(rounds, default=0) + 1


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
    res["fused_points"] = int(pts.shape[0])
    vol = engine.volume_around(pts["xyz"], a.voxel)
    res["dims"] = list(vol.dims[:])
    res["lattice_points"] = int(np.prod(vol.dims[:], dtype=np.int64))
    del pts

    def timed(f):
        t = time.perf_counter()
        r = f()
        return (time.perf_counter() - t) * 1e3, r

    tsdf, count = e.tsdf(vol)  # warm-up, and the volume that extract_mesh takes
    res["observed_points"] = int((count >= 1).sum())
    calls = {"tsdf": lambda: e.tsdf(vol), "extract_mesh": lambda: e.extract_mesh(vol, tsdf, count), "mesh": lambda: e.mesh(vol)}
    verts, tris = calls["mesh"]()
    calls["mesh_with_caps"] = lambda: e.mesh(vol, cap_v=verts.shape[0] + verts.shape[0] // 8, cap_t=tris.shape[0] + tris.shape[0] // 8)
    res["vertices"], res["triangles"] = int(verts.shape[0]), int(tris.shape[0])
    calls["extract_mesh"]()
    if a.kernels_only:
        for f in calls.values():
            f()
        print(json.dumps(res))
        return
    for k, f in calls.items():
        ms = [timed(f)[0] for _ in range(5)]
        res[k + "_ms"] = float(np.median(ms))
        res[k + "_ms_all"] = [round(x, 1) for x in ms]
    e.close()
    print(json.dumps(res))
    out = a.out or os.path.join(ROOT, "profiles", f"r{next_round():02d}_mesh.json")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
