#!/usr/bin/env python3
"""tools/mesh_render_probe.py [--out JSON] [--kernels-only] [--voxel V]: what the mesh render costs (mvs_engine_mesh_render,
mvs_engine_mesh_visibility and mvs_engine_mesh_colours_visible, include/mvskit_engine.h).

Input: the bench scene, pool, lattice and mesh of tools/mesh_probe.py (12 views 1920x1080 `multi`), the mesh as extracted and decimated
on a grid of 8 voxels (decimate_mesh, placement mean).
1. Per mesh: Engine.render_mesh (every map comes down to the host), the same call with the counts alone (no map leaves the device),
   Engine.mesh_visibility, and Engine.mesh_colours with that visibility beside Engine.mesh_colours without: ms per call, the median of 5
   after a warm-up call (host clock around the call, which ends in a synchronise); covered pixels and skipped triangles per view; the
   triangles per view that go through the list to the wave-per-triangle kernel (mvs_engine_mesh_render_lists, the device's own count,
   held against tests/mesh_render_reading.py on the device's screen positions); the vertices' visible views.
2. The counts-only render with MVS_MRENDER_SMALL = 16, 32, 64, 256 in the environment (the clipped box a lane rasterises itself; the
   engine reads it at every call), the list lengths of each.
3. --kernels-only: a warm-up and one call of each on the decimated mesh, for a run under `rocprofv3 --kernel-trace --stats -- python
   tools/mesh_render_probe.py --kernels-only` (the k_mrender_* rows of the kernel statistics).
Without --out the result goes to profiles/rNN_mesh_render.json, NN = one more than the highest round number in profiles/.  No time is gated."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")]
from mesh_probe import DEPTH0, NCC0, next_round  # noqa: E402

SMALL = (16, 32, 64, 256)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--voxel", type=float, default=0.01)
    a = ap.parse_args()
    import mesh_render_reading as rr
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
    del pts
    verts, tris = e.mesh(vol)
    dverts, dtris, _ = e.decimate_mesh(verts, tris, 8 * a.voxel, engine.decimation_origin(vol))
    meshes = {"as extracted": (verts, tris), "decimated at 8 voxels": (dverts, dtris)}

    def median_ms(f):
        f()
        ms = []
        for _ in range(5):
            t = time.perf_counter()
            f()
            ms.append((time.perf_counter() - t) * 1e3)
        return float(np.median(ms)), [round(x, 2) for x in ms]

    def counts_only(v, t):
        cov, skip = np.zeros(sc.nviews, np.int64), np.zeros(sc.nviews, np.int64)
        e._check(e.L.mvs_engine_mesh_render(e.h, v.shape[0], v.ctypes.data_as(C.c_void_p), t.shape[0], t.ctypes.data_as(C.c_void_p), None, None, None,
                                            cov.ctypes.data_as(C.c_void_p), skip.ctypes.data_as(C.c_void_p)))
        return cov, skip

    if a.kernels_only:
        normals = e.mesh_normals(dverts, dtris)
        for _ in range(2):
            counts_only(dverts, dtris)
            vis = e.mesh_visibility(dverts, dtris)
            e.mesh_colours(dverts, normals, visible=vis)
        print(json.dumps(res))
        return

    res["meshes"] = {}
    for name, (v, t) in meshes.items():
        r = {"vertices": int(v.shape[0]), "triangles": int(t.shape[0])}
        normals = e.mesh_normals(v, t)
        cov, skip = counts_only(v, t)
        r["covered"], r["skipped"] = cov.tolist(), skip.tolist()
        screen, vdepth = e.mesh_screen(v, t)
        r["listed"] = {}
        for s in SMALL:  # the device's own count of its list, and the reading's from the device's screen positions
            os.environ["MVS_MRENDER_SMALL"] = str(s)
            r["listed"][str(s)] = e.mesh_render_lists(v, t).tolist()
            assert r["listed"][str(s)] == [rr.listed(screen[k], vdepth[k], t, sc.W, sc.H, s) for k in range(sc.nviews)], s
        del os.environ["MVS_MRENDER_SMALL"]
        del screen, vdepth
        vis = e.mesh_visibility(v, t)
        r["visible_views_histogram"] = np.bincount([bin(int(w)).count("1") for w in vis], minlength=sc.nviews + 1).tolist()
        used0 = e.mesh_colours(v, normals)[1]
        used1 = e.mesh_colours(v, normals, visible=vis)[1]
        r["views_blended_histogram"] = {"maps": np.bincount(used0 & 0x7F).tolist(), "maps_and_mesh": np.bincount(used1 & 0x7F).tolist()}
        for key, f in (("render_mesh_ms", lambda: e.render_mesh(v, t)), ("render_counts_only_ms", lambda: counts_only(v, t)),
                       ("mesh_visibility_ms", lambda: e.mesh_visibility(v, t)), ("mesh_colours_ms", lambda: e.mesh_colours(v, normals)),
                       ("mesh_colours_visible_ms", lambda: e.mesh_colours(v, normals, visible=vis))):
            r[key], r[key + "_all"] = median_ms(f)
        r["render_counts_only_ms_by_small"] = {}
        for s in SMALL:
            os.environ["MVS_MRENDER_SMALL"] = str(s)
            r["render_counts_only_ms_by_small"][str(s)] = median_ms(lambda: counts_only(v, t))
        del os.environ["MVS_MRENDER_SMALL"]
        res["meshes"][name] = r
    e.close()
    print(json.dumps(res))
    out = a.out or os.path.join(ROOT, "profiles", f"r{next_round():02d}_mesh_render.json")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
