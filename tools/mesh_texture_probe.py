#!/usr/bin/env python3
"""tools/mesh_texture_probe.py [--out JSON] [--kernels-only] [--voxel V] [--no-reading]: what the textured mesh costs
(mvs_engine_mesh_face_views and mvs_engine_mesh_texture, include/mvskit_texture.h).

Input: the bench scene, pool, lattice and mesh of tools/mesh_probe.py (12 views 1920x1080 `multi`), the mesh as extracted at res 8 and
decimated on a grid of 8 voxels (decimate_mesh, placement mean) at res 32, both in an atlas 4096 wide.
1. Per mesh: Engine.mesh_visibility, Engine.mesh_face_views with that visibility and Engine.texture_mesh (the size call and the full
   call: the atlas comes down to the host): ms per call, the median of 5 after a warm-up call (host clock around the call, which ends in
   a synchronise); the triangles per label, the untextured ones, the atlas size.
2. The numpy reading of both calls (tests/mesh_texture_reading.py) on the device's own screen positions and pyramid levels, timed once,
   and whether its labels, areas, texture coordinates and atlas bytes are the device's (--no-reading leaves it out).
3. --kernels-only: a warm-up and one call of each on the decimated mesh, for a run under `rocprofv3 --kernel-trace --stats -- python
   tools/mesh_texture_probe.py --kernels-only` (the k_mtex_* rows of the kernel statistics).
Without --out the result goes to profiles/rNN_mesh_texture.json, NN = one more than the highest round number in profiles/.  No time is gated."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")]
from mesh_probe import DEPTH0, NCC0, next_round  # noqa: E402

WIDTH = 4096


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--no-reading", action="store_true")
    ap.add_argument("--voxel", type=float, default=0.01)
    a = ap.parse_args()
    import mesh_render_reading as rr
    import mesh_texture_reading as tr
    from mvskit_amd import engine, synth

    t0 = time.perf_counter()
    sc = synth.make_scene(nviews=12, W=1920, H=1080, arc_deg=110.0, radius=4.0, kind="multi")
    res = {"views": sc.nviews, "width": sc.W, "height": sc.H, "voxel": a.voxel, "atlas_width": WIDTH, "scene_s": round(time.perf_counter() - t0, 1)}
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
    meshes = {"as extracted, res 8": (verts, tris, 8), "decimated at 8 voxels, res 32": (dverts, dtris, 32)}

    def median_ms(f):
        f()
        ms = []
        for _ in range(5):
            t = time.perf_counter()
            f()
            ms.append((time.perf_counter() - t) * 1e3)
        return float(np.median(ms)), [round(x, 2) for x in ms]

    if a.kernels_only:
        for _ in range(2):
            vis = e.mesh_visibility(dverts, dtris)
            label = e.mesh_face_views(dverts, dtris, visible=vis)[0]
            e.texture_mesh(dverts, dtris, label, res=32, width=WIDTH)
        print(json.dumps(res))
        return

    res["meshes"] = {}
    for name, (v, t, r_) in meshes.items():
        r = {"vertices": int(v.shape[0]), "triangles": int(t.shape[0]), "res": r_}
        vis = e.mesh_visibility(v, t)
        label, area, faces = e.mesh_face_views(v, t, visible=vis)
        atlas, uv, ntex = e.texture_mesh(v, t, label, res=r_, width=WIDTH)
        r["labels_per_view"], r["unlabelled"], r["untextured"] = faces.tolist(), int((label < 0).sum()), int(t.shape[0] - ntex)
        r["atlas"] = [int(atlas.shape[0]), WIDTH]
        r["atlas_texels_owned"] = int(ntex) * (r_ + 3) ** 2 // 2
        for key, f in (("mesh_visibility_ms", lambda: e.mesh_visibility(v, t)), ("mesh_face_views_ms", lambda: e.mesh_face_views(v, t, visible=vis)),
                       ("texture_mesh_ms", lambda: e.texture_mesh(v, t, label, res=r_, width=WIDTH))):
            r[key], r[key + "_all"] = median_ms(f)
        if not a.no_reading:
            screen, vdepth = e.mesh_screen(v, t)
            images = [e.pyramid(k, 0) for k in range(sc.nviews)]
            signs = [tr.front_sign(rr.camera64(sc.P[k], 0)) for k in range(sc.nviews)]
            t1 = time.perf_counter()
            want = tr.face_views(list(screen), list(vdepth), t, [(sc.W, sc.H)] * sc.nviews, signs, visible=vis)
            r["reading_face_views_ms"] = round((time.perf_counter() - t1) * 1e3, 1)
            r["reading_face_views_equal"] = bool(want[0].tobytes() == label.tobytes() and want[1].tobytes() == area.tobytes() and want[2].tobytes() == faces.tobytes())
            t1 = time.perf_counter()
            rd = tr.texture(list(screen), list(vdepth), t, label, images, r_, WIDTH)
            r["reading_texture_ms"] = round((time.perf_counter() - t1) * 1e3, 1)
            r["reading_texture_equal"] = bool(rd["atlas"].tobytes() == atlas.tobytes() and rd["uv"].tobytes() == uv.tobytes() and rd["n_textured"] == ntex)
            del screen, vdepth, images, rd
        print(name, json.dumps(r), flush=True)
        res["meshes"][name] = r
    e.close()
    print(json.dumps(res))
    out = a.out or os.path.join(ROOT, "profiles", f"r{next_round():02d}_mesh_texture.json")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
