#!/usr/bin/env python3
"""tools/mesh_seams_probe.py [--out JSON] [--voxel V] [--no-reading]: what the seam calls do and cost (mvs_engine_mesh_adjacency,
mvs_engine_mesh_face_quality, mvs_engine_mesh_smooth_labels, mvs_engine_mesh_seam_levels, mvs_engine_mesh_texture_levelled;
include/mvskit_seams.h).

Input: the bench scene, pool, lattice and mesh of tools/mesh_probe.py (12 views 1920x1080 `multi`), the mesh as extracted (atlas at res 8)
and decimated on a grid of 8 voxels (res 32), both in an atlas 4096 wide, labelled by Engine.mesh_face_views under Engine.mesh_visibility.
1. Per mesh: the seams before and after Engine.smooth_face_views at keep 128 / 192 / 240 with the moves and the iterations used; at keep
   192 the seam edges, the pair table's sample counts and the offsets of Engine.seam_levels; ms per call of the five, the median of 5
   after a warm-up call (host clock around the call, which ends in a synchronise).
2. The reading of each call (tests/mesh_seams_reading.py) on the device's own screen positions and pyramid levels, timed once, and
   whether its bytes are the device's.  The smoothing's reading is a Python loop over the triangles: it runs on the decimated mesh only
   (--no-reading leaves all of it out).
Without --out the result goes to profiles/rNN_mesh_seams.json, NN = one more than the highest round number in profiles/.  No time is gated."""
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
LOOP_READING_MAX = 50000  # triangles up to which the Python loop of the smoothing's reading is run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--no-reading", action="store_true")
    ap.add_argument("--voxel", type=float, default=0.01)
    a = ap.parse_args()
    import mesh_render_reading as rr
    import mesh_seams_reading as sr
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
        return round(float(np.median(ms)), 2)

    def timed(f):
        t = time.perf_counter()
        out = f()
        return out, round((time.perf_counter() - t) * 1e3, 1)

    res["meshes"] = {}
    for name, (v, t, r_) in meshes.items():
        r = {"vertices": int(v.shape[0]), "triangles": int(t.shape[0]), "res": r_}
        vis = e.mesh_visibility(v, t)
        label = e.mesh_face_views(v, t, visible=vis)[0]
        nbr, r["n_irregular"] = e.mesh_adjacency(v.shape[0], t)
        quality = e.mesh_face_quality(v, t, visible=vis)
        r["smoothing"] = {}
        for keep in (128, 192, 240):
            out, stats = e.smooth_face_views(t, quality, label, keep=keep)
            r["smoothing"][str(keep)] = dict(zip(("seams_before", "seams_after", "moves", "iterations"), stats.tolist()))
            if keep == 192:
                smooth = out
        offset, pairs, r["seam_edges"] = e.seam_levels(v, t, smooth)
        r["offsets_sixteenths"], r["pair_samples"] = offset.tolist(), int(pairs[:, :, 0].sum() // 2)
        r["seam_edges_unsmoothed"] = e.seam_levels(v, t, label)[2]
        atlas, uv, ntex = e.texture_mesh_levelled(v, t, smooth, offset, res=r_, width=WIDTH)
        r["atlas"] = [int(atlas.shape[0]), WIDTH]
        for key, f in (("mesh_adjacency_ms", lambda: e.mesh_adjacency(v.shape[0], t)), ("mesh_face_quality_ms", lambda: e.mesh_face_quality(v, t, visible=vis)),
                       ("smooth_face_views_ms", lambda: e.smooth_face_views(t, quality, label)), ("seam_levels_ms", lambda: e.seam_levels(v, t, smooth)),
                       ("texture_mesh_levelled_ms", lambda: e.texture_mesh_levelled(v, t, smooth, offset, res=r_, width=WIDTH)),
                       ("texture_mesh_ms", lambda: e.texture_mesh(v, t, smooth, res=r_, width=WIDTH))):
            r[key] = median_ms(f)
        if not a.no_reading:
            screen, vdepth = e.mesh_screen(v, t)
            screens, vdepths = list(screen), list(vdepth)
            images = [e.pyramid(k, 0) for k in range(sc.nviews)]
            signs = [tr.front_sign(rr.camera64(sc.P[k], 0)) for k in range(sc.nviews)]
            want, r["reading_adjacency_ms"] = timed(lambda: sr.adjacency(v.shape[0], t))
            r["reading_adjacency_equal"] = bool(want[0].tobytes() == nbr.tobytes() and want[1] == r["n_irregular"])
            want, r["reading_face_quality_ms"] = timed(lambda: sr.face_quality(screens, vdepths, t, [(sc.W, sc.H)] * sc.nviews, signs, visible=vis))
            r["reading_face_quality_equal"] = bool(want.tobytes() == quality.tobytes())
            if t.shape[0] <= LOOP_READING_MAX:
                want, r["reading_smooth_labels_ms"] = timed(lambda: sr.smooth_labels(v.shape[0], t, quality, label, 192, 64))
                r["reading_smooth_labels_equal"] = bool(want[0].tobytes() == smooth.tobytes())
            want, r["reading_seam_levels_ms"] = timed(lambda: sr.seam_levels(screens, vdepths, t, smooth, images))
            r["reading_seam_levels_equal"] = bool(want[0].tobytes() == offset.tobytes() and want[1].tobytes() == pairs.tobytes() and want[2] == r["seam_edges"])
            want, r["reading_texture_levelled_ms"] = timed(lambda: sr.texture_levelled(screens, vdepths, t, smooth, images, offset, r_, WIDTH))
            r["reading_texture_levelled_equal"] = bool(want["atlas"].tobytes() == atlas.tobytes() and want["uv"].tobytes() == uv.tobytes())
            del screen, vdepth, screens, vdepths, images, want
        print(name, json.dumps(r), flush=True)
        res["meshes"][name] = r
    e.close()
    print(json.dumps(res))
    out = a.out or os.path.join(ROOT, "profiles", f"r{next_round():02d}_mesh_seams.json")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
