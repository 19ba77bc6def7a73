#!/usr/bin/env python3
"""tools/mesh_fill_probe.py [--out JSON] [--kernels-only] [--voxel V] [--no-reading]: the boundary loops of the bench mesh, what hole
filling closes of them and what it costs (mvs_engine_mesh_boundaries and mvs_engine_mesh_fill, include/mvskit_engine.h).

Input: the bench scene, pool and lattice of tools/mesh_probe.py -- 12 views 1920x1080 `multi`, ground-truth seeds (stride 2), then 3
iterations of Propagate::run, Filter::run, updateThreshold; the volume is engine.volume_around the fused points at --voxel world units
(default 0.01), trunc 4 voxels; the mesh is Engine.mesh of that volume, as it comes and pruned to its largest component.
1. Per mesh: vertices, triangles, the three counts of Engine.mesh_boundaries and a histogram of the loop lengths (3, 4, 5-8, 9-16, 17-64,
   65-256, 257 and more).
2. Per mesh and max_edges of 16, 64 and 256: loops filled, vertices and triangles added, and the counts of the filled mesh.
3. ms per call of Engine.mesh_boundaries and of Engine.fill_holes at max_edges 64 (the size call and the full call together, as
   Engine.fill_holes makes them), the median of 5 after a warm-up call (host clock around the call, which ends in a synchronise).
4. Beside them the numpy reading of tests/mesh_fill_reading.py on the same mesh, one run, and whether its bytes are the engine's
   (--no-reading leaves it out; the fields are then listed as not measured).
5. --kernels-only: two rounds of one call of each on the pruned mesh (the first is the warm-up), for a run under `rocprofv3 --kernel-trace --stats -- python
   tools/mesh_fill_probe.py --kernels-only` (the k_mfill_* rows of the kernel statistics).
Without --out the result goes to profiles/r24_mesh_fill.json.  No time is gated."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")]
NCC0, DEPTH0 = 0.7, 1  # bench.py
BINS = ((3, 3), (4, 4), (5, 8), (9, 16), (17, 64), (65, 256), (257, 1 << 31))


def histogram(loop, length):
    lengths = length[(loop == np.arange(loop.shape[0])) & (length > 0)]
    return {(f"{lo}" if lo == hi else f"{lo}+" if hi > 1 << 30 else f"{lo}-{hi}"): int(((lengths >= lo) & (lengths <= hi)).sum()) for lo, hi in BINS}


def median_ms(call):
    call()  # warm-up
    ms = []
    for _ in range(5):
        t = time.perf_counter()
        out = call()
        ms.append((time.perf_counter() - t) * 1e3)
    return out, float(np.median(ms)), [round(x, 2) for x in ms]


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
    pv, pt, _ = e.prune_mesh(verts, tris, 1, True)
    if a.kernels_only:
        for _ in range(2):
            e.mesh_boundaries(pv.shape[0], pt)
            e.fill_holes(pv, pt, 64)
        print(json.dumps(res))
        return
    if not a.no_reading:
        import mesh_fill_reading as fr
    res["meshes"] = []
    for name, v, t in (("as extracted", verts, tris), ("largest component", pv, pt)):
        n_v = v.shape[0]
        found, b_ms, b_all = median_ms(lambda: e.mesh_boundaries(n_v, t))
        loop, length, n_loops, n_complex, n_irregular = found
        m = {"mesh": name, "vertices": int(n_v), "triangles": int(t.shape[0]), "n_loops": n_loops, "n_complex": n_complex, "n_irregular": n_irregular,
             "loop_lengths": histogram(loop, length), "longest_loop": int(length.max()) if n_v else 0, "boundaries_ms": b_ms, "boundaries_ms_all": b_all,
             "fills": []}
        for k in (16, 64, 256):
            fv, ft, nf = e.fill_holes(v, t, k)
            after = e.mesh_boundaries(fv.shape[0], ft)
            m["fills"].append({"max_edges": k, "filled": nf, "vertices_added": int(fv.shape[0] - n_v), "triangles_added": int(ft.shape[0] - t.shape[0]),
                               "n_loops_after": after[2], "n_complex_after": after[3], "n_irregular_after": after[4]})
        got, m["fill_ms"], m["fill_ms_all"] = median_ms(lambda: e.fill_holes(v, t, 64))
        if not a.no_reading:
            t1 = time.perf_counter()
            want_b = fr.boundaries(n_v, t)
            m["reading_boundaries_ms"] = (time.perf_counter() - t1) * 1e3
            t1 = time.perf_counter()
            want_f = fr.fill(v, t, 64)
            m["reading_fill_ms"] = (time.perf_counter() - t1) * 1e3
            m["reading_same_bytes"] = bool(want_b[0].tobytes() == loop.tobytes() and want_b[1].tobytes() == length.tobytes() and
                                           want_b[2:] == found[2:] and want_f[0].tobytes() == got[0].tobytes() and
                                           want_f[1].tobytes() == got[1].tobytes() and want_f[2] == got[2])
        res["meshes"].append(m)
    e.close()
    res["not_measured"] = ["reading_boundaries_ms", "reading_fill_ms", "reading_same_bytes"] if a.no_reading else []
    print(json.dumps(res))
    out = a.out or os.path.join(ROOT, "profiles", "r24_mesh_fill.json")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
