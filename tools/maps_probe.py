#!/usr/bin/env python3
"""tools/maps_probe.py [--out JSON] [--kernels-only] [--source S]: what the dense maps and their fusion cost
(mvs_engine_render_maps and mvs_engine_fused_points, include/mvskit_engine.h).

Input: the bench scene -- 12 views 1920x1080 `multi`, synth.make_scene with the arguments of bench.load_scene -- and the pool after
bench.py's schedule: ground-truth seeds (synth.make_seeds, stride 2), then 3 iterations of Propagate::run, Filter::run, updateThreshold.
1. mvs_engine_render_maps into host arrays (all five maps of all views) and the count-only call (n_valid, no map leaves the device),
   mvs_engine_fused_points' size call and its full call: ms per call, the median of 5 after a warm-up call (host clock around the call,
   which ends in a synchronise); valid pixels per view, the agreeing-views histogram, the points emitted.
2. --kernels-only: a warm-up and one call of each, for a run under `rocprofv3 --kernel-trace --stats -- python tools/maps_probe.py
   --kernels-only` (the k_maps_* rows of the kernel statistics).
3. The only route to the same depth maps before these calls existed, timed: mvs_engine_depth_normal_map once per view (kind 1 for
   source 0), then the planes evaluated per pixel in numpy (float64) from the downloaded patches.  Depth only: no agreement, no fusion."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
NCC0, NCC_BEFORE0, DEPTH0 = 0.7, 0.4, 1  # bench.py


def parent_way(e, sc, source):
    """the depth map of every view by the calls of the commit before -> (ms by stage, valid pixels per view)"""
    ms = {}
    t = time.perf_counter()
    alive = e.patches()
    pat = np.zeros(int(alive["id"].max()) + 1 if alive.shape[0] else 1, alive.dtype)
    pat[alive["id"]] = alive
    ms["download_patches"] = (time.perf_counter() - t) * 1e3
    csize, level = e.cfg.csize, e.cfg.level
    grids, valid = [], []
    t = time.perf_counter()
    for v in range(sc.nviews):
        grids.append(e.depth_normal_map(v, 1 if source == 0 else 0)[2])
    ms["depth_normal_map"] = (time.perf_counter() - t) * 1e3
    t = time.perf_counter()
    for v in range(sc.nviews):
        H, W = e.level_shape(v)
        P = sc.P[v].astype(np.float64)
        P[:2] /= 2.0 ** level
        Minv = np.linalg.inv(P[:, :3])
        C = -Minv @ P[:, 3]
        o = P[2] / np.linalg.norm(P[2, :3])
        ids = np.repeat(np.repeat(grids[v], csize, axis=0), csize, axis=1)[:H, :W]
        y, x = np.mgrid[0:H, 0:W]
        sel = np.maximum(ids, 0)
        n = pat["normal"][sel][..., :3].astype(np.float64)
        X0 = pat["coord"][sel][..., :3].astype(np.float64)
        d = np.stack([x, y, np.ones_like(x)], axis=-1).astype(np.float64) @ Minv.T
        with np.errstate(divide="ignore", invalid="ignore"):
            tt = (n * (X0 - C)).sum(-1) / (n * d).sum(-1)
            depth = (C + tt[..., None] * d) @ o[:3] + o[3]
            ok = (ids >= 0) & (tt > 0) & (depth > 0) & np.isfinite(depth)
        valid.append(int(ok.sum()))
    ms["numpy_planes"] = (time.perf_counter() - t) * 1e3
    ms["total"] = sum(ms.values())
    return {k: round(v, 1) for k, v in ms.items()}, valid


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--source", type=int, default=0)
    a = ap.parse_args()
    from mvskit_amd import engine, synth

    t0 = time.perf_counter()
    sc = synth.make_scene(nviews=12, W=1920, H=1080, arc_deg=110.0, radius=4.0, kind="multi")
    res = {"views": sc.nviews, "width": sc.W, "height": sc.H, "source": a.source, "scene_s": round(time.perf_counter() - t0, 1)}
    e = engine.Engine(sc.nviews, level=0, csize=2, wsize=7, minImageNum=3, enable_check=1, seed=1, nccThreshold=NCC0, depth=DEPTH0)
    e.set_scene(sc)
    e.upload_patches(synth.make_seeds(sc, level=0, csize=2, stride=2, seed=777))
    for it in range(3):
        e.propagate(it)
        e.filter()
        e.update_threshold()
    res["pool"] = e.num_patches()

    def timed(f):
        t = time.perf_counter()
        r = f()
        return (time.perf_counter() - t) * 1e3, r

    calls = {"render_maps": lambda: e.render_maps(source=a.source), "valid_pixels": lambda: e.valid_pixels(source=a.source),
             "fused_points": lambda: e.fused_points(source=a.source)}
    out = {k: timed(f)[1] for k, f in calls.items()}  # warm-up
    res["valid_pixels"] = [int(x) for x in out["valid_pixels"]]
    agree = np.concatenate([m["agree"][m["ids"] >= 0] for m in out["render_maps"]])
    pop = np.unpackbits(agree.view(np.uint8).reshape(-1, 8), axis=1).sum(1)
    res["agreeing_views_histogram"] = np.bincount(pop, minlength=sc.nviews)[:sc.nviews].tolist()
    res["fused_points"] = int(out["fused_points"].shape[0])
    if a.kernels_only:
        for f in calls.values():
            f()
        print(json.dumps(res))
        return
    del out, agree, pop
    for k, f in calls.items():
        ms = [timed(f)[0] for _ in range(5)]
        res[k + "_ms"] = float(np.median(ms))
        res[k + "_ms_all"] = [round(x, 1) for x in ms]
    for _ in range(2):  # once to warm up, once timed
        res["parent_way_ms"], res["parent_way_valid_pixels"] = parent_way(e, sc, a.source)
    res["parent_way_over_render_maps"] = res["parent_way_ms"]["total"] / res["render_maps_ms"]
    e.close()
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
