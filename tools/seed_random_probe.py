#!/usr/bin/env python3
"""tools/seed_random_probe.py [--out JSON] [--kernels-only] [--hypotheses K]: what a cold start costs and what it is worth
(mvs_engine_seed_random, include/mvskit_engine.h).

Input: the bench scene -- 12 views 1920x1080 `multi`, synth.make_scene with the arguments of bench.load_scene, ground truth kept for
the depth ranges and the quality figures.  Per view the range is 0.5 x the smallest to 2 x the largest true depth along the optical
axis; K = 8, max_tilt pi / 3, min_ncc = nccThresholdBefore: the call's defaults.
1. mvs_engine_seed_random: ms per call, the median of 5 after a warm-up call (host clock around the call, which ends in a
   synchronise; the pool is cleared in between), patches kept, the share of the cells that got one.
2. --kernels-only: a warm-up and one call, for a run under `rocprofv3 --kernel-trace --stats -- python tools/seed_random_probe.py
   --kernels-only` (the k_seed_random* rows of the kernel statistics are the kernels' share).
3. The 3-iteration schedule of bench.py (Propagate::run, Filter::run, updateThreshold) from the cold start's pool, and beside it the
   same schedule from bench.py's ground-truth seeds (synth.make_seeds, stride 2): alive patches after every iteration and
   tools/quality_probe.py's distance to the analytic surface (relative depth error along the optical axis, normal angle)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
NCC0, NCC_BEFORE0, DEPTH0 = 0.7, 0.4, 1  # bench.py


def quality(sc, p):
    from quality_probe import patch_errors

    p = p[p["dscale"] > 0]
    if p.shape[0] == 0:
        return {"patches": 0}
    rel, ang = patch_errors(sc, p)
    return {"patches": int(p.shape[0]), "depth_rel_err_median": float(np.median(rel)), "depth_rel_err_p90": float(np.percentile(rel, 90)),
            "normal_deg_median": float(np.median(ang)), "normal_deg_p90": float(np.percentile(ang, 90)), "ncc_median": float(np.median(p["ncc"]))}


def schedule(e, sc, iters=3):
    rows = []
    for it in range(iters):
        t = time.perf_counter()
        c = e.propagate(it)
        removed = e.filter()
        e.update_threshold()
        row = {"iter": it, "s": round(time.perf_counter() - t, 3), "inserted": c["inserted"], "replaced": c["replaced"],
               "filter_removed": sum(removed.values()), "alive": e.num_patches()}
        row.update(quality(sc, e.patches()))
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--hypotheses", type=int, default=8)
    a = ap.parse_args()
    from mvskit_amd import engine, synth

    t0 = time.perf_counter()
    sc = synth.make_scene(nviews=12, W=1920, H=1080, arc_deg=110.0, radius=4.0, kind="multi")
    lo, hi = [], []
    for v in range(sc.nviews):
        X = sc.points[v].reshape(-1, 3).astype(np.float64)
        X = X[np.isfinite(X).all(axis=1)]
        P = sc.P[v].astype(np.float64)
        z = (X @ P[2, :3] + P[2, 3]) / np.linalg.norm(P[2, :3])
        lo.append(0.5 * z.min())
        hi.append(2.0 * z.max())
    res = {"views": sc.nviews, "width": sc.W, "height": sc.H, "hypotheses": a.hypotheses, "depth_min": [round(x, 3) for x in lo],
           "depth_max": [round(x, 3) for x in hi], "scene_s": round(time.perf_counter() - t0, 1)}
    e = engine.Engine(sc.nviews, level=0, csize=2, wsize=7, minImageNum=3, enable_check=1, seed=1, nccThreshold=NCC0, depth=DEPTH0)
    e.set_scene(sc)
    # the views are set without masks, so the gate drops only a cell whose centre pixel lies outside the image (level 0, csize 2: none
    # unless a side is odd); every other cell builds all K hypotheses
    cells = gated = 0
    for v in range(sc.nviews):
        gw, gh = e.grid_dims(v)
        cells += gw * gh
        gated += min(gw, sc.W // 2) * min(gh, sc.H // 2)  # centre pixel (2 cx + 1, 2 cy + 1) inside W x H

    def call():
        e.clear_patches()
        e.set_thresholds(NCC0, NCC_BEFORE0, DEPTH0)
        t = time.perf_counter()
        n = e.seed_random(lo, hi, hypotheses=a.hypotheses)
        return (time.perf_counter() - t) * 1e3, n

    _, n = call()  # warm-up
    res["cells"] = cells
    res["cells_gated"] = gated
    res["patches"] = n
    res["cells_seeded"] = n / cells
    if a.kernels_only:
        call()
        print(json.dumps(res))
        return
    ms = [call()[0] for _ in range(5)]
    res["call_ms"] = float(np.median(ms))
    res["call_ms_all"] = [round(x, 1) for x in ms]
    res["hypotheses_per_s"] = gated * a.hypotheses / (res["call_ms"] * 1e-3)
    res["cold_start_pool"] = quality(sc, e.patches())
    res["cold_start_schedule"] = schedule(e, sc)
    seeds = synth.make_seeds(sc, level=0, csize=2, stride=2, seed=777)
    e.clear_patches()
    e.set_thresholds(NCC0, NCC_BEFORE0, DEPTH0)
    e.upload_patches(seeds)
    res["ground_truth_seeds"] = int(seeds.shape[0])
    res["ground_truth_schedule"] = schedule(e, sc)
    e.close()
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
