#!/usr/bin/env python3
"""tools/seed_points_probe.py [--out JSON] [--kernels-only] [--hypotheses K] [--stride S]: what a warm start costs and what it is worth
(mvs_engine_seed_points and mvs_engine_depth_ranges, include/mvskit_engine.h).

Input: the bench scene -- 12 views 1920x1080 `multi`, synth.make_scene with the arguments of bench.load_scene.  The "sparse" cloud is the
ground-truth surface point of every 8th pixel in x and y of every view, concatenated (the finite ones); K = 4, min_ncc =
nccThresholdBefore: the call's defaults.
1. mvs_engine_seed_points: ms per call, the median of 5 after a warm-up call (host clock around the call, which ends in a synchronise;
   the pool is cleared in between), patches kept; mvs_engine_depth_ranges likewise.
2. --kernels-only: a warm-up and one call of each, for a run under `rocprofv3 --kernel-trace --stats -- python
   tools/seed_points_probe.py --kernels-only` (the k_seed_points* and k_depth_ranges rows of the kernel statistics).
3. The same pool as a user had to make it before these calls existed, timed: the hypotheses built in numpy (the gate, the order and the
   normals in float64, rounded to float32), then mvs_engine_probe's ops 1, 0, 2 and 3 with their host round trips, numpy picking the
   winners in between, and an upload of what is left.  (numpy's float64 normals are not the device's float32 ones to the last bit, so
   the two pools are compared by their sizes, not by their bytes.)
4. The 3-iteration schedule of bench.py (Propagate::run, Filter::run, updateThreshold) from the warm start's pool, and beside it the
   same schedule from bench.py's ground-truth seeds (synth.make_seeds, stride 2): alive patches after every iteration and
   tools/quality_probe.py's distance to the analytic surface."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
NCC0, NCC_BEFORE0, DEPTH0 = 0.7, 0.4, 1  # bench.py


def numpy_hypotheses(sc, pts, K, dtype):
    """steps 1 and 2 on the host (level 0, no masks): -> (records [n * K], count [n])"""
    X = pts.astype(np.float64)
    n, nv = X.shape[0], sc.nviews
    ok = np.zeros((n, nv), bool)
    dist = np.full((n, nv), np.inf)
    centers = np.zeros((nv, 3))
    for v in range(nv):
        P = sc.P[v].astype(np.float64)
        x = X @ P[:, :3].T + P[:, 3]
        with np.errstate(divide="ignore", invalid="ignore"):
            fx, fy = np.floor(x[:, 0] / x[:, 2] + 0.5), np.floor(x[:, 1] / x[:, 2] + 0.5)
        ok[:, v] = (x[:, 2] > 0) & (fx >= 0) & (fx < sc.W) & (fy >= 0) & (fy < sc.H)
        centers[v] = -np.linalg.solve(P[:, :3], P[:, 3])
        dist[ok[:, v], v] = ((centers[v] - X[ok[:, v]]) ** 2).sum(axis=1)
    count = np.minimum(ok.sum(axis=1), K).astype(np.int32)
    order = np.argsort(dist, axis=1, kind="stable")[:, :K]
    rec = np.zeros((n, K), dtype)
    t = centers[order] - X[:, None, :]
    t /= np.linalg.norm(t, axis=2, keepdims=True)
    rec["coord"][:, :, :3] = pts[:, None, :]
    rec["coord"][:, :, 3] = 1
    rec["normal"][:, :, :3] = t
    rec["normal"][:, :, 3] = -(X[:, None, :] * t).sum(axis=2)
    rec["ncc"] = -1
    rec["nimages"] = 1
    rec["flags"] = 1
    rec["id"] = np.arange(K)[None, :]
    rec["images"][:, :, 0] = order
    live = np.arange(K)[None, :] < count[:, None]
    rec[~live] = np.zeros((), dtype)
    return rec.reshape(-1), count


def parent_way(e, sc, pts, K):
    """the pool of seed_points by the calls of the commit before it -> (ms by stage, patches)"""
    from mvskit_amd import engine

    ms = {}
    t = time.perf_counter()
    hyp, count = numpy_hypotheses(sc, pts, K, e.dtype)
    ms["numpy_hypotheses"] = (time.perf_counter() - t) * 1e3
    t = time.perf_counter()
    n = pts.shape[0]
    slot = (np.arange(K)[None, :] < count[:, None]).ravel()
    idx = np.nonzero(slot)[0]
    p, _, f = e.probe(engine.PROBE_PREPROCESS, hyp[idx])
    ms["probe_preprocess"] = (time.perf_counter() - t) * 1e3
    t = time.perf_counter()
    _, s, _ = e.probe(engine.PROBE_NCC, p)
    ms["probe_ncc"] = (time.perf_counter() - t) * 1e3
    t = time.perf_counter()
    flag = np.ones(n * K, np.int32)
    ncc = np.full(n * K, np.nan, np.float32)
    where = np.full(n * K, -1)
    flag[idx], ncc[idx], where[idx] = f, s, np.arange(idx.size)
    best = np.full(n, np.float32(e.thresholds()[1]), np.float32)
    win = np.full(n, -1)
    for k in range(K):
        with np.errstate(invalid="ignore"):
            take = slot[k::K] & (flag[k::K] == 0) & (ncc[k::K] > best)
        best[take] = ncc[k::K][take]
        win[take] = k
    who = np.nonzero(win >= 0)[0]
    batch = np.repeat(p[:1], n)
    batch[who] = p[where[who * K + win[who]]]
    ms["numpy_winners"] = (time.perf_counter() - t) * 1e3
    t = time.perf_counter()
    ref, _, _ = e.probe(engine.PROBE_REFINE, batch)
    ms["probe_refine"] = (time.perf_counter() - t) * 1e3
    t = time.perf_counter()
    post, _, pflag = e.probe(engine.PROBE_POSTPROCESS, ref)
    ms["probe_postprocess"] = (time.perf_counter() - t) * 1e3
    t = time.perf_counter()
    keep = post[who[pflag[who] == 0]]
    e.upload_patches(keep)
    ms["upload"] = (time.perf_counter() - t) * 1e3
    ms["total"] = sum(ms.values())
    return {k: round(v, 1) for k, v in ms.items()}, int(keep.shape[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--hypotheses", type=int, default=4)
    ap.add_argument("--stride", type=int, default=8)
    a = ap.parse_args()
    from mvskit_amd import engine, synth
    from seed_random_probe import quality, schedule

    t0 = time.perf_counter()
    sc = synth.make_scene(nviews=12, W=1920, H=1080, arc_deg=110.0, radius=4.0, kind="multi")
    s = a.stride
    pts = np.concatenate([sc.points[v, s // 2::s, s // 2::s].reshape(-1, 3) for v in range(sc.nviews)])
    pts = np.ascontiguousarray(pts[np.isfinite(pts).all(axis=1)], dtype=np.float32)
    res = {"views": sc.nviews, "width": sc.W, "height": sc.H, "hypotheses": a.hypotheses, "stride": s, "points": int(pts.shape[0]),
           "scene_s": round(time.perf_counter() - t0, 1)}
    e = engine.Engine(sc.nviews, level=0, csize=2, wsize=7, minImageNum=3, enable_check=1, seed=1, nccThreshold=NCC0, depth=DEPTH0)
    e.set_scene(sc)

    def call():
        e.clear_patches()
        e.set_thresholds(NCC0, NCC_BEFORE0, DEPTH0)
        t = time.perf_counter()
        n = e.seed_points(pts, hypotheses=a.hypotheses)
        return (time.perf_counter() - t) * 1e3, n

    def ranges():
        t = time.perf_counter()
        r = e.depth_ranges(pts)
        return (time.perf_counter() - t) * 1e3, r

    _, n = call()  # warm-up
    _, (lo, hi, cnt) = ranges()
    res["patches"] = n
    res["points_seeded"] = n / max(pts.shape[0], 1)
    res["depth_min"] = [round(float(x), 3) for x in lo]
    res["depth_max"] = [round(float(x), 3) for x in hi]
    res["depth_count"] = [int(x) for x in cnt]
    if a.kernels_only:
        call()
        ranges()
        print(json.dumps(res))
        return
    ms = [call()[0] for _ in range(5)]
    res["call_ms"] = float(np.median(ms))
    res["call_ms_all"] = [round(x, 1) for x in ms]
    res["points_per_s"] = pts.shape[0] / (res["call_ms"] * 1e-3)
    ms = [ranges()[0] for _ in range(5)]
    res["depth_ranges_ms"] = float(np.median(ms))
    res["depth_ranges_ms_all"] = [round(x, 2) for x in ms]
    res["warm_start_pool"] = quality(sc, e.patches())
    res["warm_start_schedule"] = schedule(e, sc)
    # the same pool by the calls of the commit before: once to warm up, once timed
    for _ in range(2):
        e.clear_patches()
        e.set_thresholds(NCC0, NCC_BEFORE0, DEPTH0)
        res["parent_way_ms"], res["parent_way_patches"] = parent_way(e, sc, pts, a.hypotheses)
    res["parent_way_over_call"] = res["parent_way_ms"]["total"] / res["call_ms"]
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
