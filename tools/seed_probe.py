#!/usr/bin/env python3
"""tools/seed_probe.py [--out JSON] [--kernels-only] [--no-cpu]: what DepthNormInit::createPatches' PLY branch costs
(depth_normal_init.cpp:34-91) on the device (mvs_engine_seed_patches) and on the path before it (the host mirror's CPU loop).

Input: the bench scene -- 12 views 1920x1080 `multi`, synth.make_scene with the arguments of bench.load_scene (which drops the
ground-truth geometry this probe needs) -- points = the ground-truth point of every second pixel in x and y of every view, maps =
the scene's normals with NaN -> 0, masks = where the scene has geometry.
1. mvs_engine_seed_patches: ms per call, median of 5 after a warm-up call (host clock around the call, which ends in a synchronise;
   the pool is cleared in between), points/s, patches appended.
2. Its host-to-device copies alone: the same arrays (pageable host memory) copied with torch, median of 5.
3. --kernels-only: a warm-up and one call, for a run under `rocprofv3 --kernel-trace --stats -- python tools/seed_probe.py
   --kernels-only` (the k_seed_* rows of the kernel statistics are the kernels' share).
4. The same stage at the parent revision: DepthNormInit::buildPatches' loop + PatchManager::addPatches on the same arrays, timed inside
   the mirror with std::chrono (mvshost_seed_cpu_probe / mvshost_seed_cpu_ms), one run.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def probe_input():
    from mvskit_amd import synth

    sc = synth.make_scene(nviews=12, W=1920, H=1080, arc_deg=110.0, radius=4.0, kind="multi")
    valid = ~np.isnan(sc.points).any(axis=3)
    pts = np.ascontiguousarray(np.concatenate([sc.points[v][::2, ::2][valid[v][::2, ::2]] for v in range(sc.nviews)]), dtype=np.float32)
    maps = np.ascontiguousarray(np.nan_to_num(sc.normals, nan=0.0), dtype=np.float32)
    masks = np.where(valid, 255, 0).astype(np.uint8)
    sc.points = sc.normals = None
    return sc, pts, maps, masks


def median(xs):
    return float(np.median(np.asarray(xs)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    import torch

    from mvskit_amd import build, engine

    t0 = time.perf_counter()
    sc, pts, maps, masks = probe_input()
    res = {"views": sc.nviews, "width": sc.W, "height": sc.H, "points": int(len(pts)), "scene_s": round(time.perf_counter() - t0, 1)}
    e = engine.Engine(sc.nviews, level=0, csize=2, wsize=7, minImageNum=3, enable_check=1, seed=1)
    e.set_scene(sc)
    views = (engine.SeedView * sc.nviews)()
    for v in range(sc.nviews):
        views[v].normals, views[v].mask = maps[v].ctypes.data, masks[v].ctypes.data
    added = C.c_int64()

    def call():
        e.clear_patches()
        t = time.perf_counter()
        r = e.L.mvs_engine_seed_patches(e.h, len(pts), pts.ctypes.data_as(C.c_void_p), views, C.byref(added))
        dt = time.perf_counter() - t
        assert r == 0, e.L.mvs_last_error()
        return dt * 1e3

    call()  # warm-up
    res["patches"] = int(added.value)
    if a.kernels_only:
        call()
        print(json.dumps(res))
        return
    ms = [call() for _ in range(5)]
    res["device_call_ms"] = median(ms)
    res["device_call_ms_all"] = [round(x, 2) for x in ms]
    res["device_points_per_s"] = len(pts) / (res["device_call_ms"] * 1e-3)

    def copies():
        torch.cuda.synchronize()
        t = time.perf_counter()
        keep = [torch.from_numpy(pts).cuda()]
        for v in range(sc.nviews):  # one view's map and mask at a time, as the call streams them
            keep = [torch.from_numpy(maps[v]).cuda(), torch.from_numpy(masks[v]).cuda()]
        torch.cuda.synchronize()
        del keep
        return (time.perf_counter() - t) * 1e3

    copies()
    hc = [copies() for _ in range(5)]
    res["h2d_copies_ms"] = median(hc)
    res["h2d_bytes"] = int(pts.nbytes + maps.nbytes + masks.nbytes)
    res["h2d_gb_per_s"] = res["h2d_bytes"] / (res["h2d_copies_ms"] * 1e-3) / 1e9
    e.close()
    if not a.no_cpu:
        host = C.CDLL(build.build_host())
        host.mvshost_seed_cpu_probe.restype = C.c_longlong
        host.mvshost_seed_cpu_probe.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_int]
        host.mvshost_seed_cpu_ms.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double)]
        P = np.ascontiguousarray(sc.P, dtype=np.float32)
        rgb = np.ascontiguousarray(sc.images, dtype=np.uint8)
        n = host.mvshost_seed_cpu_probe(sc.nviews, sc.W, sc.H, P.ctypes.data, rgb.ctypes.data, masks.ctypes.data, maps.ctypes.data, len(pts), pts.ctypes.data, 0)
        loop_ms, add_ms = C.c_double(), C.c_double()
        host.mvshost_seed_cpu_ms(C.byref(loop_ms), C.byref(add_ms))
        res["cpu_patches"] = int(n)
        res["cpu_build_loop_ms"] = loop_ms.value
        res["cpu_add_patches_ms"] = add_ms.value
        res["cpu_total_ms"] = loop_ms.value + add_ms.value
        res["cpu_points_per_s"] = len(pts) / (res["cpu_total_ms"] * 1e-3)
        res["cpu_over_device"] = res["cpu_total_ms"] / res["device_call_ms"]
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
