#!/usr/bin/env python3
"""tools/export_probe.py [--out JSON] [--parent-host LIB]: what PatchManager::writePly costs (patch_manager.cpp:542-633).

1. mvs_engine_export_ply on the bench's pool -- 12 views 1920x1080 `multi` (bench.py's scene, loaded through bench.load_scene), seeds
   one per 2x2 cells, after PmMvps::run's three iterations (Propagate::run + Filter::run + updateThreshold): ms per call for ASCII and
   binary (median of 5 calls with the size known, plus the size query), bytes, GB/s of file written, and the share a device-to-host
   copy of the same number of bytes into pageable host memory takes of the call.
2. The host mirror's writePly on the same scene, this tree's library against another build's (--parent-host: a libmvskit_host.so
   built from the parent revision against tools/build_variant.sh's engine): mvshost_run (three iterations, final pool written once)
   timed with and without mvshost_set_ply_output, each in a process of its own; the difference is one writePly.
3. The six refined_patches*.ply files of PmMvps::run (mvshost_run_dataset, three iterations) on a small dataset on disk, written by
   both libraries and compared byte for byte (--parent-host only).
"""
import argparse
import ctypes as C
import filecmp
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

NCC0, NCC_BEFORE0, DEPTH0 = 0.7, 0.4, 1  # as bench.py
ITERS = 3


def bench_scene():
    import bench

    args = argparse.Namespace(views=12, width=1920, height=1080, seed_stride=2, scene_cache=os.path.join("/tmp", "mvskit_scene_cache"))
    return bench.load_scene(args, 0)


def engine_probe():
    import torch

    from mvskit_amd import engine

    sc, seeds = bench_scene()
    e = engine.Engine(sc.nviews, level=0, csize=2, wsize=7, minImageNum=3, enable_check=1, seed=1, nccThreshold=NCC0, depth=DEPTH0)
    e.set_scene(sc)
    e.reserve(0)
    e.upload_patches(seeds)
    e.set_thresholds(NCC0, NCC_BEFORE0, DEPTH0)
    for it in range(ITERS):
        e.propagate(it)
        e.filter()
        e.update_threshold()
    torch.cuda.synchronize()
    res = {"pool_alive": e.num_patches()}
    for name, fmt in (("ascii", engine.PLY_ASCII), ("binary", engine.PLY_BINARY_LE)):
        n = C.c_int64()
        t0 = time.perf_counter()
        assert e.L.mvs_engine_export_ply(e.h, fmt, 0, None, C.byref(n)) == 0
        query_ms = 1000.0 * (time.perf_counter() - t0)
        buf = np.empty(n.value, np.uint8)
        ms = []
        for _ in range(5):
            t0 = time.perf_counter()
            assert e.L.mvs_engine_export_ply(e.h, fmt, n.value, buf.ctypes.data_as(C.c_void_p), C.byref(n)) == 0
            ms.append(1000.0 * (time.perf_counter() - t0))
        # the copy alone: the same bytes from device memory into pageable host memory
        dev = torch.empty(n.value, dtype=torch.uint8, device="cuda")
        host = np.empty(n.value, np.uint8)
        ht = torch.from_numpy(host)
        ht.copy_(dev)
        d2h = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ht.copy_(dev)
            torch.cuda.synchronize()
            d2h.append(1000.0 * (time.perf_counter() - t0))
        del dev
        med = float(np.median(ms))
        res[name] = {"bytes": int(n.value), "ms_per_call": med, "size_query_ms": query_ms, "GB_per_s": n.value / med / 1e6,
                     "d2h_copy_ms": float(np.median(d2h)), "d2h_share": float(np.median(d2h)) / med, "calls_ms": ms}
    e.close()
    return res


def mirror_once(host_lib, ply_path):
    """One mvshost_run of the bench scene (three iterations), with the final pool written to ply_path or not: seconds."""
    import torch  # noqa: F401  (torch's HIP runtime first, as mvskit_amd.engine loads it)

    L = C.CDLL(host_lib)
    L.mvshost_set_ply_output.argtypes = [C.c_char_p]
    L.mvshost_set_ply_output.restype = None
    L.mvshost_run.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_uint,
                              C.c_int, C.c_longlong, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p]
    sc, seeds = bench_scene()
    P = np.ascontiguousarray(sc.P, dtype=np.float32)
    img = np.ascontiguousarray(sc.images)
    sd = np.ascontiguousarray(seeds)
    nout, ptot = C.c_longlong(), C.c_longlong()
    L.mvshost_set_ply_output(ply_path.encode() if ply_path else b"")
    t0 = time.perf_counter()
    r = L.mvshost_run(sc.nviews, sc.W, sc.H, P.ctypes.data, img.ctypes.data, 0, 2, 7, 3, C.c_float(NCC0), 1, ITERS, sd.shape[0], sd.ctypes.data,
                      0, None, C.byref(nout), C.byref(ptot))
    dt = time.perf_counter() - t0
    assert r == 0, r
    return {"seconds": dt, "pool": int(nout.value), "ply_bytes": os.path.getsize(ply_path) if ply_path else 0}


def write_dataset(root):
    from mvskit_amd import synth

    sc = synth.make_scene(nviews=3, W=320, H=240, arc_deg=30.0, radius=4.0, kind="plane")
    seeds = synth.make_seeds(sc, stride=4, seed=21)
    for d in ("txt", "image", "ply"):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    with open(os.path.join(root, "option"), "w") as f:
        f.write(f"level 0\ncsize 2\nthreshold 0.7\nwsize 7\nminImageNum 2\nimages -1 0 {sc.nviews}\n")
    for v in range(sc.nviews):
        with open(os.path.join(root, "txt", f"{v:08d}.txt"), "w") as f:
            f.write("CONTOUR\n" + "\n".join(" ".join(repr(float(x)) for x in row) for row in sc.P[v]) + "\n")
        with open(os.path.join(root, "image", f"{v:04d}0000.ppm"), "wb") as f:
            f.write(b"P6\n%d %d\n255\n" % (sc.W, sc.H))
            f.write(np.ascontiguousarray(sc.images[v]).tobytes())
    with open(os.path.join(root, "ply", "00000000.patch"), "w") as f:
        f.write(f"PATCHES\n{seeds.shape[0]}\n")
        for r in seeds:
            f.write("PATCHS\n" + " ".join(repr(float(x)) for x in r["coord"]) + "\n" + " ".join(repr(float(x)) for x in r["normal"]) + "\n")
            f.write(f"{float(r['ncc'])!r} {float(r['dscale'])!r} {float(r['ascale'])!r}\n{int(r['nimages'])}\n")
            f.write(" ".join(str(int(x)) for x in r["images"][: r["nimages"]]) + "\n0\n\n")


def dataset_once(host_lib, root):
    import torch  # noqa: F401

    L = C.CDLL(host_lib)
    L.mvshost_run_dataset.argtypes = [C.c_char_p, C.c_int, C.c_uint, C.c_longlong, C.c_void_p, C.c_void_p]
    n = C.c_longlong()
    assert L.mvshost_run_dataset((root.rstrip("/") + "/").encode(), ITERS, 9, 0, None, C.byref(n)) == 0
    return {"pool": int(n.value)}


def child(kind, *a):
    """Runs one mirror measurement in a fresh process (two engine libraries never share one)."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", kind, *a], capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(r.stdout[-2000:] + r.stderr[-4000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-host", default=None, help="libmvskit_host.so of the parent revision (and its engine beside it)")
    ap.add_argument("--child", nargs="+", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        kind, lib, path = args.child[0], args.child[1], (args.child[2] if len(args.child) > 2 else "")
        print(json.dumps(mirror_once(lib, path) if kind == "mirror" else dataset_once(lib, path)))
        return
    from mvskit_amd import build

    res = {"scene": "bench.py's: 12 views 1920x1080 multi, seeds 1 per 2x2 cells, after three iterations of Propagate::run + Filter::run",
           "export_ply": engine_probe()}
    libs = {"this": build.build_host()}
    if args.parent_host:
        libs["parent"] = os.path.abspath(args.parent_host)
    tmp = tempfile.mkdtemp(prefix="export_probe_")
    res["mirror_writePly"] = {}
    for name, lib in libs.items():
        without = child("mirror", lib)
        with_ = child("mirror", lib, os.path.join(tmp, f"{name}.ply"))
        res["mirror_writePly"][name] = {"run_s_without_ply": without["seconds"], "run_s_with_ply": with_["seconds"],
                                        "writePly_ms": 1000.0 * (with_["seconds"] - without["seconds"]), "pool": with_["pool"], "ply_bytes": with_["ply_bytes"]}
    if "parent" in libs:
        res["mirror_writePly"]["same_file"] = filecmp.cmp(os.path.join(tmp, "this.ply"), os.path.join(tmp, "parent.ply"), shallow=False)
        files = {}
        for name, lib in libs.items():
            root = os.path.join(tmp, f"data_{name}")
            write_dataset(root)
            child("dataset", lib, root)
            files[name] = root
        names = [f"refined_patches{s}_{it}.ply" for it in range(ITERS) for s in ("_before_refine", "")]
        res["pmmvps_run_six_plys"] = {n: filecmp.cmp(os.path.join(files["this"], "ply", n), os.path.join(files["parent"], "ply", n), shallow=False)
                                      for n in names}
    res["not_measured"] = "configs[3] (48 views of 3840x2160, ~26 M patches alive): not run by this probe"
    print(json.dumps(res, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
