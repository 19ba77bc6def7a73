"""The device headers of mvskit_amd/csrc are cut by concern ("The device sources are cut by concern"): every header
compiles on its own, the units that do not sample a patch cannot reach the patch arithmetic through any chain of includes, and no
header grows back into a monolith.  CPU only: hipcc parses the headers for gfx950, nothing runs."""
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

from mvskit_amd import build

CSRC = build.CSRC
INCLUDE = os.path.join(build.ROOT, "include")

# body files by design: text included more than once inside a unit, not a header
#   mvs_mesh_attr_colours.cuh -- the body of k_mattr_colours / k_mattr_colours_vis, included twice by mvs_mesh_attr.hip
BODY_FILES = {"mvs_mesh_attr_colours.cuh"}

# the cut of mvs_device.cuh, in include order
CUT = ["mvs_math.cuh", "mvs_wave.cuh", "mvs_camera.cuh", "mvs_sample.cuh", "mvs_eval.cuh", "mvs_cand.cuh", "mvs_refine.cuh"]
# the patch side: the arithmetic of a patch and everything built on it
PATCH_SIDE = {"mvs_sample.cuh", "mvs_eval.cuh", "mvs_cand.cuh", "mvs_refine.cuh", "mvs_check.cuh", "mvs_device.cuh", "mvs_patch_common.cuh",
              "mvs_seed_chain.cuh", "mvs_sweep.cuh", "mvs_filter.cuh", "mvs_probe.cuh"}
# the sources that do not sample a patch
NON_SAMPLING = ["mvs_image.hip", "mvs_index.hip", "mvs_maps.hip", "mvs_seed.hip", "mvs_mesh.hip", "mvs_mesh_attr.hip", "mvs_mesh_attr_colours.cuh",
                "mvs_mesh_clean.hip", "mvs_mesh_decimate.hip", "mvs_mesh_fill.hip", "mvs_mesh_render.hip", "mvs_mesh_common.cuh", "mvs_common.cuh",
                "mvs_ply.hip"]


def _headers():
    return sorted(f for f in os.listdir(CSRC) if f.endswith((".cuh", ".h")))


def _includes(name):
    with open(os.path.join(CSRC, name)) as f:
        return re.findall(r'^\s*#\s*include\s+"([^"]+)"', f.read(), flags=re.M)


def _closure(name):
    seen, todo = set(), [name]
    while todo:
        for inc in _includes(todo.pop()):
            if inc not in seen and os.path.exists(os.path.join(CSRC, inc)):
                seen.add(inc)
                todo.append(inc)
    return seen


def test_every_header_stands_alone(tmp_path):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    lang = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    jobs = []
    for h in _headers():
        if h in BODY_FILES:
            continue
        src = tmp_path / (h.replace(".", "_") + ".hip")
        src.write_text(f'#include "{h}"\n')
        for cap in (16, 64):
            jobs.append((h, cap, [hipcc] + lang + build.CAP_FLAGS[cap] + ["--cuda-device-only", "-fsyntax-only", "-I", INCLUDE, "-I", CSRC,
                                                                          "-x", "hip", str(src)]))

    def run(job):
        h, cap, cmd = job
        r = subprocess.run(cmd, capture_output=True, text=True)
        return h, cap, r.returncode, r.stderr

    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        results = list(pool.map(run, jobs))
    failed = [f"{h} (cap {cap}): exit {rc}\n{err[-1500:]}" for h, cap, rc, err in results if rc != 0]
    assert len(results) == 2 * (len(_headers()) - len(BODY_FILES))
    assert not failed, "\n".join(failed)


def test_layers():
    for unit in NON_SAMPLING:
        reached = _closure(unit) & PATCH_SIDE
        assert not reached, f"{unit} reaches the patch side: {sorted(reached)}"
    assert not (_closure("mvs_ply.hip") & (set(CUT) | PATCH_SIDE | {"mvs_common.cuh"}))  # the PLY writer shares nothing with them
    patch = _closure("mvs_patch.hip")
    assert set(CUT) | {"mvs_device.cuh", "mvs_check.cuh"} <= patch, sorted((set(CUT) | {"mvs_device.cuh", "mvs_check.cuh"}) - patch)
    # the seeding units that score hypotheses stay on the patch side
    for unit in ("mvs_seed_points.hip", "mvs_seed_random.hip"):
        assert "mvs_device.cuh" in _closure(unit)
    # the umbrella includes the cut in order and defines nothing
    assert _includes("mvs_device.cuh") == CUT
    with open(os.path.join(CSRC, "mvs_device.cuh")) as f:
        text = f.read()
    assert not re.search(r"\bDEV\s|__global__|__device__", text)


def test_no_header_outgrows_its_concern():
    for h in _headers():
        if not h.endswith(".cuh"):
            continue
        with open(os.path.join(CSRC, h)) as f:
            n = sum(1 for _ in f)
        assert n <= 800, f"{h}: {n} lines"
        if h == "mvs_device.cuh":
            assert n <= 60, f"mvs_device.cuh is the umbrella (comment + includes): {n} lines"
