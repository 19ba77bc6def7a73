"""The RGBA8 pyramids of all views lie in ONE device allocation, level after level and view after view, and while it is below 4 GiB the
full-window sweep and the refine probe address its texels by the allocation's base plus a 32-bit byte offset per lane (the narrow
samplers); MVS_SAMPLER_WIDE=1, read on every launch, keeps the 64-bit address per lane that a larger block needs.
Both forms read the same texels, so they must give the same bytes.  What can go wrong is a level's offset, a carry from one view's
levels into the next view's, and the two ends of the block:

  1. five views of unequal, odd sizes: one Propagate::run with either form and on the CPU oracle (ENGINE schedule);
  2. every level of every view of that scene read back (mvs_engine_get_pyramid) against the numpy reading of the reference's
     pyramid filter (second_reading.ref_pyr_down): the levels lie where DView::img says, and none overlaps its neighbour;
  3. patches whose windows touch the last admissible row and column of the last level of the last view -- the end of the allocation --
     and the first admissible ones of the first view's level 0 -- its start: Optim::refinePatch through the refine probe, either form.

Engine.sampler_launches (mvs_engine_sampler_launches) says which form the launchers chose; every case asserts it."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

import oracle_binding as ob
from mvskit_amd import engine, synth
from parity_support import COUNTERS, pools_match_oracle, seeds_for_sizes
from second_reading import RefCam, ref_get_paxes, ref_project, ref_pyr_down

pytestmark = pytest.mark.gpu
F = np.float32

SIZES = [(97, 65), (96, 64), (81, 57), (97, 63), (89, 65)]  # odd and even sides; no two views alike
KW = dict(level=0, csize=2, wsize=7, minImageNum=2, seed=11, enable_check=1)
RECORD_FIELDS = ("coord", "normal", "ncc", "dscale", "ascale", "nimages", "images", "nvimages", "vimages")


@contextmanager
def _sampler(wide):
    """MVS_SAMPLER_WIDE around the engine calls of the block (False: unset), restored afterwards"""
    old = os.environ.pop("MVS_SAMPLER_WIDE", None)
    if wide:
        os.environ["MVS_SAMPLER_WIDE"] = "1"
    try:
        yield
    finally:
        os.environ.pop("MVS_SAMPLER_WIDE", None)
        if old is not None:
            os.environ["MVS_SAMPLER_WIDE"] = old


# ------------------------------------------------------------------ 1, 2: five views of unequal size
@pytest.fixture(scope="module")
def unequal():
    sc = synth.make_scene(nviews=5, W=97, H=65, arc_deg=30.0, radius=4.0, kind="multi")
    seeds = seeds_for_sizes(sc, synth.make_seeds(sc, stride=1, seed=5), SIZES, 0)
    assert seeds.shape[0] > 1000
    return sc, seeds


def _engine_pass(sc, seeds, wide):
    e = engine.Engine(sc.nviews, **KW)
    e.set_scene(sc, sizes=SIZES)
    with _sampler(wide):
        e.upload_patches(seeds)
        c = e.propagate(0)
        p = e.patches()
        launches = e.sampler_launches()
    e.close()
    return c, p, launches


@pytest.fixture(scope="module")
def oracle_pass(unequal):
    """the oracle's Propagate::run, computed once and left unchanged"""
    sc, seeds = unequal
    o = ob.Oracle(sc.nviews, schedule=ob.SCHEDULE_ENGINE, sum_mode=ob.SUM_TREE64, nthreads=8, **KW)
    o.set_scene(sc, sizes=SIZES)
    o.add_patches(seeds)
    c, p = o.propagate(0), o.patches()
    o.close()
    return c, p


def test_unequal_views_narrow_wide_and_oracle(unequal, oracle_pass):
    """One Propagate::run (two colour passes, a sweep launch each).  The two forms: the same ten counters and the same pool, byte for
    byte.  Either form and the oracle: the same ten counters, the same lists, and the records' fields equal bit for bit."""
    sc, seeds = unequal
    cn, pn, ln = _engine_pass(sc, seeds, wide=False)
    cw, pw, lw = _engine_pass(sc, seeds, wide=True)
    co, po = oracle_pass
    print("narrow", cn, ln)
    print("wide  ", cw, lw)
    print("oracle", co)
    assert ln["sweep_narrow"] == 2 and ln["sweep_wide"] == 0, ln
    assert lw["sweep_narrow"] == 0 and lw["sweep_wide"] == 2, lw
    assert len(COUNTERS) == 10
    for k in COUNTERS:
        assert cn[k] == cw[k] == co[k], (k, cn, cw, co)
    assert co["inserted"] > 1000 and co["patches"] > co["inserted"], co  # the pass expanded into every view
    assert pn.shape == pw.shape and pn.tobytes() == pw.tobytes()
    refs = np.bincount(pn["images"][:, 0], minlength=5)
    print("reference views", refs)
    assert refs.min() > 100, refs  # every view is the reference view of patches: every view's level offsets were used
    pools_match_oracle(po, pn)
    for f in RECORD_FIELDS:
        same = float(np.mean([a.tobytes() == b.tobytes() for a, b in zip(po[f], pn[f])]))
        print(f"{f}: {same:.4f} of {po.shape[0]} records bit-equal to the oracle's")
        np.testing.assert_array_equal(po[f], pn[f], err_msg=f)


def test_pyramid_readback_from_the_block(unequal):
    sc, _ = unequal
    e = engine.Engine(sc.nviews, **KW)
    e.set_scene(sc, sizes=SIZES)
    for v, (w, h) in enumerate(SIZES):
        want = np.ascontiguousarray(sc.images[v][:h, :w])
        for l in range(KW["level"] + 3):
            got = e.pyramid(v, l)
            assert got.shape == (h >> l, w >> l, 3), (v, l, got.shape)
            np.testing.assert_array_equal(got, want, err_msg=f"view {v} level {l}")
            want = ref_pyr_down(want)
    e.close()


# ------------------------------------------------------------------ 3: the ends of the block
END_SIZES = [(129, 97), (128, 96), (121, 89)]
ZOOM = 3.2  # the last view's focal length over the others': a patch of one pixel per sample in view 0 covers 3.2 there -> its level 2


@pytest.fixture(scope="module")
def zoomed():
    """three cameras on an arc in front of the plane z = 0, the last with ZOOM times the focal length of the others"""
    W, H = 129, 97
    P, C = synth.make_cameras(3, W, H, 20.0, 4.0)
    Pz, _ = synth.make_cameras(3, W, H, 20.0, 4.0, focal_px=ZOOM * 765.702941895 * W / 640.0)
    P = P.copy()
    P[2] = Pz[2]
    f = 765.702941895 * W / 640.0
    return synth.make_scene(nviews=3, W=W, H=H, radius=4.0, kind="plane", cameras=(P, C), focal=[f, f, ZOOM * f], keep_geometry=False)


def _on_plane(P, u, v):
    """the point of the plane z = 0 that projects to pixel (u, v) of the level-0 projection P"""
    M, p4 = P[:, :3].astype(np.float64), P[:, 3].astype(np.float64)
    Mi = np.linalg.inv(M)
    c, d = -Mi @ p4, Mi @ np.array([u, v, 1.0])
    t = -c[2] / d[2]
    return c + t * d


def _records(points, images):
    rec = np.zeros(len(points), dtype=synth.PATCH_DTYPE)
    rec["coord"][:, :3] = np.asarray(points)
    rec["coord"][:, 3] = 1.0
    rec["normal"][:, 2] = 1.0  # the plane's normal, towards the cameras
    rec["ncc"], rec["dscale"], rec["ascale"], rec["flags"] = -1.0, 0.005, 0.1, 1
    rec["images"][:, : len(images)] = images
    rec["nimages"] = len(images)
    return rec


def _window_in(cams, rec, view, size):
    """Head of Optim::getTex (optim.cpp:790-818, 895-915) for the record as it stands, in `view` (reference view = its first):
    -> (level chosen, window admitted, largest texel column read, largest row, smallest column, smallest row)"""
    coord, normal = rec["coord"].astype(F), rec["normal"].astype(F)
    px, py = ref_get_paxes(cams[int(rec["images"][0])], coord, normal, 0)
    P = cams[view].P[0]
    c = ref_project(P, coord)
    dx, dy = (ref_project(P, (coord + px).astype(F)) - c).astype(F), (ref_project(P, (coord + py).astype(F)) - c).astype(F)
    ratio = (np.linalg.norm(dx).astype(F) + np.linalg.norm(dy).astype(F)) / F(2)
    ld = max(0, min(2, int(np.floor(np.log2(float(ratio)) + 0.5))))
    s = F(2.0 ** ld)
    c, dx, dy = (c / s).astype(F), (dx / s).astype(F), (dy / s).astype(F)
    m = F(3)
    xs = [float((c + a * dx * m + b * dy * m)[0]) for a in (-1, 1) for b in (-1, 1)]
    ys = [float((c + a * dx * m + b * dy * m)[1]) for a in (-1, 1) for b in (-1, 1)]
    W, H = size[0] >> ld, size[1] >> ld
    ok = not (min(xs) < 2 or W - 3 <= max(xs) or min(ys) < 2 or H - 3 <= max(ys))
    return ld, ok, int(max(xs)) + 1, int(max(ys)) + 1, int(min(xs)), int(min(ys))


def test_windows_at_both_ends_of_the_block(zoomed):
    """Patches on the plane, reference view 0.  (a) Their centres run in steps of a quarter of a level-2 texel over the bottom-right
    corner of the LAST view's level 2 (30 x 22 texels of the 121 x 89 crop), the last level of the allocation: some windows are refused
    by getTexSafe, and of those admitted some read the last admissible column (W - 3) and some the last admissible row (H - 3).
    (b) Others run over the top-left corner of view 0's level 0, the start of the allocation, down to the first admissible row and
    column (2).  The numpy reading of getTex's head (_window_in) asserts that the records do what they are here for; the refinement
    (25 evaluations around each record) then samples there and beyond in either form, and the two must agree byte for byte."""
    sc = zoomed
    cams = [RefCam(sc.P[v], 0) for v in range(3)]
    P2, P0 = sc.P[2], sc.P[0]
    w2, h2 = END_SIZES[2][0] >> 2, END_SIZES[2][1] >> 2
    pts = []
    for j in range(14):
        for i in range(14):
            # level-2 texel (x, y) of view 2 is level-0 pixel (4 x, 4 y): the window's far corner from 0.75 texels inside the limit to 2.5 outside
            x, y = (w2 - 3) - 3.15 - 0.5 + 0.25 * i, (h2 - 3) - 3.15 - 0.5 + 0.25 * j
            pts.append(_on_plane(P2, 4.0 * x, 4.0 * y))
    end = _records(pts, [0, 2, 1])
    pts = [_on_plane(P0, 2.0 + 3.0 - 0.75 + 0.25 * i, 2.0 + 3.0 - 0.75 + 0.25 * j) for j in range(10) for i in range(10)]
    start = _records(pts, [0, 1, 2])
    recs = np.concatenate([end, start])

    far = [_window_in(cams, r, 2, END_SIZES[2]) for r in end]
    assert all(f[0] == 2 for f in far), sorted({f[0] for f in far})
    admitted = [f for f in far if f[1]]
    print("end of the block:", len(admitted), "of", len(far), "windows admitted; largest column / row read",
          max(f[2] for f in admitted), max(f[3] for f in admitted), "of", w2, "x", h2)
    assert 20 < len(admitted) < len(far) - 20
    assert max(f[2] for f in admitted) == w2 - 3 and max(f[3] for f in admitted) == h2 - 3
    assert any(f[2] == w2 - 3 and f[3] == h2 - 3 for f in admitted)  # the window in the very corner
    near = [_window_in(cams, r, 0, END_SIZES[0]) for r in start]
    assert all(f[0] == 0 for f in near)
    admitted0 = [f for f in near if f[1]]
    print("start of the block:", len(admitted0), "of", len(near), "windows admitted; smallest column / row read",
          min(f[4] for f in admitted0), min(f[5] for f in admitted0))
    assert 10 < len(admitted0) < len(near) - 10
    assert any(f[4] == 2 and f[5] == 2 for f in admitted0)

    e = engine.Engine(3, **KW)
    e.set_scene(sc, sizes=END_SIZES)
    with _sampler(False):
        narrow, _, _ = e.probe(engine.PROBE_REFINE, recs)
        ln = e.sampler_launches()
    with _sampler(True):
        wide, _, _ = e.probe(engine.PROBE_REFINE, recs)
        lw = e.sampler_launches()
    e.close()
    print("launches", ln, lw)
    assert ln["refine_narrow"] == 1 and ln["refine_wide"] == 0, ln
    assert lw["refine_narrow"] == 1 and lw["refine_wide"] == 1, lw
    assert narrow.tobytes() == wide.tobytes()
    moved = int((narrow["coord"] != synth.convert_records(recs, narrow.dtype)["coord"]).any(axis=1).sum())
    print("records the refinement moved:", moved, "of", recs.shape[0])
    assert moved > recs.shape[0] // 2  # the search found better proposals: it sampled
