"""A second, independent reading of the reference's hot-path arithmetic -- written in numpy straight from the reference's
source text (file:line cited per function), with no code shared with oracle/pmmvs_oracle.cpp -- compared with the oracle in
its reference summation order (ORC_SUM_SEQ).  The reference ships no golden vectors and cannot be built here (Eigen, CImg,
NLopt absent), so this is what stands between "the oracle agrees with itself" and "two restatements of the same source
agree": pyramids byte for byte, projections / patch axes / sampling / normalisation / NCC to float rounding (the oracle's
documented deviations are reciprocal-multiplies and fused multiply-adds).  The checks that involve a camera live
in reading_checks.py, which tests/test_camera_families.py runs on cameras off the arc."""
import numpy as np
import pytest

import oracle_binding as ob
from mvskit_amd import synth
import reading_checks as rc
from second_reading import F, RefCam, ref_get_color, ref_get_mask_all, ref_get_unit, ref_mask_down, ref_pyr_down, ref_quad_residual, ref_robustincc


# ------------------------------------------------------------------ the comparison
@pytest.fixture(scope="module")
def setup():
    return rc.make_setup(synth.make_scene(nviews=4, W=160, H=120, arc_deg=45.0, radius=4.0, kind="multi"))


def test_pyramid_second_reading(setup):
    sc, o, cams, pyrs, _ = setup
    for v in (0, 3):
        for level in (1, 2):
            np.testing.assert_array_equal(o.pyramid(v, level), pyrs[v][level])


def test_pyramid_second_reading_odd_sizes():
    """Image::alloc halves with W / 2 rounded down (image.cpp:135-138): below an odd parent the last output pixel's 2x + 2 tap is
    the parent's last column (kept), below an even parent it lies outside (dropped).  The fixture above has even parents only.
    Two views of unequal size: 97x75 -> 48x37 -> 24x18 -> 12x9 and 91x70 -> 45x35 -> 22x17 -> 11x8, so both kinds of parent occur
    in both directions and at more than one level."""
    sc = synth.make_scene(nviews=2, W=97, H=75, arc_deg=20.0, radius=4.0, kind="plane")
    sizes = [(97, 75), (91, 70)]
    o = ob.Oracle(2, level=1, csize=2, wsize=7, minImageNum=2, schedule=ob.SCHEDULE_ENGINE, sum_mode=ob.SUM_SEQ, enable_check=0, nthreads=1)
    o.set_scene(sc, sizes=sizes)
    odd_parents = 0
    for v, (w, h) in enumerate(sizes):
        img = np.ascontiguousarray(sc.images[v][:h, :w])
        for level in range(1, 4):
            odd_parents += (img.shape[1] & 1) + (img.shape[0] & 1)
            img = ref_pyr_down(img)
            got = o.pyramid(v, level)
            assert got.shape == (h >> level, w >> level, 3)
            np.testing.assert_array_equal(got, img, err_msg=f"view {v} level {level}")
    assert odd_parents >= 6
    assert o.grid_dims(0) == (24, 19) and o.grid_dims(1) == (23, 18)  # ceil(48 / 2) x ceil(37 / 2), ceil(45 / 2) x ceil(35 / 2)
    o.close()


def test_mask_pyramid_second_reading_odd_sizes():
    """The oracle has no accessor for its mask pyramid, so it is read through the one place that uses it, Optim::postProcess
    (optim.cpp:260-298: `if (m_pmmvps.m_photoSets.getMask(patch.m_coord, m_pmmvps.m_level) == 0) return -1`): the same records go
    through an oracle with masks and one without.  Where the numpy reading of the level-1 masks says "masked", the masked oracle
    must refuse the record; everywhere else it must return what the unmasked one returns.  Level 1 of a 97x75 scene (48x37), masks
    binarised at 127 (image.cpp:149-156) with a zero band between the odd columns 41 and 47, a zero last column and last row
    (never read at level 1: 2 * 48 < 97, 2 * 37 < 75) and a sub-threshold block."""
    sc = synth.make_scene(nviews=3, W=97, H=75, arc_deg=25.0, radius=4.0, kind="plane")
    nv, level = sc.nviews, 1
    raw = np.full((nv, sc.H, sc.W), 255, np.uint8)
    raw[:, :, 41:48] = 0
    raw[:, :, sc.W - 1] = 0
    raw[:, sc.H - 1, :] = 0
    raw[1, 20:31, 60:71] = 127  # not above 127: background
    raw[2, 40:51, 10:21] = 128  # above: foreground
    kw = dict(level=level, csize=1, wsize=5, minImageNum=2, schedule=ob.SCHEDULE_ENGINE, sum_mode=ob.SUM_SEQ, enable_check=0, nthreads=1, seed=1)
    om, o0 = ob.Oracle(nv, **kw), ob.Oracle(nv, **kw)
    om.set_scene(sc, masks=raw)
    o0.set_scene(sc)
    cams = [RefCam(sc.P[v], level) for v in range(nv)]
    masks = []
    for v in range(nv):
        m0 = np.where(raw[v] > 127, 255, 0).astype(np.uint8)
        masks.append([m0, ref_mask_down(m0)])
        assert masks[v][1].shape == (37, 48)
    assert masks[2][1][20:25, 5:10].all() and not masks[1][1][11:15, 31:35].any()
    assert masks[0][1][:, 47].all() and masks[0][1][36, :20].all()  # the zero last column and row of level 0 left no trace
    seeds = synth.make_seeds(sc, level=level, csize=1, stride=2, seed=4)
    masked = plain = passed = 0
    for i, s in enumerate(seeds):
        f, rec = o0.preprocess(s)
        if f != 0:
            continue
        _, rec = o0.refine(rec, (0, 0, i, 0))
        f0, r0 = o0.postprocess(rec)
        fm, rm = om.postprocess(rec)
        if ref_get_mask_all(cams, masks, rec["coord"].astype(F), level) == 0:
            assert fm != 0, rec["coord"]
            masked += 1
        else:
            assert fm == f0, (rec["coord"], fm, f0)
            if f0 == 0:
                assert rm.tobytes() == r0.tobytes()
                passed += 1
            plain += 1
    assert masked > 30 and passed > 100 and plain > masked, (masked, plain, passed)
    om.close()
    o0.close()


def test_camera_second_reading(setup):
    rc.check_camera(setup)


def test_units_axes_and_samples_second_reading(setup):
    sc, o, cams, pyrs, seeds = setup
    rc.check_units_and_axes(setup)
    rng = np.random.RandomState(3)
    for _ in range(200):
        v, level = rng.randint(sc.nviews), rng.randint(3)
        H, W = pyrs[v][level].shape[:2]
        x, y = F(rng.uniform(1, W - 2)), F(rng.uniform(1, H - 2))
        np.testing.assert_allclose(o.get_color(v, x, y, level), ref_get_color(pyrs[v][level], x, y), rtol=1e-6, atol=1e-4)


def test_texture_and_incc_second_reading(setup):
    rc.check_texture_and_incc(setup)
    for r in np.linspace(0, 0.33, 12):
        assert abs(ob.lib().orc_robustincc(float(r)) - ref_robustincc(r)) < 1e-7


# ------------------------------------------------------------------ refinement variables, cost, scales, neighbours
def test_encode_decode_and_cost_second_reading(setup):
    rc.check_encode_decode_and_cost(setup)


def test_scales_and_neighbours_second_reading(setup):
    rc.check_scales_and_neighbours(setup)


def test_generate_patch_second_reading(setup):
    rc.check_generate_patch(setup)


def test_filter_quad_second_reading(setup):
    """The oracle solves the 5-parameter fit by normal equations in double, the reference by an SVD in float: the residual the
    decision rests on must agree (a curved, noisy neighbourhood and a flat one; the decision threshold is 2.5)."""
    sc, o, cams, pyrs, seeds = setup
    rng = np.random.RandomState(13)
    worst = 0.0
    for k, s in enumerate(seeds[:40]):
        n = int(rng.randint(7, 120))
        unit = float(ref_get_unit(cams[int(s["images"][0])], s["coord"].astype(F), 0))
        z = s["normal"][:3].astype(np.float64)
        t1 = np.cross(z, [1.0, 0.3, 0.2]); t1 /= np.linalg.norm(t1)
        t2 = np.cross(z, t1)
        uv = rng.uniform(-6, 6, (n, 2)) * unit
        curv = (0.0 if k % 3 == 0 else rng.uniform(-0.5, 0.5)) / unit
        noise = rng.normal(0, (0.1, 1.0, 4.0)[k % 3] * unit, n)
        hgt = curv * (uv[:, 0] ** 2 - 0.5 * uv[:, 1] ** 2 + 0.3 * uv[:, 0] * uv[:, 1]) + 0.2 * uv[:, 0] + noise
        pts = s["coord"][:3].astype(np.float64) + uv[:, :1] * t1 + uv[:, 1:] * t2 + hgt[:, None] * z
        coords = np.concatenate([pts, np.ones((n, 1))], 1).astype(F)
        got = float(o.quad_residual(s, coords))
        exp = float(ref_quad_residual(cams, s, coords, 0, min(4, sc.nviews)))
        assert abs(got - exp) <= 2e-3 * max(exp, 1e-3), (k, n, got, exp)
        assert (got < 2.5) == (exp < 2.5)
        worst = max(worst, abs(got - exp) / max(exp, 1e-3))
    assert worst < 2e-3


def test_set_inccs_matrix_second_reading(setup):
    rc.check_set_inccs_matrix(setup)
