"""The checks of the CPU oracle against the second reading that involve a camera (a helper module like second_reading.py): the bodies
that tests/test_oracle_second_reading.py runs on the arc scene and tests/test_camera_families.py on the scenes of camera_scenes.py.

Every check takes `k`, a dict {quantity: factor} on that quantity's tolerance (None: 1 throughout, the arc, where the tolerances were
set).  The factor a test passes is the scene's kappa (camera_scenes.kappa): by how much the world's coordinates exceed its depths.
A float32 projection u = (P0 . X + p03) / (P2 . X + p23) rounds relative to |P[:, :3]| |X| + |P[:, 3]|, kappa times the depth it is
then divided by, so the two readings' pixel positions differ by kappa times what they do on the arc.  PIXEL_QUANTITIES are the ones
that are a pixel position or a smooth function of some, so that their disagreement is linear in the positions':
  project          the position itself: atol 1e-4 pixel times kappa
  axes             a unit step over the distance of two projections one pixel apart: the relative error of the distance, twice the
                   projection's tolerance over one pixel, 2 kappa 1e-4 of the axis' largest component on top of its rtol
  tex              a bilinear sample: its error is the position's times the image gradient
  normalised tex   the same samples minus their mean over their deviation, both linear in the samples
  incc, cost,      1 - the dot product of two normalised textures (and its robust form, and sums of those): linear in the samples
  incc matrix      for small differences
  scales           m_dscale and m_ascale are quotients of one-pixel differences of projections, like the axes' length
A test scales only those of them that miss the unscaled tolerance on its scene (tests/test_camera_families.py lists them with the
values seen).  The other tolerances never take a factor: unproject, the round trip, decode and generate_patch are dominated by
their relative part on coordinates that large; encode, the unit, ipscale and the camera's axes hold unscaled at kappa 173.
Each check prints the worst value it met as a share of its tolerance and returns it."""
import numpy as np

import oracle_binding as ob
from mvskit_amd import synth
from second_reading import (F, RefCam, ref_compute_incc, ref_cost_func, ref_decode, ref_dot, ref_encode, ref_get_paxes, ref_get_tex,
                            ref_get_unit, ref_is_neighbor, ref_normalize, ref_project, ref_pyr_down, ref_robustincc, ref_set_scales,
                            ref_unproject)

PROJ_ATOL = 1e-4  # pixels, on the arc
PIXEL_QUANTITIES = ("project", "axes", "tex", "normalised tex", "incc", "cost", "scales", "incc matrix")
FAMILY_AXES_RTOL = 2.0 * float(np.spacing(np.float32(160.0)))  # check_units_and_axes: images of at most 256 pixels
COS_THR = F(np.cos(F(60.0 * np.pi / 180.0)))


def make_setup(sc):
    """(scene, oracle in the reference's summation order, RefCams, pyramids of three levels, make_seeds(stride=9, seed=4))"""
    o = ob.Oracle(sc.nviews, level=0, csize=2, wsize=7, minImageNum=2, schedule=ob.SCHEDULE_ENGINE, sum_mode=ob.SUM_SEQ, enable_check=0, seed=1)
    o.set_scene(sc)
    cams = [RefCam(sc.P[v], 0) for v in range(sc.nviews)]
    pyrs = []
    for v in range(sc.nviews):
        levels = [sc.images[v]]
        for _ in range(2):
            levels.append(ref_pyr_down(levels[-1]))
        pyrs.append(levels)
    seeds = synth.make_seeds(sc, stride=9, seed=4)
    return sc, o, cams, pyrs, seeds


def _k(k, quantity):
    """the factor on `quantity`'s tolerance: k[quantity], 1 where k is None or does not name it"""
    return 1.0 if k is None else float(k.get(quantity, 1.0))


def _share(got, want, rtol, atol):
    """the largest |got - want| / (atol + rtol |want|): at most 1 where np.testing.assert_allclose(got, want, rtol, atol) passes"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want) / (atol + rtol * np.abs(want))))


class _Worst(dict):
    def take(self, key, share):
        self[key] = max(self.get(key, 0.0), float(share))

    def report(self, what):
        print(what, "worst shares of the tolerances:", ", ".join(f"{k} {v:.3f}" for k, v in self.items()))
        return self


def check_camera(setup, k=None):
    sc, o, cams, _, seeds = setup
    w = _Worst()
    for v in range(sc.nviews):
        c = o.camera(v)
        np.testing.assert_allclose(c["center"], cams[v].center, rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(c["oaxis"], cams[v].oaxis, rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(c["xaxis"], cams[v].xaxis, rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(c["yaxis"], cams[v].yaxis, rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(c["zaxis"], cams[v].zaxis, rtol=1e-5, atol=1e-6)
        assert abs(c["ipscale"] - cams[v].ipscale) <= 1e-5 * abs(cams[v].ipscale)
        w.take("center", _share(c["center"], cams[v].center, 1e-5, 1e-6))
        w.take("oaxis", _share(c["oaxis"], cams[v].oaxis, 1e-6, 1e-7))
        w.take("axes", max(_share(c[a], getattr(cams[v], a), 1e-5, 1e-6) for a in ("xaxis", "yaxis", "zaxis")))
        w.take("ipscale", abs(c["ipscale"] - cams[v].ipscale) / (1e-5 * abs(cams[v].ipscale)))
    for s in seeds[:40]:
        X = s["coord"].astype(F)
        for v in (0, 2):
            for level in (0, 1):
                P = cams[v].P[level]
                ic = ref_project(P, X)
                got = o.project(v, X, level)
                np.testing.assert_allclose(got, ic, rtol=2e-6, atol=_k(k, "project") * PROJ_ATOL)
                w.take("project", _share(got, ic, 2e-6, _k(k, "project") * PROJ_ATOL))
                homog = (ic * F(np.dot(P[2], X))).astype(F)  # (u*w, v*w, w): unproject inverts P exactly
                back = ref_unproject(P, homog)
                got = o.unproject(v, np.append(homog, F(1)), level)
                np.testing.assert_allclose(got, back, rtol=1e-4, atol=1e-4)
                np.testing.assert_allclose(back[:3], X[:3], rtol=1e-3, atol=1e-3)
                w.take("unproject", _share(got, back, 1e-4, 1e-4))
                w.take("round trip", _share(back[:3], X[:3], 1e-3, 1e-3))
    return w.report("camera")


def check_units_and_axes(setup, k=None, axes_rtol=2e-5):
    """axes_rtol: 2e-5 was set on the arc's first 30 seeds (worst seen 1.5e-5).  FAMILY_AXES_RTOL derives it instead: an axis is a
    unit step over the distance of two projections one pixel apart; a projected coordinate below 256 pixels is a float32 spaced 2^-16,
    the two readings round it differently (fused or not, divide or reciprocal) by up to one spacing each way, and the distance takes
    the difference of two of them: 2 * 2^-16 = 3.05e-5 of one pixel, the same factor on every component of the axis."""
    sc, o, cams, _, seeds = setup
    w = _Worst()
    for s in seeds[:30]:
        X, N = s["coord"].astype(F), s["normal"].astype(F)
        v = int(s["images"][0])
        unit = ref_get_unit(cams[v], X, 0)
        assert abs(o.get_unit(v, X) - unit) <= 2e-6 * unit
        w.take("unit", abs(o.get_unit(v, X) - unit) / (2e-6 * unit))
        px, py = o.get_paxes(v, X, N)
        rx, ry = ref_get_paxes(cams[v], X, N, 0)
        for got, want in ((px, rx), (py, ry)):
            atol = 1e-9 + (2.0 * _k(k, "axes") * PROJ_ATOL * float(np.abs(want).max()) if _k(k, "axes") > 1.0 else 0.0)
            np.testing.assert_allclose(got, want, rtol=axes_rtol, atol=atol)
            w.take("patch axes", _share(got, want, axes_rtol, atol))
    return w.report("units and axes")


def check_texture_and_incc(setup, k=None):
    sc, o, cams, pyrs, seeds = setup
    w = _Worst()
    checked = 0
    for s in seeds[:60]:
        X, N = s["coord"].astype(F), s["normal"].astype(F)
        idx = [int(i) for i in s["images"][: s["nimages"]]]
        if len(idx) < 2:
            continue
        px, py = ref_get_paxes(cams[idx[0]], X, N, 0)
        t = ref_get_tex(cams[idx[1]], pyrs[idx[1]], X, px, py, N, 0, 7, COS_THR)
        flag, tex = o.get_tex(X, px, py, N, idx[1], normalize=False)
        assert (t is None) == (flag != 0)
        if t is not None:
            np.testing.assert_allclose(tex.reshape(49, 3), t, rtol=1e-5, atol=_k(k, "tex") * 2e-3)  # positions differ by float rounding of the axes
            w.take("tex", _share(tex.reshape(49, 3), t, 1e-5, _k(k, "tex") * 2e-3))
            flag, texn = o.get_tex(X, px, py, N, idx[1], normalize=True)
            np.testing.assert_allclose(texn.reshape(49, 3), ref_normalize(t), rtol=1e-3, atol=_k(k, "normalised tex") * 2e-3)
            w.take("normalised tex", _share(texn.reshape(49, 3), ref_normalize(t), 1e-3, _k(k, "normalised tex") * 2e-3))
        for robust in (0, 1):
            got = o.compute_incc(s, robust=robust)
            exp = ref_compute_incc(cams, pyrs, X, N, idx, 0, 7, min(2 * 2, sc.nviews), robust, COS_THR)  # m_tau, pmmvps.cpp:32
            assert abs(got - exp) <= _k(k, "incc") * 5e-5 * max(1.0, abs(exp)), (got, exp)  # measured worst case 6.4e-6 on the arc
            w.take("incc", abs(got - exp) / (_k(k, "incc") * 5e-5 * max(1.0, abs(exp))))
            checked += 1
    assert checked > 60
    return w.report("texture and incc")


def check_encode_decode_and_cost(setup, k=None):
    sc, o, cams, pyrs, seeds = setup
    rng = np.random.RandomState(7)
    w = _Worst()
    checked = 0
    for s in seeds[:40]:
        idx = [int(i) for i in s["images"][: s["nimages"]]]
        if len(idx) < 2:
            continue
        X, N = s["coord"].astype(F), s["normal"].astype(F)
        rec = s.copy()
        rec["dscale"] = F(0.01)
        cam = cams[idx[0]]
        ray = (X - cam.center).astype(F)
        ray = (ray / np.linalg.norm(ray).astype(F)).astype(F)
        x = ref_encode(cam, X, ray, rec["dscale"], X, N)
        np.testing.assert_allclose(o.encode(rec), x, rtol=0, atol=2e-4)  # angles in units of pi/48: 2e-4 units = 1.3e-5 rad
        w.take("encode", _share(o.encode(rec), x, 0, 2e-4))
        x2 = (x + rng.uniform(-1.5, 1.5, 3)).astype(F)
        c, n = o.decode(rec, x2)
        rc, rn = ref_decode(cam, X, ray, rec["dscale"], x2)
        np.testing.assert_allclose(c, rc, rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(n, rn, rtol=0, atol=2e-6)
        w.take("decoded coord", _share(c, rc, 1e-6, 1e-6))
        w.take("decoded normal", _share(n, rn, 0, 2e-6))
        got = o.cost(rec, x2)
        exp = ref_cost_func(cams, pyrs, X, ray, rec["dscale"], idx, x2, 0, 7, min(4, sc.nviews), 2, COS_THR)
        assert abs(got - exp) <= _k(k, "cost") * 5e-5 * max(1.0, abs(exp)), (got, exp)
        w.take("cost", abs(got - exp) / (_k(k, "cost") * 5e-5 * max(1.0, abs(exp))))
        checked += 1
    assert checked > 25
    return w.report("encode, decode and cost")


def check_scales_and_neighbours(setup, k=None):
    sc, o, cams, pyrs, seeds = setup
    tau = min(4, sc.nviews)
    ks = _k(k, "scales")
    w = _Worst()
    done = []
    for s in seeds[:60]:
        f, rec = o.preprocess(s)
        if f != 0:
            continue
        idx = [int(i) for i in rec["images"][: rec["nimages"]]]
        ds, asc = ref_set_scales(cams, rec["coord"].astype(F), idx, 0, 7, tau)
        # m_dscale is a quotient of ~1-pixel differences of projections ~100 pixels large: rounding of the projections (fused or not)
        # shows at 1e-5 relative
        assert abs(rec["dscale"] - ds) <= ks * 2e-4 * ds and abs(rec["ascale"] - asc) <= ks * 2e-4 * asc, (rec["dscale"], ds, rec["ascale"], asc)
        w.take("scales", max(abs(rec["dscale"] - ds) / (ks * 2e-4 * ds), abs(rec["ascale"] - asc) / (ks * 2e-4 * asc)))
        done.append(rec)
    assert len(done) > 30
    pairs = same = 0
    for i in range(0, len(done) - 1):
        for j in (i + 1, (i + 7) % len(done)):
            if i == j:
                continue
            for thr in (0.25, 1.0, 4.0):
                pairs += 1
                same += o.is_neighbor(done[i], done[j], thr) == ref_is_neighbor(cams, done[i], done[j], 2, 0, thr)
    assert pairs > 100 and same == pairs
    return w.report("scales and neighbours")


def check_generate_patch(setup, k=None):
    """Propagate::generatePatch, propagate.cpp:220-237: depth along the optical axis of the source's reference view, the pixel
    unprojected at that depth, the source's normal; views whose cell falls outside the grid are dropped (setGridsImages)."""
    sc, o, cams, pyrs, seeds = setup
    rng = np.random.RandomState(11)
    w = _Worst()
    checked = 0
    for s in seeds[:60]:
        v = int(s["images"][0])
        X = s["coord"].astype(F)
        ic0 = ref_project(cams[v].P[0], X)
        ic = np.array([ic0[0] + rng.uniform(-3, 3), ic0[1] + rng.uniform(-3, 3), 1.0], F)
        f, rec = o.generate_patch(s, ic)
        if f != 0:
            continue
        depth = F(np.dot(cams[v].oaxis, X))
        exp = ref_unproject(cams[v].P[0], (depth * ic).astype(F))
        np.testing.assert_allclose(rec["coord"], exp, rtol=2e-5, atol=2e-5)
        w.take("generated coord", _share(rec["coord"], exp, 2e-5, 2e-5))
        np.testing.assert_array_equal(rec["normal"], s["normal"])
        kept = [int(i) for i in rec["images"][: rec["nimages"]]]
        assert kept and kept[0] == v and set(kept) <= {int(i) for i in s["images"][: s["nimages"]]}
        for i in kept:  # every kept view sees the new point inside its grid (cells of csize 2 at level 0)
            p = ref_project(cams[i].P[0], exp)
            gx, gy = int(np.floor(p[0] + F(0.5))) // 2, int(np.floor(p[1] + F(0.5))) // 2
            assert 0 <= gx < (sc.W + 1) // 2 and 0 <= gy < (sc.H + 1) // 2
        checked += 1
    assert checked > 40
    return w.report("generate_patch")


def check_set_inccs_matrix(setup, k=None):
    """Optim::setINCCs (matrix form, optim.cpp:748-783), what Optim::setRefImage (348-383) sums by rows to pick the reference view."""
    sc, o, cams, pyrs, seeds = setup
    w = _Worst()
    checked = 0
    for s in seeds[:40]:
        idx = [int(i) for i in s["images"][: s["nimages"]]]
        if len(idx) < 3:
            continue
        X, N = s["coord"].astype(F), s["normal"].astype(F)
        px, py = ref_get_paxes(cams[idx[0]], X, N, 0)
        texs = []
        for v in idx:
            t = ref_get_tex(cams[v], pyrs[v], X, px, py, N, 0, 7, COS_THR)
            texs.append(None if t is None else ref_normalize(t))
        n = len(idx)
        exp = np.zeros((n, n), F)
        for i in range(n):
            for j in range(i + 1, n):
                exp[i, j] = exp[j, i] = F(2) if texs[i] is None or texs[j] is None else ref_robustincc(F(1) - ref_dot(texs[i], texs[j]))
        got = o.set_inccs_matrix(s, robust=1)
        np.testing.assert_allclose(got, exp, rtol=0, atol=_k(k, "incc matrix") * 5e-5)
        w.take("incc matrix", _share(got, exp, 0, _k(k, "incc matrix") * 5e-5))
        sums_e, sums_g = exp.sum(1), got.sum(1)
        if np.sort(sums_e)[1] - np.sort(sums_e)[0] > 1e-3:  # away from ties both readings choose the same reference view
            assert int(np.argmin(sums_e)) == int(np.argmin(sums_g))
        checked += 1
    assert checked > 15
    return w.report("set_inccs_matrix")
