"""The CONVERGED refiner (mvs_engine_set_refiner, include/mvskit_engine.h): Optim::refinePatch run until a tolerance or the
reference's 500-evaluation budget (optim.cpp:471-524), beside the default halving search.

CPU: the ABI entry points, and the algorithm itself -- tests/refiner_restatement.py on the oracle's cost_func against a converged
optimiser (scipy's Powell with the reference's budget and tolerance).  GPU: the probe against the restatement, the budget
semantics, the default left untouched, and whole iterations through the C ABI and the host mirror."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import oracle_binding as ob
import refiner_restatement as rr
from parity_support import probe_vs_restatement, refiner_candidates, refiner_oracle
from mvskit_amd import build, engine, synth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from quality_probe import patch_errors  # noqa: E402

F = np.float32
RD0 = RA0 = 4.0  # mvs_default_config: refine_rd0, refine_ra0
BOUNDS = [(None, None), (-23.99999, 23.99999), (-23.99999, 23.99999)]  # optim.cpp:496-506


def _in_input_frame(o, inp, out):
    """encode() of record `out` in the frame of `inp` (its centre, ray and dscale): Optim::encode, optim.cpp:549-580"""
    cam = o.camera(int(inp["images"][0]))
    ray = (inp["coord"] - cam["center"]).astype(F)
    ray = (ray / F(np.linalg.norm(ray))).astype(F)
    x0 = F(np.dot((out["coord"] - inp["coord"]).astype(F), ray)) / F(inp["dscale"])
    tmp = inp.copy()
    tmp["normal"] = out["normal"]
    x = o.encode(tmp)  # the angles depend on the normal and the reference view only
    x[0] = x0
    return x


# ------------------------------------------------------------------ CPU
def test_default_refiner_and_exports():
    for name in ("mvs_default_refiner", "mvs_engine_set_refiner"):
        assert name in engine.EXPORTS
    assert engine.PROBE_REFINE_X == 6
    for cap in (16, 32, 64):
        build.build_engine(cap=cap)
        L = engine.load_library(cap=cap)
        for name in ("mvs_default_refiner", "mvs_engine_set_refiner"):
            assert hasattr(L, name), (cap, name)
        r = engine.Refiner(7, 7, F(7))
        L.mvs_default_refiner(C.byref(r))
        assert (r.mode, r.max_evals, r.xtol) == (engine.REFINE_HALVING, 500, float(F(1e-4)))
        assert L.mvs_engine_set_refiner(None, C.byref(r)) == -1  # MVS_ERR_ARG
    assert C.sizeof(engine.Refiner) == 12


def test_restatement_against_a_converged_optimiser(small_multi_scene):
    """Nelder-Mead (the kernel's operation order, float32) vs scipy Powell with the reference's budget and tolerance
    (maxfev 500, xtol 1e-7), on the oracle's cost_func; the halving search (Oracle.refine) for scale."""
    from scipy.optimize import minimize

    o = refiner_oracle(small_multi_scene.nviews)
    o.set_scene(small_multi_scene)
    cands = refiner_candidates(o, small_multi_scene)
    assert cands.shape[0] >= 150
    gap_s, gap_h, evals, ok, worse = [], [], [], 0, 0
    for j, c in enumerate(cands):
        x = rr.clamp_angles(o.encode(c))

        def cost(y, c=c):
            return o.cost(c, np.asarray(y, F))

        f0 = cost(x)
        xs, fs, n, conv = rr.refine_converged(cost, x, RD0, RA0, 500, 1e-4)
        res = minimize(cost, x.astype(np.float64), method="Powell", bounds=BOUNDS, options={"maxfev": 500, "xtol": 1e-7})
        fref = min(float(res.fun), f0)
        _, rh = o.refine(c, (0, 0, j, 0))
        fh = cost(_in_input_frame(o, c, rh))
        gap_s.append(fs - fref)
        gap_h.append(fh - fref)
        evals.append(n)
        ok += conv
        worse += fs > f0
    gap_s, gap_h, evals = np.array(gap_s), np.array(gap_h), np.array(evals)
    print(f"gap to scipy: simplex median {np.median(gap_s):.3g} p90 {np.percentile(gap_s, 90):.3g}; halving median {np.median(gap_h):.3g} "
          f"p90 {np.percentile(gap_h, 90):.3g}; evals median {np.median(evals):.0f} p90 {np.percentile(evals, 90):.0f}; converged {ok}/{len(evals)}")
    assert np.median(gap_s) <= max(0.25 * np.median(gap_h), 1e-4)
    assert ok >= 0.95 * len(evals)
    assert worse == 0
    assert (evals <= 500).all()


def test_restatement_budget_semantics():
    """A bowl it can solve, and the same bowl with a budget too small: the count never passes max_evals."""
    def bowl(x):
        return float(((x.astype(np.float64) - np.array([0.3, -1.0, 2.0])) ** 2).sum())

    x, f, n, ok = rr.refine_converged(bowl, np.zeros(3, F), RD0, RA0, 500, 1e-4)
    assert ok and n <= 500 and f < 1e-6
    for budget in (5, 9, 40):
        _, _, n, ok = rr.refine_converged(bowl, np.zeros(3, F), RD0, RA0, budget, 1e-4)
        assert not ok and n <= budget


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
def test_probe_matches_restatement(small_multi_scene):
    probe_vs_restatement(small_multi_scene, 3, 0)


@pytest.mark.gpu
def test_probe_matches_restatement_32_view_library():
    """20 views, minImageNum 8: tau = 16 views per proposal, all 64 lanes of the four-proposal passes busy."""
    sc = synth.make_scene(nviews=20, W=256, H=160, arc_deg=120.0, radius=4.0, kind="multi")
    probe_vs_restatement(sc, 8, 32)


@pytest.mark.gpu
def test_budget_exhausted_keeps_the_input(small_multi_scene):
    o = refiner_oracle(small_multi_scene.nviews)
    o.set_scene(small_multi_scene)
    cands = refiner_candidates(o, small_multi_scene, n=80)
    e = engine.Engine(small_multi_scene.nviews, level=0, csize=2, wsize=7, minImageNum=3, enable_check=0)
    e.set_scene(small_multi_scene)
    e.set_refiner("converged", max_evals=9)
    rec, _, ni = e.probe(engine.PROBE_REFINE_X, cands)
    assert (ni < 0).sum() > 0.5 * cands.shape[0]
    assert (np.abs(ni) <= 9).all()
    for j in np.nonzero(ni < 0)[0]:
        assert rec[j]["coord"].tobytes() == cands[j]["coord"].tobytes(), j
        assert rec[j]["normal"].tobytes() == cands[j]["normal"].tobytes(), j
    # the ABI's range checks
    for bad in (dict(mode="converged", max_evals=4), dict(mode="converged", max_evals=4097), dict(mode="converged", xtol=0.0),
                dict(mode="converged", xtol=float("inf")), dict(mode="converged", xtol=float("nan"))):
        with pytest.raises(engine.EngineError):
            e.set_refiner(**bad)
    r = engine.Refiner(2, 500, F(1e-4))
    assert e.L.mvs_engine_set_refiner(e.h, C.byref(r)) == -1
    e.set_refiner("halving")
    with pytest.raises(engine.EngineError):
        e.probe(engine.PROBE_REFINE_X, cands)  # MVS_ERR_STATE under HALVING


def _one_iteration(scene, seeds, refiner):
    e = engine.Engine(scene.nviews, level=0, csize=2, wsize=7, minImageNum=3, enable_check=0, seed=5)
    if refiner == "default":
        r = engine.Refiner()
        e.L.mvs_default_refiner(C.byref(r))
        e._check(e.L.mvs_engine_set_refiner(e.h, C.byref(r)))
    elif refiner == "back":
        e.set_refiner("converged")
        e.set_refiner("halving")
    e.set_scene(scene)
    e.upload_patches(seeds)
    e.propagate(0)
    return e, e.patches()


@pytest.mark.gpu
def test_default_refiner_is_unchanged(small_multi_scene):
    seeds = synth.make_seeds(small_multi_scene, stride=4, seed=21)
    e0, p0 = _one_iteration(small_multi_scene, seeds, None)
    e1, p1 = _one_iteration(small_multi_scene, seeds, "default")
    e2, p2 = _one_iteration(small_multi_scene, seeds, "back")
    assert p0.shape[0] > seeds.shape[0]
    assert p0.tobytes() == p1.tobytes() and p0.tobytes() == p2.tobytes()
    sub = seeds[:150]
    pre, _, flag = e0.probe(engine.PROBE_PREPROCESS, sub)
    sub = pre[flag == 0]
    r0, _, _ = e0.probe(engine.PROBE_REFINE, sub)
    r1, _, _ = e1.probe(engine.PROBE_REFINE, sub)
    assert r0.tobytes() == r1.tobytes()
    e1.set_refiner("converged")
    r2, _, _ = e1.probe(engine.PROBE_REFINE, sub)
    assert r2.tobytes() != r0.tobytes()  # PROBE_REFINE follows the engine's refiner


def _reconstruct(sc, seeds, mode):
    e = engine.Engine(sc.nviews, level=0, csize=2, wsize=7, minImageNum=3, enable_check=1, seed=3)
    e.set_refiner(mode)
    e.set_scene(sc)
    e.upload_patches(seeds)
    counters = []
    for it in range(3):
        counters.append(e.propagate(it))
        e.filter()
        e.update_threshold()
    p = e.patches()
    return p[p["dscale"] > 0], counters


@pytest.mark.gpu
def test_converged_reconstructs_the_scene_and_host_mirror_agrees(small_multi_scene):
    sc = small_multi_scene
    seeds = synth.make_seeds(sc, stride=3, seed=19)
    rel0, _ = patch_errors(sc, seeds)
    made_h, _ = _reconstruct(sc, seeds, "halving")
    made, counters = _reconstruct(sc, seeds, "converged")
    # test_quality.test_engine_reconstructs_the_scene's ground-truth bounds
    assert made.shape[0] > 10 * seeds.shape[0]
    rel, ang = patch_errors(sc, made)
    _, ang_h = patch_errors(sc, made_h)
    print(f"converged: {made.shape[0]} patches, median normal error {np.median(ang):.2f} deg (halving {np.median(ang_h):.2f}); "
          f"evals per patch {sum(c['evals'] for c in counters) / sum(c['patches'] for c in counters):.1f}")
    assert np.median(rel) < 0.7 * np.median(rel0)
    assert np.median(rel) < 6e-4 and np.percentile(rel, 90) < 2e-3 and np.percentile(rel, 99) < 8e-3
    assert np.median(ang) < 8.0 and np.median(made["ncc"]) > 0.95
    assert np.median(ang) <= np.median(ang_h)

    # one iteration of the host mirror (PmMvps::m_refiner) against the Python binding
    host = C.CDLL(build.build_host())
    host.mvshost_set_filter.argtypes = [C.c_int]
    host.mvshost_set_filter.restype = None
    host.mvshost_set_refiner.argtypes = [C.c_int, C.c_int, C.c_float]
    host.mvshost_set_refiner.restype = None
    host.mvshost_run.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_uint,
                                 C.c_int, C.c_longlong, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p]
    P = np.ascontiguousarray(sc.P, dtype=F)
    img = np.ascontiguousarray(sc.images)
    sd = np.ascontiguousarray(synth.make_seeds(sc, stride=4, seed=21))
    cap = 200000
    out = np.zeros(cap, dtype=engine.PATCH_DTYPE)
    n, ptot = C.c_longlong(), C.c_longlong()
    host.mvshost_set_filter(0)
    host.mvshost_set_refiner(engine.REFINE_CONVERGED, 500, 1e-4)
    try:
        assert host.mvshost_run(sc.nviews, sc.W, sc.H, P.ctypes.data, img.ctypes.data, 0, 2, 7, 3, C.c_float(0.7), 9, 1, sd.shape[0], sd.ctypes.data,
                                cap, out.ctypes.data, C.byref(n), C.byref(ptot)) == 0
    finally:
        host.mvshost_set_refiner(engine.REFINE_HALVING, 500, 1e-4)
        host.mvshost_set_filter(1)
    hm = out[: n.value]
    e = engine.Engine(sc.nviews, level=0, csize=2, wsize=7, minImageNum=3, nccThreshold=0.7, seed=9)
    e.set_refiner("converged")
    e.set_scene(sc)
    e.upload_patches(sd)
    e.set_thresholds(0.7, float(F(0.7) - F(0.3)), 1)  # PmMvps::init + the ++m_depth before the first iteration
    e.propagate(0)
    pm = e.patches()
    assert hm.shape[0] == pm.shape[0] > sd.shape[0]
    for f in ("coord", "normal", "ncc", "dscale", "nimages", "images"):
        assert hm[f].tobytes() == pm[f].tobytes(), f
