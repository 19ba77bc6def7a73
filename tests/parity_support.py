"""The engine-against-oracle harness of the GPU tests (a helper module like oracle_binding.py): an oracle and an engine on the same
scene and configuration, the comparisons every parity test makes of their records, pools and maps with the north-star tolerance, the
loop of two iterations with its assertions, the converged refiner's probe against its restatement, and the small pools, grids and seed
lists that several test modules share."""
import os
from contextlib import contextmanager

import numpy as np

import oracle_binding as ob
import refiner_restatement as rr
from mvskit_amd import engine, synth

REL_TOL = 1e-3  # BASELINE.json north_star: depth/normal maps within 1e-3 relative
COUNTERS = ("candidates", "prefiltered", "patches", "fail0", "fail1", "inserted", "replaced", "evals", "view_evals", "trimmed")
REMOVALS = ("outside", "exact", "neighbor", "groups")
GRID_KW = dict(level=0, csize=2, wsize=7, minImageNum=2, seed=11, enable_check=1)  # the sweep tests' 65 x 49 grid scene
SEEDED = (0, 2)  # the views that hold seeds where two of five do


def pair(scene, **kw):
    n = scene.nviews
    okw = dict(level=0, csize=2, wsize=7, minImageNum=kw.pop("minImageNum", 3), schedule=ob.SCHEDULE_ENGINE,
               sum_mode=ob.SUM_TREE64, enable_check=0, nthreads=8)
    ekw = dict(level=0, csize=2, wsize=7, minImageNum=okw["minImageNum"], enable_check=0)
    for k, v in kw.items():
        okw[k] = v
        ekw[k] = v
    if okw.get("list_cap", 0) > 32:
        okw["wide"] = True  # 64 views per list: the oracle's wide build (192-byte records, as libmvskit_engine_cap64.so)
    o = ob.Oracle(n, **okw)
    e = engine.Engine(n, **ekw)
    o.set_scene(scene)
    e.set_scene(scene)
    return o, e


def cmp_records(a, b, what):
    assert a["nimages"] == b["nimages"], f"{what}: nimages {a['nimages']} != {b['nimages']}"
    n = int(a["nimages"])
    np.testing.assert_array_equal(a["images"][:n], b["images"][:n], err_msg=what)
    np.testing.assert_allclose(a["coord"], b["coord"], rtol=REL_TOL, atol=1e-6, err_msg=what)
    np.testing.assert_allclose(a["normal"], b["normal"], rtol=0, atol=REL_TOL, err_msg=what)
    for f in ("ncc", "dscale", "ascale"):
        np.testing.assert_allclose(a[f], b[f], rtol=REL_TOL, atol=1e-6, err_msg=what + f)


def maps_close(o, e, nviews):
    tot = bad = 0
    for v in range(nviews):
        for kind in (0, 1):
            do, no, io = o.depth_normal_map(v, kind)
            de, ne, ie = e.depth_normal_map(v, kind)
            assert (np.isnan(do) == np.isnan(de)).all(), f"empty mask differs view {v} kind {kind}"
            m = ~np.isnan(do)
            tot += int(m.sum())
            rel = np.abs(do[m] - de[m]) / np.abs(do[m])
            ang = np.arccos(np.clip((no[m] * ne[m]).sum(-1), -1, 1))
            bad += int(((rel > REL_TOL) | (ang > REL_TOL)).sum())
    return tot, bad


def dense_pool(sc, per_cell, window=12, ref=0):
    """`per_cell` patches in every cell of a `window` x `window` block of view `ref`'s grid (make_seeds' noisy plane seeds, one
    draw per RNG seed), scored and scaled by hand: what Filter::run meets after a few iterations without the trim."""
    recs = []
    for k in range(per_cell):
        sd = synth.make_seeds(sc, stride=1, seed=100 + k, views=[ref])
        P = sc.P.astype(np.float64)[ref]
        x = sd["coord"].astype(np.float64) @ P.T
        cx = np.floor(x[:, 0] / x[:, 2] + 0.5).astype(int) // 2
        cy = np.floor(x[:, 1] / x[:, 2] + 0.5).astype(int) // 2
        keep = (cx >= 60) & (cx < 60 + window) & (cy >= 50) & (cy < 50 + window)
        recs.append(sd[keep])
    pool = np.ascontiguousarray(np.concatenate(recs))
    pool["ncc"] = 0.9
    pool["dscale"] = 0.004
    return pool


def grid_of(w, h, level, csize):
    """gw, gh = ceil(W[level] / csize), ceil(H[level] / csize), W[level] = W >> level (patch_manager.cpp:36-37, image.cpp:135-138)"""
    return -(-(w >> level) // csize), -(-(h >> level) // csize)


def pair_sized(sc, masks=None, sizes=None, full_cells=False, **kw):
    """pair() with masks / per-view sizes.  full_cells: the engine's pool holds MAX_NUM_OF_PATCHES = max_propag * csize^2 patches in
    every cell (mvs_config.max_patches).  The default is four per cell, half of that staged per pass, which the csize 3 scenes here,
    with up to 18 per cell, exceed: the engine then refuses the pass with MVS_ERR_CAPACITY and names max_patches."""
    if full_cells:
        wh = sizes or [(sc.W, sc.H)] * sc.nviews
        cells = sum(gw * gh for gw, gh in (grid_of(w, h, kw["level"], kw["csize"]) for w, h in wh))
        o = ob.Oracle(sc.nviews, schedule=ob.SCHEDULE_ENGINE, sum_mode=ob.SUM_TREE64, nthreads=8, **kw)
        e = engine.Engine(sc.nviews, max_patches=cells * kw.get("max_propag", 2) * kw["csize"] ** 2, **kw)
    else:
        o, e = pair(sc, **kw)
        if masks is None and sizes is None:
            return o, e
    o.set_scene(sc, masks=masks, sizes=sizes)
    e.set_scene(sc, masks=masks, sizes=sizes)
    return o, e


def loop_two_iterations(o, e, sc, seeds, floors, what):
    o.add_patches(seeds)
    e.upload_patches(seeds)
    for it in range(2):
        co, ce = o.propagate(it), e.propagate(it)
        print(what, "it", it, "oracle", co, "engine", ce)
        assert co == ce, (what, it, co, ce)
        assert set(COUNTERS) <= set(co), f"{what}: counters {sorted(co)} lack some of {COUNTERS}"
        if floors is not None:
            assert 2 * co["patches"] >= floors[it][0] and 2 * co["inserted"] >= floors[it][1], (what, it, co, floors)
        ro, re_ = o.filter(), e.filter()
        print(what, "it", it, "removed: oracle", ro, "engine", re_)
        assert [ro[k] for k in REMOVALS] == [re_[k] for k in REMOVALS], (what, it, ro, re_)
        if it == 0:
            assert sum(ro[k] > 0 for k in REMOVALS) >= 3, (what, ro)
        o.update_threshold()
        e.update_threshold()
    po, pe = o.patches(), e.patches()
    assert po.shape == pe.shape and po.shape[0] > 0, f"pools of {po.shape} (oracle) and {pe.shape} (engine) records"
    np.testing.assert_array_equal(po["nimages"], pe["nimages"])
    np.testing.assert_array_equal(po["images"], pe["images"])
    np.testing.assert_array_equal(po["vimages"], pe["vimages"])
    np.testing.assert_allclose(pe["coord"], po["coord"], rtol=REL_TOL, atol=1e-6)
    np.testing.assert_allclose(pe["normal"], po["normal"], rtol=0, atol=REL_TOL)
    tot, bad = maps_close(o, e, sc.nviews)
    same = float((pe["coord"] == po["coord"]).all(axis=1).mean())
    print(what, "pool", po.shape[0], "map cells", tot, "bad", bad, "bit-equal coordinates", same)
    assert bad == 0 and tot > 2000, (what, tot, bad)
    assert same > 0.99, (what, same)
    return po


def seeds_for_sizes(sc, seeds, sizes, level):
    """make_seeds lists every view that sees the point inside the scene's full image; a view cropped to sizes[v] sees less.  The
    same rule with the view's own size: a view is listed only if the point projects at least 8 pixels inside its image, and a seed
    whose reference view is not is dropped -- the reference indexes m_pgrids with a patch's m_grids unchecked (filter.cpp:113-119),
    so a record that lists a view outside whose grid it lies is not an input it takes."""
    P = sc.P.astype(np.float64)
    out = []
    for s in seeds:
        keep = []
        for v in s["images"][: s["nimages"]]:
            x = P[v] @ s["coord"].astype(np.float64)
            u, w = x[0] / x[2], x[1] / x[2]
            if x[2] > 0 and 8 <= u < sizes[v][0] - 8 and 8 <= w < sizes[v][1] - 8:
                keep.append(int(v))
            elif v == s["images"][0]:
                keep = []
                break
        if len(keep) >= 2:
            r = s.copy()
            r["images"][:] = 0
            r["images"][: len(keep)] = keep
            r["nimages"] = len(keep)
            out.append(r)
    return np.array(out, dtype=seeds.dtype)


@contextmanager
def sweep_grid(n):
    """MVS_SWEEP_GRID=<n> around the engine calls of the block (None: the default grid), restored afterwards"""
    old = os.environ.pop("MVS_SWEEP_GRID", None)
    if n is not None:
        os.environ["MVS_SWEEP_GRID"] = str(n)
    try:
        yield
    finally:
        os.environ.pop("MVS_SWEEP_GRID", None)
        if old is not None:
            os.environ["MVS_SWEEP_GRID"] = old


def pools_match_oracle(po, pe):
    assert po.shape == pe.shape and po.shape[0] > 0, f"pools of {po.shape} (oracle) and {pe.shape} (engine) records"
    np.testing.assert_array_equal(po["nimages"], pe["nimages"])
    np.testing.assert_array_equal(po["images"], pe["images"])
    np.testing.assert_array_equal(po["vimages"], pe["vimages"])
    np.testing.assert_allclose(pe["coord"], po["coord"], rtol=REL_TOL, atol=1e-6)
    np.testing.assert_allclose(pe["normal"], po["normal"], rtol=0, atol=REL_TOL)
    for k in range(0, po.shape[0], max(po.shape[0] // 64, 1)):
        cmp_records(pe[k], po[k], f"record {k}")


def two_iterations(x):
    """Propagate::run(0), Filter::run, updateThreshold (m_depth 2: Optim::check from here), Propagate::run(1)"""
    counters, removed = [], []
    counters.append(x.propagate(0))
    r = x.filter()
    removed.append([r[k] for k in REMOVALS])
    x.update_threshold()
    counters.append(x.propagate(1))
    return counters, removed


def cells_in_ref_view(sc, seeds, csize=2):
    """Cell (cx, cy) of every seed in its reference view: PatchManager::setGrids, patch_manager.cpp:241-250."""
    ref = seeds["images"][:, 0].astype(np.int64)
    P = sc.P.astype(np.float64)[ref]
    X = seeds["coord"].astype(np.float64)
    x = np.einsum("nij,nj->ni", P, X)
    px, py = x[:, 0] / x[:, 2], x[:, 1] / x[:, 2]
    return np.floor(px + 0.5).astype(np.int64) // csize, np.floor(py + 0.5).astype(np.int64) // csize


def refiner_oracle(nviews, minImageNum=3, list_cap=0):
    kw = dict(level=0, csize=2, wsize=7, minImageNum=minImageNum, schedule=ob.SCHEDULE_ENGINE, sum_mode=ob.SUM_TREE64, enable_check=0, nthreads=8)
    if list_cap:
        kw["list_cap"] = list_cap
    return ob.Oracle(nviews, **kw)


def refiner_candidates(o, scene, n=200, stride=6, seed=31):
    """seeds that pass Optim::preProcess, as the refiner receives them"""
    out = []
    for s in synth.make_seeds(scene, stride=stride, seed=seed):
        f, r = o.preprocess(s)
        if f == 0:
            out.append(r)
        if len(out) >= n:
            break
    return np.array(out, dtype=o.dtype)


def probe_vs_restatement(scene, minImageNum, list_cap, max_evals=500, xtol=1e-4):
    """the CONVERGED refiner through the probe against tests/refiner_restatement.py on the oracle's cost_func (rd0 = ra0 = 4,
    mvs_default_config).  With the reference's budget of 500 evaluations at least 90 % of the runs must converge; a smaller budget
    cuts runs short in the restatement too, and the engine's converged share must then lie within 0.1 of the restatement's."""
    F = np.float32
    o = refiner_oracle(scene.nviews, minImageNum, list_cap)
    o.set_scene(scene)
    cands = refiner_candidates(o, scene, n=120)
    assert cands.shape[0] >= 60
    e = engine.Engine(scene.nviews, list_cap=list_cap or None, level=0, csize=2, wsize=7, minImageNum=minImageNum, enable_check=0)
    e.set_scene(scene)
    e.set_refiner("converged", max_evals=max_evals, xtol=xtol)
    rec, xf, ni = e.probe(engine.PROBE_REFINE_X, cands)
    rec2, xf2, ni2 = e.probe(engine.PROBE_REFINE_X, cands)
    assert rec.tobytes() == rec2.tobytes() and xf.tobytes() == xf2.tobytes() and ni.tobytes() == ni2.tobytes()  # deterministic
    plain, _, _ = e.probe(engine.PROBE_REFINE, cands)
    assert plain.tobytes() == rec.tobytes(), "PROBE_REFINE and PROBE_REFINE_X give different records"
    agree, same_cost, worst, ev_e, ev_r, conv_r = 0, 0, 0.0, [], [], 0
    for j, c in enumerate(cands):
        x = rr.clamp_angles(o.encode(c))
        f0 = o.cost(c, x)
        fe = o.cost(c, xf[j, :3])
        worst = max(worst, abs(float(xf[j, 3]) - fe))
        assert abs(float(xf[j, 3]) - fe) <= 1e-5, (j, xf[j], fe)
        assert fe <= f0 + 1e-5, (j, fe, f0)
        assert 0 < abs(int(ni[j])) <= max_evals
        xs, fs, n, conv = rr.refine_converged(lambda y, c=c: o.cost(c, np.asarray(y, F)), x, 4.0, 4.0, max_evals, xtol)
        same_x = np.all(np.abs(xf[j, :3] - xs) <= 1e-5 * np.maximum(1.0, np.abs(xs)))
        agree += int(same_x and (n if conv else -n) == int(ni[j]))
        same_cost += int(abs(fe - fs) <= 1e-5)
        ev_e.append(abs(int(ni[j])))
        ev_r.append(n)
        conv_r += int(conv)
    print(f"{scene.nviews} views, list cap {e.list_cap}: same trajectory {agree}/{cands.shape[0]}, same final cost (1e-5) {same_cost}, "
          f"worst reported-cost difference {worst:.3g}, evals median {np.median(ev_e):.0f} (restatement {np.median(ev_r):.0f}), "
          f"converged {float((ni > 0).mean()):.3f} (restatement {conv_r / cands.shape[0]:.3f})")
    # The kernel's four-proposal passes use the class-lane pivot sums, orc_cost the two-pass form: they differ by ~1e-7, and near the
    # minimum the costs of the vertices differ by less than that, so most trajectories part in their last iterations and end at other
    # points of the same flat valley (same trajectory 8/120 and 18/120 on the GPU; the restatement with 2e-7 of noise
    # added to its costs agrees with itself on none).  What must agree is where they end: the cost, and about how long it takes.
    assert same_cost >= 0.9 * cands.shape[0]
    assert abs(np.median(ev_e) - np.median(ev_r)) <= 0.1 * np.median(ev_r)
    assert agree >= 0.05 * cands.shape[0]
    if max_evals >= 500:
        assert (ni > 0).mean() >= 0.9
    else:
        assert abs(float((ni > 0).mean()) - conv_r / cands.shape[0]) <= 0.1
    e.close()
    o.close()
