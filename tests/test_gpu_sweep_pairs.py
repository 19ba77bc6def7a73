"""The sweep refines two consecutive trials of a destination cell in ONE pass of the frame-lane arithmetic where the second is certain
to find room (refine_patch_pair).  Which trials are refined together must not change a bit of the result: every case
runs the HIP engine with the pairing on and with MVS_SWEEP_PAIR=0 (read on every launch: every trial alone) and asserts that the two pools
are the same bytes, the two counter lists equal, and both equal to the CPU oracle's (ENGINE schedule) with the pool matching it as
parity_support.pools_match_oracle does.

mvs_engine_sweep_pairs (Engine.sweep_pairs) says how the trials were refined; every case asserts the statistic it is about, so that
none passes without having met what it is named for, and that nothing is refined as a pair with the switch off."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

import oracle_binding as ob
from mvskit_amd import engine, synth
from parity_support import COUNTERS, GRID_KW, REMOVALS, SEEDED, dense_pool, pools_match_oracle, sweep_grid, two_iterations

pytestmark = pytest.mark.gpu


@contextmanager
def _pairing(on):
    """MVS_SWEEP_PAIR around the engine calls of the block: unset (the default: on) or 0, restored afterwards"""
    old = os.environ.pop("MVS_SWEEP_PAIR", None)
    if not on:
        os.environ["MVS_SWEEP_PAIR"] = "0"
    try:
        yield
    finally:
        os.environ.pop("MVS_SWEEP_PAIR", None)
        if old is not None:
            os.environ["MVS_SWEEP_PAIR"] = old


def _iterations(n, with_filter=True):
    """n times Propagate::run, with Filter::run and updateThreshold in between (m_depth 2 from the second: Optim::check, if enabled)"""
    def run(x):
        counters, removed = [], []
        for it in range(n):
            counters.append(x.propagate(it))
            if it + 1 < n:
                if with_filter:
                    r = x.filter()
                    removed.append([r[k] for k in REMOVALS])
                x.update_threshold()
        return counters, removed
    return run


def _engine_run(sc, pool, plan, on, grid=None, refiner=None, before=None, **ekw):
    """-> (counters, removals, pool, sweep_pairs, timing of the last sweep) of a fresh engine"""
    kw = dict(level=0, csize=2, wsize=7, minImageNum=3, enable_check=0)
    kw.update(ekw)
    e = engine.Engine(sc.nviews, **kw)
    if refiner:
        e.set_refiner(refiner)
    e.set_scene(sc)
    with _pairing(on), sweep_grid(grid):
        e.upload_patches(pool)
        if before:
            before(e)
        c, r = plan(e)
        t = e.timing()
        p = e.patches()
        s = e.sweep_pairs()
    e.close()
    assert set(s) == set(engine.Engine.SWEEP_PAIR_KEYS) and all(v >= 0 for v in s.values()), s
    return c, r, p, s, t


def _oracle_run(sc, pool, plan, before=None, **kw):
    """-> (counters, removals, pool) of the CPU oracle as parity_support.pair sets it up"""
    okw = dict(level=0, csize=2, wsize=7, minImageNum=3, schedule=ob.SCHEDULE_ENGINE, sum_mode=ob.SUM_TREE64, enable_check=0, nthreads=8)
    okw.update(kw)
    o = ob.Oracle(sc.nviews, **okw)
    o.set_scene(sc)
    o.add_patches(pool)
    if before:
        before(o)
    c, r = plan(o)
    p = o.patches()
    o.close()
    return c, r, p


def _check_case(oracle, on, off):
    """the assertions every case shares; -> (the statistics with the pairing on, the oracle's counters summed over the iterations)"""
    oc, orem, po = oracle
    c1, r1, p1, s1, _ = on
    c0, r0, p0, s0, _ = off
    print("oracle", oc)
    print("pairing on ", s1)
    print("pairing off", s0)
    assert p1.shape == p0.shape and p1.tobytes() == p0.tobytes()
    assert c1 == c0 and r1 == r0
    for it in range(len(oc)):
        assert set(COUNTERS) <= set(oc[it]) and oc[it] == c1[it], (it, oc[it], c1[it])
    assert orem == r1
    pools_match_oracle(po, p1)
    # with the switch off the same trials wait for each other and are then refined one by one
    assert s0["paired"] == 0 and s0["can_pair"] == s1["can_pair"] == s1["paired"], (s0, s1)
    for k in engine.Engine.SWEEP_PAIR_KEYS[1:5]:
        assert s0[k] == s1[k], (k, s0, s1)
    assert s1["paired"] % 2 == 0
    return s1, {k: sum(c[k] for c in oc) for k in COUNTERS}


# ------------------------------------------------------------------ 1. plain pairs with Optim::check; the grid size
@pytest.fixture(scope="module")
def plane_case():
    """test_gpu_sweep_resident.py's grid scene (3 views of 130 x 98 `plane`, seeds at stride 3, two iterations, the second with
    Optim::check): the oracle and the engine without pairing, computed once and left unchanged"""
    sc = synth.make_scene(nviews=3, W=130, H=98, arc_deg=30.0, radius=4.0, kind="plane")
    seeds = synth.make_seeds(sc, stride=3, seed=5)
    oracle = _oracle_run(sc, seeds, two_iterations, **GRID_KW)
    off = _engine_run(sc, seeds, two_iterations, False, **GRID_KW)
    return sc, seeds, oracle, off


@pytest.mark.parametrize("grid", [None, 1])
def test_plain_pairs_with_check(plane_case, grid):
    """max_propag 2 and sparse lists: nearly every source entry gives two trials that can pair, in both iterations.  One resident
    wave (MVS_SWEEP_GRID=1) runs every cell, pairs and all, one after the other: the stash and the working block of one cell's pair must
    not leak into the next cell."""
    sc, seeds, oracle, off = plane_case
    on = _engine_run(sc, seeds, two_iterations, True, grid=grid, **GRID_KW)
    s, tot = _check_case(oracle, on, off)
    assert s["paired"] > 1000 and tot["patches"] > 2000
    assert oracle[0][1]["patches"] > 1000  # the iteration with Optim::check has its share of them


# ------------------------------------------------------------------ 2. lists that fill up
FILL_SEED = 5  # make_seeds' seed of the case below: the oracle alone shows replaced > 0 with it


def test_lists_that_fill_up():
    """Seeds in every cell and three iterations at cap = max_propag * csize^2 = 8: lists reach 6, 7 and 8 entries, so cells go from
    "room for two" over "room for one" (the trial is refined alone, no guaranteed room) to the replace-worst branch."""
    sc = synth.make_scene(nviews=3, W=64, H=48, arc_deg=30.0, radius=4.0, kind="multi")
    seeds = synth.make_seeds(sc, stride=1, seed=FILL_SEED)
    kw = dict(minImageNum=2, seed=11, enable_check=1)
    plan = _iterations(3)
    oracle = _oracle_run(sc, seeds, plan, **kw)
    on = _engine_run(sc, seeds, plan, True, **kw)
    off = _engine_run(sc, seeds, plan, False, **kw)
    s, tot = _check_case(oracle, on, off)
    assert s["paired"] > 0 and s["alone_no_room"] > 0, s
    assert tot["replaced"] > 0 and tot["prefiltered"] > 0, tot


# ------------------------------------------------------------------ 3. a partner that fails
def test_partner_that_fails():
    """`multi` has depth edges: trials generated across them fail preProcess (fail0), some of them while a candidate waits -- the slot
    goes to the next trial, or the waiting candidate is refined alone when none comes."""
    sc = synth.make_scene(nviews=3, W=128, H=88, arc_deg=30.0, radius=4.0, kind="multi")
    seeds = synth.make_seeds(sc, stride=2, seed=5)
    kw = dict(minImageNum=2, seed=7, enable_check=1)
    plan = _iterations(2)
    oracle = _oracle_run(sc, seeds, plan, **kw)
    on = _engine_run(sc, seeds, plan, True, **kw)
    off = _engine_run(sc, seeds, plan, False, **kw)
    s, tot = _check_case(oracle, on, off)
    assert tot["fail0"] > 0 and s["alone_partner_failed"] > 0 and s["paired"] > 0, (s, tot)


# ------------------------------------------------------------------ 4. odd trial counts and a third source
@pytest.mark.parametrize("max_propag", [1, 3])
def test_odd_trial_counts_and_a_third_source(small_multi_scene, max_propag):
    """View propagation: the cell's own list is a third source.  max_propag 1: nothing pairs within a source entry, a pair is two
    entries' trials (of one source list or of two); 3: every entry leaves an odd trial, which pairs with the next entry's first or is
    refined alone at the end of the cell.  The two-seeded-views-of-five scene of test_gpu_sweep_joblist.py."""
    sc = small_multi_scene
    seeds = synth.make_seeds(sc, stride=4, seed=23, views=list(SEEDED))
    kw = dict(seed=5, view_propagation=1, max_propag=max_propag)
    plan = _iterations(1)  # (a second iteration at max_propag 3 is 570 000 trials: half a minute of oracle)
    oracle = _oracle_run(sc, seeds, plan, **kw)
    on = _engine_run(sc, seeds, plan, True, **kw)
    off = _engine_run(sc, seeds, plan, False, **kw)
    s, tot = _check_case(oracle, on, off)
    assert s["paired"] > 0 and s["alone_no_partner"] > 0, s
    assert tot["patches"] > 0


# ------------------------------------------------------------------ 5. a cell that gives up with a candidate pending
def test_cell_that_gives_up_with_a_candidate_pending(small_plane_scene):
    """The dense cells of test_gpu_sweep_joblist.py::test_cell_that_gives_up_is_followed_by_listed_cells (30 patches per cell,
    max_propag 8, two resident waves): a cell whose Optim::check outgrows the LDS id set gives up in the middle of finishing a pair --
    the second candidate is dropped with everything else of the cell, and the second tier runs the cell again, pairs and all."""
    sc = small_plane_scene
    pool = dense_pool(sc, per_cell=30, window=5)
    kw = dict(seed=4, enable_check=1, minImageNum=2, max_propag=8)

    def before(x):
        x.update_threshold()  # m_depth 2: Optim::check runs

    def plan(x):
        return [x.propagate(1)], []

    oracle = _oracle_run(sc, pool, plan, before=before, **kw)
    on = _engine_run(sc, pool, plan, True, grid=2, before=before, **kw)
    off = _engine_run(sc, pool, plan, False, grid=2, before=before, **kw)
    s, tot = _check_case(oracle, on, off)
    assert on[4]["check_retried_cells"] > 0 and off[4]["check_retried_cells"] == on[4]["check_retried_cells"], (on[4], off[4])
    assert s["paired"] > 0, s
    assert (on[2]["coord"] == oracle[2]["coord"]).all(axis=1).mean() > 0.99


# ------------------------------------------------------------------ 6. the CONVERGED refiner keeps the single path
def test_converged_refiner_never_pairs(small_multi_scene):
    """The simplex refiner is not paired: the same candidates wait for each other and are refined one by one, switch on or off."""
    sc = small_multi_scene
    seeds = synth.make_seeds(sc, stride=4, seed=21)
    kw = dict(seed=3, enable_check=1)
    plan = _iterations(2)
    c1, r1, p1, s1, _ = _engine_run(sc, seeds, plan, True, refiner="converged", **kw)
    c0, r0, p0, s0, _ = _engine_run(sc, seeds, plan, False, refiner="converged", **kw)
    print("pairing on ", s1, "off", s0)
    assert p1.shape[0] > seeds.shape[0] and p1.tobytes() == p0.tobytes() and c1 == c0 and r1 == r0
    assert s1 == s0 and s1["paired"] == 0 and s1["can_pair"] > 0, (s1, s0)
