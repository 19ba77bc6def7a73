"""A trial of the sweep into a FULL cell (the replace-worst branch) draws nothing before Optim::refinePatch: generatePatch, the pre-filter
and preProcess are functions of the source patch, the cell's worst patch and the index.  When such a trial ends before the refinement,
the trials of the same source entry still to come would compute the same and end the same way; the engine adds their counts -- the
evaluations included -- and does not run them (sweep_cell).  That must not change a bit of the result: every case
compares the HIP engine with the CPU oracle (ENGINE schedule), the pool as parity_support.pools_match_oracle does and every counter of
every iteration for equality.

mvs_engine_sweep_repeats (Engine.sweep_repeats) says how many trials were not run; every case asserts the statistic it is about, so
that none passes without having met its path.  `from_stash` (a trial that takes over the candidate the trial before it brought through
preProcess) is not built: it is 0 everywhere."""
import pytest

import oracle_binding as ob
from mvskit_amd import engine, synth
from parity_support import COUNTERS, REMOVALS, SEEDED, dense_pool, grid_of, pools_match_oracle, sweep_grid

pytestmark = pytest.mark.gpu


def _iterations(n):
    """n times Propagate::run, with Filter::run and updateThreshold in between (m_depth 2 from the second: Optim::check, if enabled)"""
    def run(x):
        counters, removed = [], []
        for it in range(n):
            counters.append(x.propagate(it))
            if it + 1 < n:
                r = x.filter()
                removed.append([r[k] for k in REMOVALS])
                x.update_threshold()
        return counters, removed
    return run


def _engine_run(sc, pool, plan, grid=None, before=None, **ekw):
    """-> (counters, removals, pool, sweep_repeats, timing of the last sweep) of a fresh engine"""
    kw = dict(level=0, csize=2, wsize=7, minImageNum=3, enable_check=0)
    kw.update(ekw)
    e = engine.Engine(sc.nviews, **kw)
    e.set_scene(sc)
    with sweep_grid(grid):
        e.upload_patches(pool)
        if before:
            before(e)
        c, r = plan(e)
        t = e.timing()
        p = e.patches()
        s = e.sweep_repeats()
    e.close()
    assert set(s) == set(engine.Engine.SWEEP_REPEAT_KEYS) and all(v >= 0 for v in s.values()), s
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


def _check_case(oracle, eng):
    """the assertions every case shares; -> (the statistic, the oracle's counters summed over the iterations)"""
    oc, orem, po = oracle
    c, r, p, s, _ = eng
    print("oracle", oc)
    print("engine", c)
    print("repeats", s)
    assert len(oc) == len(c)
    for it in range(len(oc)):
        assert set(COUNTERS) <= set(oc[it]) and oc[it] == c[it], (it, oc[it], c[it])
    assert orem == r
    pools_match_oracle(po, p)
    assert s["from_stash"] == 0, s
    return s, {k: sum(x[k] for x in oc) for k in COUNTERS}


# ------------------------------------------------------------------ 1., 2., 5. lists that fill up
FILL_KW = dict(minImageNum=2, seed=11, enable_check=1)


@pytest.fixture(scope="module")
def fill_scene():
    """test_gpu_sweep_pairs.py::test_lists_that_fill_up's scene: seeds in every cell of 3 views of 64 x 48 `multi`"""
    sc = synth.make_scene(nviews=3, W=64, H=48, arc_deg=30.0, radius=4.0, kind="multi")
    return sc, synth.make_seeds(sc, stride=1, seed=5)


@pytest.fixture(scope="module")
def fill_oracle(fill_scene):
    """three iterations at max_propag 2 (cap 8) on the oracle, computed once and left unchanged"""
    sc, seeds = fill_scene
    return _oracle_run(sc, seeds, _iterations(3), **FILL_KW)


@pytest.mark.parametrize("grid", [None, 1])
def test_lists_that_fill_up(fill_scene, fill_oracle, grid):
    """Lists reach cap = 8 and trials are pre-filtered against the worst patch, in pairs: trial 0 of a source entry pre-filtered means trial 1
    pre-filtered, and trial 1 is skipped.  A pre-filtered trial is alone only where the list changed between the two trials of its
    entry -- trial 0 replaced the worst patch (or, once per cell at most, took the last free place) --: skipped >= prefiltered / 2 -
    replaced.  One resident wave (MVS_SWEEP_GRID=1) runs every cell: what one cell counted and skipped must not leak into the next."""
    sc, seeds = fill_scene
    eng = _engine_run(sc, seeds, _iterations(3), grid=grid, **FILL_KW)
    s, tot = _check_case(fill_oracle, eng)
    print("skipped", s["skipped"], "prefiltered", tot["prefiltered"], "replaced", tot["replaced"])
    assert tot["replaced"] > 0 and tot["prefiltered"] > 0, tot
    assert s["skipped"] > 0, s
    assert 2 * s["skipped"] >= tot["prefiltered"] - 2 * tot["replaced"], (s, tot)


@pytest.mark.parametrize("max_propag", [1, 3])
def test_one_and_three_trials_per_entry(fill_scene, max_propag):
    """max_propag 1: no trial has a predecessor, nothing can repeat.  3: an early outcome of trial 0 skips two trials, one of trial 1 one."""
    sc, seeds = fill_scene
    kw = dict(FILL_KW, max_propag=max_propag)
    oracle = _oracle_run(sc, seeds, _iterations(3), **kw)
    # the engine's pool sized for MAX_NUM_OF_PATCHES = max_propag * csize^2 patches in every cell (the default holds four per cell)
    gw, gh = grid_of(sc.W, sc.H, 0, 2)
    eng = _engine_run(sc, seeds, _iterations(3), max_patches=sc.nviews * gw * gh * max_propag * 4, **kw)
    s, tot = _check_case(oracle, eng)
    assert tot["prefiltered"] > 0 and tot["replaced"] > 0, tot
    if max_propag == 1:
        assert s["skipped"] == 0, s
    else:
        assert s["skipped"] > 0, s


# ------------------------------------------------------------------ 3. the third source
def test_third_source(small_multi_scene):
    """View propagation: the cell's own list is a third source, whose patches are re-anchored on the swept view's ray (as_view) -- still
    without a draw.  The seeds of test_gpu_sweep_pairs.py::test_odd_trial_counts_and_a_third_source at max_propag 2: the lists of the two
    seeded views fill within the first iteration (the oracle pre-filters and replaces in it)."""
    sc = small_multi_scene
    seeds = synth.make_seeds(sc, stride=4, seed=23, views=list(SEEDED))
    kw = dict(seed=5, view_propagation=1, max_propag=2)
    oracle = _oracle_run(sc, seeds, _iterations(1), **kw)
    eng = _engine_run(sc, seeds, _iterations(1), **kw)
    s, tot = _check_case(oracle, eng)
    assert tot["prefiltered"] > 0 and tot["replaced"] > 0, tot
    assert s["skipped"] > 0, s


# ------------------------------------------------------------------ 6. a cell that gives up
def test_cell_that_gives_up_adds_nothing(small_plane_scene):
    """The dense cells of test_gpu_sweep_pairs.py::test_cell_that_gives_up_with_a_candidate_pending (30 patches per cell, max_propag 8, two
    resident waves, m_depth 2): a cell whose Optim::check outgrows the LDS id set gives up and runs again on the second tier.  What it
    had counted, skipped trials included, is dropped with it -- the counters are the oracle's."""
    sc = small_plane_scene
    pool = dense_pool(sc, per_cell=30, window=5)
    kw = dict(seed=4, enable_check=1, minImageNum=2, max_propag=8)

    def before(x):
        x.update_threshold()  # m_depth 2: Optim::check runs

    def plan(x):
        return [x.propagate(1)], []

    oracle = _oracle_run(sc, pool, plan, before=before, **kw)
    eng = _engine_run(sc, pool, plan, grid=2, before=before, **kw)
    s, tot = _check_case(oracle, eng)
    assert eng[4]["check_retried_cells"] > 0, eng[4]
    assert tot["patches"] > 0
