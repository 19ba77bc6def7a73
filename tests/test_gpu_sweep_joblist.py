"""The sweep's job lists: before every launch a thread per job lists, per XCD queue, the jobs whose destination
cell will run at least one trial, and the resident waves take from those lists.  A job that is listed without need costs time only;
a job that is NOT listed although it has a trial loses patches -- so every case here compares the HIP engine with the CPU oracle
(ENGINE schedule), at the shapes where the listing, its queue-major layout and the takes can go wrong.

mvs_timing.sweep_jobs_listed is the number of jobs the waves were handed (one pass: that pass; a propagate: both passes)."""
import numpy as np
import pytest

from mvskit_amd import engine, synth
from parity_support import COUNTERS, GRID_KW, REL_TOL, SEEDED, dense_pool, grid_of, pair, pair_sized, pools_match_oracle, seeds_for_sizes, sweep_grid

pytestmark = pytest.mark.gpu


def _jobs_of_view(e, v):
    gw, gh = e.grid_dims(v)
    return ((gw + 1) // 2) * gh


def _propagate_by_passes(e, it):
    """mvs_engine_propagate as its two passes with local commits; -> (the summed counters, sweep_jobs_listed of each pass)"""
    total, listed = dict.fromkeys(COUNTERS, 0), []
    for p in range(2):
        c = e.engine_pass(it, p)
        listed.append(e.timing()["sweep_jobs_listed"])
        e.commit_local()
        for k in COUNTERS:
            total[k] += c[k]
    return total, listed


# ------------------------------------------------------------------ 1. listing too few jobs; view propagation
@pytest.fixture(scope="module")
def two_of_five(small_multi_scene):
    """Seeds in views 0 and 2 of 5: the cells of views 1, 3 and 4 hold memberships of those patches but no patch whose reference
    view is their own, so in the first pass none of their jobs has a trial without view propagation -- and with it, those
    memberships are the only source of their jobs."""
    sc = small_multi_scene
    return sc, synth.make_seeds(sc, stride=4, seed=23, views=list(SEEDED))


def test_two_seeded_views_of_five_with_check(two_of_five):
    sc, seeds = two_of_five
    o, e = pair(sc, seed=5, enable_check=1)
    o.add_patches(seeds)
    e.upload_patches(seeds)
    bound = sum(_jobs_of_view(e, v) for v in SEEDED)
    for it in range(2):
        co = o.propagate(it)
        ce, listed = _propagate_by_passes(e, it)
        print("iteration", it, "oracle", co, "engine", ce, "listed", listed, "bound", bound)
        assert set(COUNTERS) <= set(co) and all(co[k] == ce[k] for k in COUNTERS), (it, co, ce)
        # only an entry whose reference view is the swept view starts a trial, and the pool of the first pass holds the seeds of
        # two views only: no job of views 1, 3, 4 is listed there
        if it == 0:
            assert listed[0] <= bound, (listed, bound)
        # (The seeds sit on cells with cx + cy even, every fourth cell: colour 0 of iteration 0 has no source, colour 1 has.)
        assert sum(listed) > 0, (it, listed)
        o.update_threshold()
        e.update_threshold()  # m_depth 2: Optim::check in the second iteration
    assert co["patches"] > 0
    pools_match_oracle(o.patches(), e.patches())
    o.close()
    e.close()


def test_view_propagation_lists_the_own_cell_sources(two_of_five):
    sc, seeds = two_of_five
    o, e = pair(sc, seed=5, view_propagation=1)
    e0 = engine.Engine(sc.nviews, level=0, csize=2, wsize=7, minImageNum=3, enable_check=0, seed=5)
    e0.set_scene(sc)
    o.add_patches(seeds)
    e.upload_patches(seeds)
    e0.upload_patches(seeds)
    e0.engine_pass(0, 0)
    plain = e0.timing()["sweep_jobs_listed"]
    e0.close()
    for it in range(2):
        co = o.propagate(it)
        ce, listed = _propagate_by_passes(e, it)
        print("iteration", it, "oracle", co, "engine", ce, "listed", listed, "without view propagation", plain)
        assert all(co[k] == ce[k] for k in COUNTERS), (it, co, ce)
        if it == 0:
            # the same index: every job listed without view propagation is listed with it (in this pass none: the seeds' cells
            # have cx + cy even, as colour 0's destinations), and so are the cells that hold a membership of another view's patch
            assert listed[0] > plain >= 0, (listed, plain)
    po, pe = o.patches(), e.patches()  # as test_gpu_parity.py::test_view_propagation_matches_oracle
    assert po.shape == pe.shape and po.shape[0] > seeds.shape[0]
    np.testing.assert_array_equal(po["nimages"], pe["nimages"])
    np.testing.assert_array_equal(po["images"], pe["images"])
    np.testing.assert_allclose(pe["coord"], po["coord"], rtol=REL_TOL, atol=1e-6)
    np.testing.assert_allclose(pe["normal"], po["normal"], rtol=0, atol=REL_TOL)
    o.close()
    e.close()


# ------------------------------------------------------------------ 2. a pass with no source anywhere
def test_pass_without_any_source(small_plane_scene):
    """Seeds at stride 2 sit on the cells (odd, odd): cx + cy is even everywhere.  Colour 0 of iteration 0 sweeps the cells with
    cx + cy even from the cells above and to the left, where cx + cy is odd: no list there holds a patch of the swept view (the
    memberships that other views' patches leave there do not count).  m_ncc is set, so the pass scores no seed either."""
    sc = small_plane_scene
    seeds = synth.make_seeds(sc, stride=2, seed=3)
    seeds["ncc"] = 0.5
    ref = seeds["images"][:, 0].astype(int)
    x = np.einsum("nij,nj->ni", sc.P[ref].astype(np.float64), seeds["coord"].astype(np.float64))
    ix, iy = np.floor(x[:, 0] / x[:, 2] + 0.5).astype(int) // 2, np.floor(x[:, 1] / x[:, 2] + 0.5).astype(int) // 2  # PatchManager's cell
    assert seeds.shape[0] > 1000 and (ix % 2 == 1).all() and (iy % 2 == 1).all()
    e = engine.Engine(sc.nviews, level=0, csize=2, wsize=7, minImageNum=2, enable_check=0, seed=9)
    e.set_scene(sc)
    e.upload_patches(seeds)
    before = e.patches()
    c = e.engine_pass(0, 0)
    t = e.timing()
    e.commit_local()
    after = e.patches()
    print("counters", c, "timing", t)
    assert t["sweep_jobs_listed"] == 0, t
    assert all(c[k] == 0 for k in COUNTERS), c
    assert after.shape == before.shape and after.tobytes() == before.tobytes()
    c1 = e.engine_pass(0, 1)  # the other colour has the sources
    assert e.timing()["sweep_jobs_listed"] > seeds.shape[0] // 2 and c1["inserted"] > 0
    e.commit_local()
    e.close()


# ------------------------------------------------------------------ 3. awkward shapes
def _case_odd_width():
    """65 x 49 cells: a ghost job (cx == gw) in every other row; 4851 jobs per colour = 37 chunks of 128 and one of 115, 38 chunks
    over 8 queues (queues 0-5 hold five, 6-7 four)"""
    sc = synth.make_scene(nviews=3, W=130, H=98, arc_deg=30.0, radius=4.0, kind="plane")
    o, e = pair(sc, minImageNum=2, seed=11)
    assert e.grid_dims(0) == (65, 49) and sum(_jobs_of_view(e, v) for v in range(3)) == 4851 and 4851 % 128 == 115
    return o, e, synth.make_seeds(sc, stride=3, seed=5)


def _case_less_than_a_chunk():
    """8 x 6 cells in 2 views: 48 jobs, one partial chunk in queue 0 and seven empty queues"""
    sc = synth.make_scene(nviews=2, W=16, H=12, arc_deg=10.0, radius=4.0, kind="plane")
    o, e = pair(sc, minImageNum=2, seed=5)
    assert sum(_jobs_of_view(e, v) for v in range(2)) == 48
    return o, e, synth.make_seeds(sc, stride=1, seed=5)


def _case_unequal_views():
    """1376 + 1240 + 1344 jobs: chunks 10 and 20 of the 31 straddle two views"""
    sizes = [(128, 86), (121, 80), (128, 83)]
    sc = synth.make_scene(nviews=3, W=128, H=88, arc_deg=30.0, radius=4.0, kind="multi")
    o, e = pair_sized(sc, sizes=sizes, level=0, csize=2, wsize=7, minImageNum=2, seed=7)
    assert [e.grid_dims(v) for v in range(3)] == [grid_of(w, h, 0, 2) for w, h in sizes]
    assert [_jobs_of_view(e, v) for v in range(3)] == [1376, 1240, 1344]
    return o, e, seeds_for_sizes(sc, synth.make_seeds(sc, level=0, csize=2, stride=2, seed=5), sizes, 0)


@pytest.mark.parametrize("make", [_case_odd_width, _case_less_than_a_chunk, _case_unequal_views])
def test_awkward_shapes(make):
    o, e, seeds = make()
    njobs = sum(_jobs_of_view(e, v) for v in range(e.cfg.nviews))
    o.add_patches(seeds)
    e.upload_patches(seeds)
    co, ce = o.propagate(0), e.propagate(0)
    listed = e.timing()["sweep_jobs_listed"]
    print("seeds", seeds.shape[0], "oracle", co, "engine", ce, "listed", listed, "of", 2 * njobs)
    assert set(COUNTERS) <= set(co) and co == ce, (co, ce)
    assert co["inserted"] > 0 and 0 < listed <= 2 * njobs
    pools_match_oracle(o.patches(), e.patches())
    o.close()
    e.close()


# ------------------------------------------------------------------ 4. the grid size must not matter
def _two_iterations(e, seeds):
    e.upload_patches(seeds)
    c = [e.propagate(0)]
    listed = [e.timing()["sweep_jobs_listed"]]
    e.update_threshold()
    c.append(e.propagate(1))
    listed.append(e.timing()["sweep_jobs_listed"])
    return c, listed, e.patches()


@pytest.fixture(scope="module")
def grid_default():
    sc = synth.make_scene(nviews=3, W=130, H=98, arc_deg=30.0, radius=4.0, kind="plane")
    seeds = synth.make_seeds(sc, stride=3, seed=5)
    e = engine.Engine(sc.nviews, **GRID_KW)
    e.set_scene(sc)
    with sweep_grid(None):
        res = _two_iterations(e, seeds)
    e.close()
    return sc, seeds, res


@pytest.mark.parametrize("grid", [1, 3, 9])
def test_lists_are_drained_at_any_grid_size(grid_default, grid):
    """One wave drains all eight lists by stealing; 3 and 9 leave queues without a wave of their own or with unequal numbers.  The
    lists do not depend on the grid, and neither does a bit of the pool (two iterations, the second with Optim::check)."""
    sc, seeds, (cd, ld, pd) = grid_default
    e = engine.Engine(sc.nviews, **GRID_KW)
    e.set_scene(sc)
    with sweep_grid(grid):
        c, listed, p = _two_iterations(e, seeds)
    e.close()
    print("grid", grid, "listed", listed, "counters", c)
    assert c == cd and listed == ld and ld[0] > 0 and ld[1] > 0
    assert p.shape == pd.shape and p.shape[0] > 1000
    assert p.tobytes() == pd.tobytes()


# ------------------------------------------------------------------ 5. a cell that gives up is followed by clean cells from the list
def test_cell_that_gives_up_is_followed_by_listed_cells(small_plane_scene):
    """The scene of test_gpu_sweep_resident.py::test_cell_that_gives_up_is_followed_by_clean_cells: a wave whose cell goes to the
    second tier takes the next entry of its list; the second tier runs the cells of retry_jobs as before."""
    sc = small_plane_scene
    pool = dense_pool(sc, per_cell=30, window=5)
    o, e = pair(sc, seed=4, enable_check=1, minImageNum=2, max_propag=8)
    o.add_patches(pool)
    e.upload_patches(pool)
    o.update_threshold()
    e.update_threshold()
    co = o.propagate(1)
    with sweep_grid(2):
        ce = e.propagate(1)
        t = e.timing()
    print("oracle", co, "engine", ce, "timing", t)
    assert t["check_retried_cells"] > 0 and t["sweep_jobs_listed"] > t["check_retried_cells"], t
    assert set(COUNTERS) <= set(co) and co == ce, (co, ce)
    po, pe = o.patches(), e.patches()
    pools_match_oracle(po, pe)
    assert (pe["coord"] == po["coord"]).all(axis=1).mean() > 0.99
    o.close()
    e.close()
