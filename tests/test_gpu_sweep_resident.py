"""The sweep as a grid of resident waves that pull jobs from eight per-XCD queues of 128-job chunks: the shapes at
which that scheduling, and nothing else, can go wrong -- the HIP engine against the CPU oracle with the assertions of
test_gpu_parity.py::test_mixed_configurations, at grid sizes set through the development knob MVS_SWEEP_GRID (read on every launch).

Every cell runs the same instructions on the same inputs whatever wave takes it, so the number of resident waves must not change
a bit of the result: counters, the order of the pool and every field of every record."""
import numpy as np
import pytest

from mvskit_amd import engine, synth
from parity_support import COUNTERS, GRID_KW, dense_pool, grid_of, pair, pair_sized, pools_match_oracle, seeds_for_sizes, sweep_grid, two_iterations

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ 1. the grid size must not matter
@pytest.fixture(scope="module")
def grid_scene():
    """3 views of 130 x 98 at csize 2: a 65 x 49 grid, ceil(65 / 2) * 49 = 1617 jobs per view and 4851 per colour, i.e. 38 chunks of
    128 (not a multiple of 8; the last holds 115 jobs), with a ghost job (cx == gw) in every other row.  The oracle's two iterations
    (the second with Optim::check) and the engine's at the default grid are computed once and left unchanged."""
    sc = synth.make_scene(nviews=3, W=130, H=98, arc_deg=30.0, radius=4.0, kind="plane")
    seeds = synth.make_seeds(sc, stride=3, seed=5)
    o, e = pair(sc, **GRID_KW)
    assert e.grid_dims(0) == o.grid_dims(0) == grid_of(130, 98, 0, 2) == (65, 49)
    njobs = sum(((gw + 1) // 2) * gh for gw, gh in (e.grid_dims(v) for v in range(3)))
    assert njobs == 4851 and njobs % 128 != 0 and (-(-njobs // 128)) % 8 != 0
    o.add_patches(seeds)
    oc, orem = two_iterations(o)
    po = o.patches()
    o.close()
    with sweep_grid(None):
        e.upload_patches(seeds)
        ec, erem = two_iterations(e)
        pe = e.patches()
    e.close()
    return dict(scene=sc, seeds=seeds, oracle=(oc, orem, po), default=(ec, erem, pe))


def test_default_grid_matches_oracle(grid_scene):
    oc, orem, po = grid_scene["oracle"]
    ec, erem, pe = grid_scene["default"]
    print("oracle", oc, "engine", ec)
    for it in range(2):
        assert set(COUNTERS) <= set(oc[it])
        assert oc[it] == ec[it], (it, oc[it], ec[it])
    assert orem == erem
    assert oc[0]["inserted"] > 1000 and oc[1]["patches"] > 1000  # both iterations have work in most chunks
    pools_match_oracle(po, pe)


@pytest.mark.parametrize("grid", [1, 3, 8, 9])
def test_grid_size_does_not_matter(grid_scene, grid):
    """One wave drains all eight queues by stealing; 3 and 9 leave queues without a wave of their own or with unequal numbers;
    8 gives one wave per queue, which it works through alone (four or five chunks).  Counters equal to the oracle's (all ten names), the pool
    record for record what the default grid gave, every byte of it."""
    sc, seeds = grid_scene["scene"], grid_scene["seeds"]
    oc, orem, po = grid_scene["oracle"]
    _, _, pd = grid_scene["default"]
    e = engine.Engine(sc.nviews, **GRID_KW)
    e.set_scene(sc)
    with sweep_grid(grid):
        e.upload_patches(seeds)
        ec, erem = two_iterations(e)
        pe = e.patches()
    e.close()
    for it in range(2):
        assert all(oc[it][k] == ec[it][k] for k in COUNTERS), (grid, it, oc[it], ec[it])
        assert oc[it] == ec[it], (grid, it, oc[it], ec[it])
    assert orem == erem
    pools_match_oracle(po, pe)
    assert pe.shape == pd.shape
    np.testing.assert_array_equal(pe["coord"].view(np.uint32), pd["coord"].view(np.uint32))
    for f in pe.dtype.names:
        np.testing.assert_array_equal(pe[f], pd[f], err_msg=f)
    assert pe.tobytes() == pd.tobytes()


# ------------------------------------------------------------------ 2. fewer jobs than one chunk
def test_fewer_jobs_than_one_chunk():
    """2 views of 16 x 12: a grid of 8 x 6, 24 jobs per view and 48 per colour -- one partial chunk in queue 0, seven queues
    without any.  First a pass in which no cell has a source (the empty pool): all-zero counters, nothing staged (job_nstage zero
    everywhere: inserted + replaced == 0 and the pool as it was).  Then one iteration on seeds."""
    sc = synth.make_scene(nviews=2, W=16, H=12, arc_deg=10.0, radius=4.0, kind="plane")
    o, e = pair(sc, minImageNum=2, seed=5)
    assert e.grid_dims(0) == o.grid_dims(0) == (8, 6)
    c0 = e.propagate(0)
    assert all(c0[k] == 0 for k in COUNTERS), c0
    assert c0["inserted"] + c0["replaced"] == 0 and e.num_patches() == 0 and e.patches().shape[0] == 0
    seeds = synth.make_seeds(sc, stride=1, seed=5)
    assert seeds.shape[0] > 0
    o.add_patches(seeds)
    e.upload_patches(seeds)
    co, ce = o.propagate(0), e.propagate(0)
    print("seeds", seeds.shape[0], "oracle", co, "engine", ce)
    assert set(COUNTERS) <= set(co) and co == ce, (co, ce)
    pools_match_oracle(o.patches(), e.patches())
    o.close()
    e.close()


# ------------------------------------------------------------------ 3. a cell that gives up is followed by a clean cell
def test_cell_that_gives_up_is_followed_by_clean_cells(small_plane_scene):
    """The dense cells of test_gpu_parity.py::test_check_second_tier_dense_cells on two resident waves: the wave that meets an
    Optim::check too large for its LDS id set hands the cell to the second tier and goes on with later cells, whose results must
    not carry anything of the abandoned cell (its counts, its live list, its staged records)."""
    sc = small_plane_scene
    pool = dense_pool(sc, per_cell=30, window=5)
    o, e = pair(sc, seed=4, enable_check=1, minImageNum=2, max_propag=8)
    o.add_patches(pool)
    e.upload_patches(pool)
    o.update_threshold()
    e.update_threshold()  # m_depth 2: Optim::check runs
    co = o.propagate(1)
    with sweep_grid(2):
        ce = e.propagate(1)
        t = e.timing()
    print("oracle", co, "engine", ce, "retried cells", t["check_retried_cells"])
    assert t["check_retried_cells"] > 0, t
    assert set(COUNTERS) <= set(co) and co == ce, (co, ce)
    po, pe = o.patches(), e.patches()
    pools_match_oracle(po, pe)
    assert (pe["coord"] == po["coord"]).all(axis=1).mean() > 0.99
    o.close()
    e.close()


# ------------------------------------------------------------------ 4. views of unequal size
def test_views_of_unequal_size_on_three_waves():
    """Three views cropped to three sizes (test_gpu_ragged_shapes.py's per-view `sizes`): job_base differs per view (64 x 43, 61 x 40
    and 64 x 42 cells: 1376, 1240 and 1344 jobs) and is no multiple of 128, so chunks 10 and 20 of the 31 straddle two views -- the
    emptiness test maps every lane's job to its own view.  Three waves: queues 3-7 have none of their own.  One iteration equal to
    the oracle's."""
    sizes = [(128, 86), (121, 80), (128, 83)]
    sc = synth.make_scene(nviews=3, W=128, H=88, arc_deg=30.0, radius=4.0, kind="multi")
    o, e = pair_sized(sc, sizes=sizes, level=0, csize=2, wsize=7, minImageNum=2, seed=7)
    grids = [e.grid_dims(v) for v in range(3)]
    assert grids == [o.grid_dims(v) for v in range(3)] == [grid_of(w, h, 0, 2) for w, h in sizes]
    bases = np.cumsum([0] + [((gw + 1) // 2) * gh for gw, gh in grids])
    assert len(set(grids)) == 3 and list(bases) == [0, 1376, 2616, 3960] and all(b % 128 for b in bases[1:])
    seeds = seeds_for_sizes(sc, synth.make_seeds(sc, level=0, csize=2, stride=2, seed=5), sizes, 0)
    assert seeds.shape[0] > 300
    o.add_patches(seeds)
    co = o.propagate(0)
    with sweep_grid(3):
        e.upload_patches(seeds)
        ce = e.propagate(0)
    print("oracle", co, "engine", ce)
    assert set(COUNTERS) <= set(co) and co == ce, (co, ce)
    assert co["inserted"] > 500
    po, pe = o.patches(), e.patches()
    pools_match_oracle(po, pe)
    assert len(set(np.unique(po["images"][:, 0]))) == 3  # every view is the reference view of some patch
    o.close()
    e.close()
