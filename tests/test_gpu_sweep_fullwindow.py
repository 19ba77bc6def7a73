"""A window whose samples fill all three slots of every class lane and leave one extra (3 x 16 + 1 samples: wsize 7) runs the sweep on
an instantiation of its kernel without the slot-mask arithmetic (k_sweep_full); every other window, and a full one
under MVS_SWEEP_FULLWINDOW=0 (read on every launch), runs the generic kernel.  Leaving out a factor 1.0f must not change a bit of the
result: every case compares the HIP engine with the CPU oracle (ENGINE schedule), the pool as parity_support.pools_match_oracle does
and all ten counters of every iteration for equality, and the full-window kernel's pool with the generic kernel's byte for byte.

All cases run test_gpu_sweep_repeats.py's scene -- seeds in every cell of 3 views of 64 x 48 `multi`, three iterations at max_propag 2
with Optim::check: lists fill, pairs form and full-cell trials occur.  mvs_engine_sweep_kernels (Engine.sweep_kernels) says which kernel
the launcher chose; every case asserts it, so that none passes on the other kernel."""
import os
from contextlib import contextmanager

import pytest

import oracle_binding as ob
from mvskit_amd import engine, synth
from parity_support import COUNTERS, REMOVALS, pools_match_oracle, sweep_grid

pytestmark = pytest.mark.gpu

KW = dict(level=0, csize=2, minImageNum=2, seed=11, enable_check=1, max_propag=2)
ITERATIONS = 3
LAUNCHES = 2 * ITERATIONS  # a propagate is two colour passes, a sweep launch each


@contextmanager
def _environment(**values):
    """the given variables around the engine calls of the block (None: unset), restored afterwards"""
    old = {k: os.environ.pop(k, None) for k in values}
    for k, v in values.items():
        if v is not None:
            os.environ[k] = str(v)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _plan(x):
    """Propagate::run three times, with Filter::run and updateThreshold in between (m_depth 2 from the second: Optim::check)"""
    counters, removed = [], []
    for it in range(ITERATIONS):
        counters.append(x.propagate(it))
        if it + 1 < ITERATIONS:
            r = x.filter()
            removed.append([r[k] for k in REMOVALS])
            x.update_threshold()
    return counters, removed


def _engine_run(sc, pool, wsize, full=None, pair=None, grid=None):
    """-> (counters, removals, pool, sweep_kernels, sweep_pairs) of a fresh engine; full / pair: MVS_SWEEP_FULLWINDOW / MVS_SWEEP_PAIR"""
    e = engine.Engine(sc.nviews, wsize=wsize, **KW)
    e.set_scene(sc)
    with _environment(MVS_SWEEP_FULLWINDOW=full, MVS_SWEEP_PAIR=pair), sweep_grid(grid):
        e.upload_patches(pool)
        c, r = _plan(e)
        p = e.patches()
        k = e.sweep_kernels()
        s = e.sweep_pairs()
    e.close()
    assert set(k) == set(engine.Engine.SWEEP_KERNEL_KEYS), k
    return c, r, p, k, s


def _oracle_run(sc, pool, wsize):
    o = ob.Oracle(sc.nviews, wsize=wsize, schedule=ob.SCHEDULE_ENGINE, sum_mode=ob.SUM_TREE64, nthreads=8, **KW)
    o.set_scene(sc)
    o.add_patches(pool)
    c, r = _plan(o)
    p = o.patches()
    o.close()
    return c, r, p


def _matches_oracle(oracle, eng):
    oc, orem, po = oracle
    c, r, p = eng[:3]
    print("oracle", oc)
    print("engine", c)
    print("kernels", eng[3], "pairs", eng[4])
    assert len(oc) == len(c) == ITERATIONS
    for it in range(ITERATIONS):
        assert set(COUNTERS) <= set(oc[it]) and len(COUNTERS) == 10
        for k in COUNTERS:
            assert oc[it][k] == c[it][k], (it, k, oc[it], c[it])
    assert orem == r
    pools_match_oracle(po, p)
    # the scene does what it is here for: lists fill (replace-worst trials) and Optim::check rejects
    tot = {k: sum(x[k] for x in oc) for k in COUNTERS}
    assert tot["replaced"] > 0 and tot["prefiltered"] > 0 and tot["inserted"] > 0 and tot["fail1"] > 0, tot


@pytest.fixture(scope="module")
def scene():
    sc = synth.make_scene(nviews=3, W=64, H=48, arc_deg=30.0, radius=4.0, kind="multi")
    return sc, synth.make_seeds(sc, stride=1, seed=5)


@pytest.fixture(scope="module")
def oracle7(scene):
    """the oracle at wsize 7, computed once and left unchanged"""
    return _oracle_run(*scene, 7)


@pytest.fixture(scope="module")
def generic7(scene):
    """the engine at wsize 7 on the generic kernel (MVS_SWEEP_FULLWINDOW=0), computed once and left unchanged"""
    return _engine_run(*scene, 7, full=0)


def test_switch_forces_the_generic_kernel(oracle7, generic7):
    assert generic7[3] == {"generic": LAUNCHES, "full_window": 0}, generic7[3]
    _matches_oracle(oracle7, generic7)


def test_wsize7_runs_the_full_window_kernel(scene, oracle7, generic7):
    eng = _engine_run(*scene, 7)
    assert eng[3] == {"generic": 0, "full_window": LAUNCHES}, eng[3]
    assert eng[4]["paired"] > 0, eng[4]
    _matches_oracle(oracle7, eng)
    assert eng[0] == generic7[0] and eng[1] == generic7[1]
    assert eng[2].shape == generic7[2].shape and eng[2].tobytes() == generic7[2].tobytes()


def test_one_resident_wave(scene, oracle7, generic7):
    """MVS_SWEEP_GRID=1: one wave runs every cell, one after the other"""
    eng = _engine_run(*scene, 7, grid=1)
    assert eng[3] == {"generic": 0, "full_window": LAUNCHES}, eng[3]
    _matches_oracle(oracle7, eng)
    assert eng[2].tobytes() == generic7[2].tobytes()


def test_wsize5_runs_the_generic_kernel(scene):
    """25 samples leave slots empty (lanes 9..15 of the second slot, the whole third): the launcher must not pick the full-window kernel"""
    eng = _engine_run(*scene, 5)
    assert eng[3] == {"generic": LAUNCHES, "full_window": 0}, eng[3]
    _matches_oracle(_oracle_run(*scene, 5), eng)


def test_wsize7_without_pairing(scene, oracle7, generic7):
    """MVS_SWEEP_PAIR=0: every trial through the single-candidate step loop of the full-window kernel"""
    eng = _engine_run(*scene, 7, pair=0)
    assert eng[3] == {"generic": 0, "full_window": LAUNCHES}, eng[3]
    assert eng[4]["paired"] == 0 and eng[4]["can_pair"] > 0, eng[4]
    _matches_oracle(oracle7, eng)
    assert eng[2].tobytes() == generic7[2].tobytes()
