"""The sweep kernels read their launch parameters -- DParams, SweepArgs, the refiner's two numbers -- from the launch's own
kernel-argument segment, stage by stage ("launch parameters").  What that can break is a parameter read from the
wrong place or from a stale one: another engine's, or the previous launch's.  Every case here makes consecutive launches differ in
their parameters and compares with runs in which nothing else was ever launched:

  1. two engines alive at once, with different window, csize, level, thresholds and seed, their passes interleaved;
  2. one engine whose parameters change from launch to launch: (a) the three-iteration schedule against the CPU oracle (thresholds
     and m_depth move, Optim::check switches on), (b) the refiner toggled between launches against engines that never ran another
     refiner, (c) the launcher's switches flipped between launches against the default run, bit for bit;
  3. the ranges of a three-way split of the jobs, one after the other (job_lo > 0), against the unsplit pass.

Small scenes throughout: 3 views of 64 x 48 pixels (32 x 24 cells), seeds in every cell, max_propag 2 -- lists fill, pairs form, full-cell
trials occur and Optim::check rejects."""
import os
from contextlib import contextmanager

import pytest

import oracle_binding as ob
from mvskit_amd import engine, synth
from parity_support import COUNTERS, REMOVALS, pools_match_oracle

pytestmark = pytest.mark.gpu

KW = dict(level=0, csize=2, wsize=7, minImageNum=2, seed=11, enable_check=1, max_propag=2)
ITERATIONS = 3
SWITCHES = ("MVS_SWEEP_PAIR", "MVS_SWEEP_FULLWINDOW", "MVS_SAMPLER_WIDE")


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


def _default_switches():
    return _environment(**dict.fromkeys(SWITCHES))


@pytest.fixture(scope="module")
def scene():
    sc = synth.make_scene(nviews=3, W=64, H=48, arc_deg=30.0, radius=4.0, kind="multi")
    return sc, synth.make_seeds(sc, stride=1, seed=5)


def _pass(e, it, p):
    c = e.engine_pass(it, p)
    e.commit_local()
    return c


def _between_iterations(x, it, removed):
    if it + 1 < ITERATIONS:
        r = x.filter()
        removed.append([r[k] for k in REMOVALS])
        x.update_threshold()


def _state(e):
    return e.patches(), e.sweep_pairs(), e.sweep_repeats(), e.sweep_kernels(), e.sampler_launches(), e.thresholds()


# ------------------------------------------------------------------ 1. two engines alive at once
def _engine_a(scene):
    sc, seeds = scene
    e = engine.Engine(sc.nviews, **KW)
    e.set_scene(sc)
    e.upload_patches(seeds)
    return e


def _engine_b():
    """everything a launch reads differs from engine A: a 5 x 5 window (the generic kernel), csize 3, level 1, thresholds, seed"""
    sc = synth.make_scene(nviews=3, W=144, H=108, arc_deg=24.0, radius=4.0, kind="multi")
    seeds = synth.make_seeds(sc, level=1, csize=3, stride=1, seed=9)
    # (a pool of 2^16 records: the default, four per cell, does not hold a seed in every cell plus what an iteration adds at csize 3)
    e = engine.Engine(sc.nviews, level=1, csize=3, wsize=5, minImageNum=2, seed=4, enable_check=1, max_propag=3, max_patches=1 << 16)
    e.set_scene(sc)
    e.set_thresholds(0.6, 0.4, 1)
    e.upload_patches(seeds)
    return e


def _steps(e):
    """the schedule of _plan pass by pass, as a generator: one step is one sweep launch and its commit"""
    counters, removed = [], []
    for it in range(ITERATIONS):
        for p in range(2):
            counters.append(_pass(e, it, p))
            yield None
        _between_iterations(e, it, removed)
    yield counters, removed


def _drain(*gens):
    """steps of the generators in turn (a, b, a, b, ...); -> the last value of each"""
    last = [None] * len(gens)
    live = list(range(len(gens)))
    while live:
        for k in list(live):
            try:
                last[k] = next(gens[k])
            except StopIteration:
                live.remove(k)
    return last


def test_two_engines_with_different_parameters_interleaved(scene):
    with _default_switches():
        alone = []
        for make in (lambda: _engine_a(scene), _engine_b):
            e = make()
            (res,) = _drain(_steps(e))
            alone.append((res, _state(e)))
            e.close()
        a, b = _engine_a(scene), _engine_b()
        both = _drain(_steps(a), _steps(b))
        for k, e in enumerate((a, b)):
            res, st = alone[k]
            got = _state(e)
            print("engine", "AB"[k], "counters", both[k][0], "kernels", got[3], "samplers", got[4], "thresholds", got[5])
            assert both[k] == res, (k, both[k], res)
            assert got[1:] == st[1:], (k, got[1:], st[1:])
            assert got[0].shape == st[0].shape and got[0].shape[0] > 1000
            assert got[0].tobytes() == st[0].tobytes()
            tot = {c: sum(x[c] for x in res[0]) for c in COUNTERS}
            assert tot["inserted"] > 0 and tot["replaced"] > 0, tot
            if k == 0:
                assert tot["fail1"] > 0, tot  # Optim::check ran and rejected
            e.close()
        # the two engines ran different kernels on different parameters
        assert alone[0][1][3]["full_window"] == 2 * ITERATIONS and alone[1][1][3]["generic"] == 2 * ITERATIONS
        assert alone[0][1][5] != alone[1][1][5]


# ------------------------------------------------------------------ 2a. the schedule against the oracle
def test_schedule_moves_thresholds_and_depth_like_the_oracle(scene):
    sc, seeds = scene
    o = ob.Oracle(sc.nviews, schedule=ob.SCHEDULE_ENGINE, sum_mode=ob.SUM_TREE64, nthreads=8, **KW)
    o.set_scene(sc)
    o.add_patches(seeds)
    oc, orem = [], []
    for it in range(ITERATIONS):
        oc.append(o.propagate(it))
        _between_iterations(o, it, orem)
    with _default_switches():
        e = _engine_a(scene)
        seen = [e.thresholds()]
        (res,) = _drain(_steps(e))
        ec, erem = res
        seen.append(e.thresholds())
        pe, kernels = e.patches(), e.sweep_kernels()
        e.close()
    print("oracle", oc, "engine", ec, "thresholds", seen)
    assert seen[0][2] == 1 and seen[1][2] == 3 and seen[0][:2] != seen[1][:2], seen  # m_depth 1, 2, 3 and both thresholds moved
    for it in range(ITERATIONS):
        for k in COUNTERS:
            assert oc[it][k] == ec[2 * it][k] + ec[2 * it + 1][k], (it, k, oc[it], ec[2 * it], ec[2 * it + 1])
    assert orem == erem
    assert sum(c["fail1"] for c in oc[1:]) > 0 and sum(c["replaced"] for c in oc) > 0
    assert kernels == {"generic": 0, "full_window": 2 * ITERATIONS}, kernels
    pools_match_oracle(o.patches(), pe)
    o.close()


# ------------------------------------------------------------------ 2b. the refiner toggled between launches
REFINERS = (dict(mode="halving"), dict(mode="converged", max_evals=40, xtol=1e-3), dict(mode="halving"),
            dict(mode="converged", max_evals=500, xtol=1e-4), dict(mode="converged", max_evals=40, xtol=1e-3))


def _one_launch(e, seeds, refiner):
    """the same launch every time -- iteration 1, colour 1 on the seeds, with Optim::check -- under `refiner`"""
    e.clear_patches()
    e.set_refiner(**refiner)
    e.upload_patches(seeds)
    c = _pass(e, 1, 1)
    return c, e.patches()


def _check_engine(sc):
    e = engine.Engine(sc.nviews, **KW)
    e.set_scene(sc)
    a, b, _ = e.thresholds()
    e.set_thresholds(a, b, 2)  # m_depth 2: Optim::check runs
    return e


def test_refiner_toggled_between_launches_equals_fresh_engines(scene):
    sc, seeds = scene
    with _default_switches():
        t = _check_engine(sc)
        toggled = [_one_launch(t, seeds, r) for r in REFINERS]
        kernels = t.sweep_kernels()
        t.close()
        assert kernels == {"generic": 3, "full_window": 2}, kernels  # the CONVERGED refiner's kernel counts as generic
        for k, r in enumerate(REFINERS):
            f = _check_engine(sc)  # never ran another refiner
            c, p = _one_launch(f, seeds, r)
            f.close()
            print(r, c)
            assert c == toggled[k][0], (k, r, c, toggled[k][0])
            assert p.tobytes() == toggled[k][1].tobytes(), (k, r)
            assert c["inserted"] > 0 and c["fail1"] > 0, c
    # the toggles matter: the three refiners give three results
    assert len({toggled[k][1].tobytes() for k in (0, 1, 3)}) == 3
    assert toggled[0][1].tobytes() == toggled[2][1].tobytes() and toggled[1][1].tobytes() == toggled[4][1].tobytes()


# ------------------------------------------------------------------ 2c. the launcher's switches flipped between launches
FLIPS = (dict(MVS_SWEEP_PAIR=0, MVS_SWEEP_FULLWINDOW=0), dict(MVS_SAMPLER_WIDE=1), {}, dict(MVS_SWEEP_FULLWINDOW=0),
         dict(MVS_SWEEP_PAIR=0, MVS_SAMPLER_WIDE=1), {})


def _flipped_run(scene, flips):
    e = _engine_a(scene)
    counters, removed = [], []
    for it in range(ITERATIONS):
        for p in range(2):
            with _environment(**{**dict.fromkeys(SWITCHES), **flips[2 * it + p]}):
                counters.append(_pass(e, it, p))
        _between_iterations(e, it, removed)
    out = counters, removed, e.patches(), e.sweep_kernels(), e.sampler_launches(), e.sweep_pairs()
    e.close()
    return out


def test_switches_flipped_between_launches_equal_the_default_run(scene):
    d = _flipped_run(scene, ({},) * 6)
    f = _flipped_run(scene, FLIPS)
    print("default", d[3], d[4], d[5], "flipped", f[3], f[4], f[5])
    assert d[3] == {"generic": 0, "full_window": 6} and d[4]["sweep_narrow"] == 6 and d[4]["sweep_wide"] == 0, (d[3], d[4])
    # every row of the launcher's table for the default refiner ran: generic, full window with wide samplers, full window with narrow ones
    assert f[3] == {"generic": 2, "full_window": 4}, f[3]
    assert f[4]["sweep_wide"] == 4 and f[4]["sweep_narrow"] == 2, f[4]
    assert 0 < f[5]["paired"] < d[5]["paired"] and f[5]["can_pair"] == d[5]["can_pair"], (d[5], f[5])
    assert f[0] == d[0] and f[1] == d[1]
    assert f[2].shape == d[2].shape and f[2].shape[0] > 1000
    assert f[2].tobytes() == d[2].tobytes()


# ------------------------------------------------------------------ 3. job ranges that do not start at 0
def test_ranges_of_a_split_one_after_the_other_equal_the_unsplit_pass(scene):
    """three engines, each with one range of the jobs (work-balanced cuts: the second and third start behind 0), run each pass one
    after the other on one device; their exports merged in view order and committed to all three give the unsplit engine's pool"""
    import torch

    from mvskit_amd.dist import merge_in_view_order

    sc, seeds = scene
    world = 3
    dev = torch.device("cuda", 0)
    with _default_switches():
        whole = _engine_a(scene)
        parts = []
        for r in range(world):
            h = engine.Engine(sc.nviews, shard_index=r, shard_count=world, **KW)
            h.set_scene(sc)
            h.upload_patches(seeds)
            parts.append(h)
        for it in range(2):
            for p in range(2):
                cw = _pass(whole, it, p)
                total = dict.fromkeys(COUNTERS, 0)
                recs, kills, counts = [], [], []
                for h in parts:
                    c = h.engine_pass(it, p)
                    for k in COUNTERS:
                        total[k] += c[k]
                    n_new, n_kill, per_view = h.export_counts()
                    rec = torch.zeros(max(n_new, 1), 128, dtype=torch.uint8, device=dev)
                    kil = torch.full((max(n_kill, 1),), -1, dtype=torch.int32, device=dev)
                    torch.cuda.synchronize(dev)
                    h.export_device(rec.data_ptr(), rec.shape[0], kil.data_ptr(), kil.shape[0])
                    recs.append(rec[:n_new]); kills.append(kil[:n_kill]); counts.append(per_view)
                merged = merge_in_view_order(recs, counts, sc.nviews, world)
                allrec = torch.cat(merged).contiguous() if merged else torch.zeros(0, 128, dtype=torch.uint8, device=dev)
                allkill = torch.cat(kills).contiguous()
                torch.cuda.synchronize(dev)
                for h in parts:
                    h.commit_device(allrec.data_ptr(), allrec.shape[0], allkill.data_ptr(), allkill.shape[0])
                print("iteration", it, "colour", p, "whole", cw, "ranges", total, "new per range", [int(r.shape[0]) for r in recs])
                for k in COUNTERS:
                    if k == "trimmed":  # every range builds, and trims, the whole index
                        continue
                    if k in ("evals", "view_evals"):
                        # ... and scores the records whose m_ncc is negative (every seed before the first pass, a few records later) itself:
                        # the sweep's evaluations once, that scoring once per range
                        extra = total[k] - cw[k]
                        assert extra >= 0 and extra % (world - 1) == 0 and extra // (world - 1) < cw[k] // 10, (it, p, k, total, cw)
                        if (it, p) == (0, 0):
                            assert extra > 0, (k, total, cw)
                        continue
                    assert total[k] == cw[k], (it, p, k, total, cw)
                if cw["inserted"] > 0:
                    assert sum(1 for r in recs if r.shape[0] > 0) >= 2, "the split left all the work to one range"
            whole.update_threshold()
            for h in parts:
                h.update_threshold()
        pw = whole.patches()
        assert pw.shape[0] > seeds.shape[0]
        for h in parts:
            assert h.patches().tobytes() == pw.tobytes()
            h.close()
        whole.close()
