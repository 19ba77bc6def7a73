"""The scenes of tests/edge_scenes.py do what they claim -- shown with the CPU oracle and the second reading alone, no GPU.

Coverage: every class of the patchwork scene has its 200 seeds whose windows lie wholly inside it in all listed views; the
mixed-scale scene drives Optim::getTex's level pick (optim.cpp:799-811) through -1 (at working level 1), 0, +1, +2 and both clamps,
each with windows the oracle accepts and, for the unclamped values, windows it rejects while the reference view's own passes.

What the flat classes really are.  The reference blends four texels with float32 weights f00 .. f11 that are rounded products
(image.cpp:452-470); their sum is not 1, so the blend of four texels of value 200 is 200 +- a few ulp, not 200.  A window of class
(a) therefore has ssd ~ 1e-9, msd ~ 5e-6 and 1 / msd ~ 2e5, and its NCC is rounding noise of the blend amplified to order 0.1: it
differs from seed to seed (measured: -0.22 .. 0.27 over 160 seeds), in the reference as in the oracle.  Only where every sample
falls on a half-pixel (weights exactly 1/4: the reference view of a seed at a cell centre) or where the texels are 0 is the window
exactly constant.  So class (a) is asserted as what it is -- constant texels, samples within 8 ulp of 200, a finite NCC, windows
with msd ~ 5e-6 among them -- and the bit-equal NCC is asserted on class (a0), value 0, where it is a theorem.

The bound of the second reading (test_float32_second_reading_bound): the oracle in its engine summation order (ORC_SUM_TREE64)
against ref_compute_incc / ref_cost_func, on 600 seeds of each well-conditioned class and on ALL mixed-scale seeds of both working
levels (10571 and 10548 pairs; one seed each lies within 1e-3 of a level threshold and is left out).  The reading itself is recorded
in tests/golden/edge_second_reading.npz (tests/golden/make_edge_reading.py: minutes of numpy) and a 40th of it is recomputed here.
Measured worst absolute deviations: WORST_MEASURED of tests/edge_scenes.py; the worst of all is 5.59e-5, a plain INCC of class (b) (5.22e-5 on the
mixed-scale scene at level 0).  That is above the bound of tests/test_oracle_second_reading.py, 5e-5 * max(1, |expected|) (6.4e-6
measured there on textured seeds), so the bound for these inputs is four times the measured worst, 2.24e-4 * max(1, |expected|):
SECOND_READING_BOUND.  tests/test_gpu_photometric_edges.py holds the device to the same bound on the same seeds."""
import numpy as np
import pytest

import edge_scenes as es
from edge_scenes import (GOLDEN, GROUPS, compute_reading, group_name, group_seeds, level_counts, level_table, oracle_for, second_reading, windows,
                         within_bound)

F = np.float32
U = 2.0 ** -24


# ------------------------------------------------------------------ the patchwork scene
def test_patchwork_regions_and_seed_counts():
    sc, classes, seeds, k = es.patchwork()
    for c in range(1, 8):
        for v in range(sc.nviews):
            m = classes[v] == c
            wide = m.sum(axis=1).max()
            high = m.sum(axis=0).max()
            assert wide >= 40 and high >= 40, (es.CLASS_NAMES[c], v, wide, high)
    counts = {es.CLASS_NAMES[c]: int((k == c).sum()) for c in range(8)}
    print("patchwork seeds per class", counts)
    assert min(counts.values()) >= 200, counts
    # (f): the flat view is the reference view of a share of the seeds and a non-reference view of the others
    f = seeds[k == es.FLAT_ONE_VIEW]
    assert (f["images"][:, 0] == es.FLAT_VIEW).sum() >= 50 and (f["images"][:, 0] != es.FLAT_VIEW).sum() >= 150
    # the images really hold what the classes say
    for v in range(sc.nviews):
        img = sc.images[v]
        assert (img[classes[v] == es.CONST] == 200).all() and (img[classes[v] == es.BLACK] == 0).all()
        sat = img[classes[v] == es.SATURATED]
        assert set(np.unique(sat)) == {0, 255} and 0.3 < (sat == 255).mean() < 0.7
        red = img[classes[v] == es.RED_ONLY]
        assert (red[:, 1:] == 90).all() and red[:, 0].std() > 20
        flat = img[classes[v] == es.FLAT_ONE_VIEW]
        assert (flat == 150).all() if v == es.FLAT_VIEW else flat.std() > 20
        ramp = img[classes[v] == es.RAMP]
        assert (ramp[:, 0] == ramp[:, 1]).all() and 4 <= len(np.unique(ramp)) <= 9


def test_flat_windows_through_the_oracle():
    """(a): texels constant, samples 200 within 8 ulp (four weights of two roundings each, a sum of four terms rounded four times),
    NCC finite; windows that are constant only to rounding occur (those that are exactly constant are counted and printed).  (a0): samples exactly 0 in every view, NCC finite and
    bit-equal across the class.  (d): the median msd of a window lies in (0, 0.5)."""
    sc, _, _, _ = es.patchwork()
    o = oracle_for(sc)
    exact = tiny = 0
    for s in es.class_seeds(es.CONST, 200):
        for v, flag, tex in windows(o, s):
            assert flag == 0
            assert np.abs(tex - 200.0).max() <= 200.0 * 8 * U, (v, np.abs(tex - 200.0).max())
            if (tex == tex[0, 0]).all():
                exact += 1
            else:
                tiny += 1
        assert np.isfinite(o.compute_ncc(s))
    print("class a windows: exactly constant", exact, "constant to rounding", tiny)
    assert tiny >= 1  # the msd ~ 5e-6 arm; the msd == 0 arm is class a0's, below, in every window
    nccs = []
    for s in es.class_seeds(es.BLACK, 200):
        for v, flag, tex in windows(o, s):
            assert flag == 0 and not tex.any()
        nccs.append(o.compute_ncc(s))
    nccs = np.array(nccs, F)
    assert np.isfinite(nccs).all() and (nccs.view(np.uint32) == nccs.view(np.uint32)[0]).all(), np.unique(nccs)
    msd = []
    for s in es.class_seeds(es.RAMP, 200):
        for v, flag, tex in windows(o, s):
            assert flag == 0
            t = tex.astype(np.float64)
            msd.append(np.sqrt(((t - t.mean(axis=0)) ** 2).sum() / (3 * t.shape[0])))
    print("class d msd: median", np.median(msd), "min", min(msd), "max", max(msd))
    assert 0.0 < np.median(msd) < 0.5
    o.close()


# ------------------------------------------------------------------ the level pick on the mixed-scale scene
@pytest.mark.parametrize("level", [0, 1])
def test_level_coverage(level):
    seeds, tab, flags = level_table(level)
    counts = level_counts(tab, level)
    print("level", level, "pairs", tab.shape[0], "(accepted, rejected beside an accepted reference view):", counts,
          "preProcess accepts", int((flags == 0).sum()), "rejects", int((flags != 0).sum()))
    for name, (acc, rej) in counts.items():
        assert acc >= 30, (level, name, acc)
        if "clamp" not in name:
            assert rej >= 10, (level, name, rej)
    assert (flags == 0).sum() >= 200 and (flags != 0).sum() >= 200
    refs = np.bincount(np.asarray(es.MIXED_SCALES)[seeds["images"][:, 0]], minlength=4)
    assert refs.min() >= 200, refs  # every scale is the reference view of its share


# ------------------------------------------------------------------ the bound of the second reading
@pytest.mark.parametrize("group", GROUPS, ids=group_name)
def test_float32_second_reading_bound(group):
    """The oracle against the recorded reading over the whole group; every 40th seed's reading is computed again here and must be
    the recorded one to 2e-6 (numpy's float32 products may round otherwise on another CPU; the deviations measured are ten times
    that), so the file is the reading of these seeds; the oracle's side is always computed now."""
    _, _, _, seeds = group_seeds(group)
    with np.load(GOLDEN) as z:
        incc, cost = z[group_name(group) + "/incc"], z[group_name(group) + "/cost"]
    assert incc.shape[0] == seeds.shape[0], "tests/golden/make_edge_reading.py has to be run again"
    which = np.arange(0, seeds.shape[0], 40)
    live = compute_reading(group, which)
    np.testing.assert_allclose(live["incc"], incc[which], rtol=0, atol=2e-6)  # equal_nan: the same seeds are left out
    np.testing.assert_allclose(live["cost"], cost[which], rtol=0, atol=2e-6)
    sc, level, sizes, _ = group_seeds(group)
    o = oracle_for(sc, level, sizes)
    used, kept = ~np.isnan(incc[:, 0]), ~np.isnan(cost)
    got = np.array([[o.compute_incc(s, robust=r) for r in (0, 1)] for s in seeds[used]])
    r = second_reading(group)
    gotc = np.array([o.cost(rec, o.encode(rec)) for rec in r["recs"]])
    o.close()
    ok0, w0 = within_bound(got[:, 0], incc[used, 0])
    ok1, w1 = within_bound(got[:, 1], incc[used, 1])
    ok2, w2 = within_bound(gotc, cost[kept])
    pairs = int((seeds["nimages"] - 1).sum())
    skipped = int((seeds["nimages"] - 1)[~used].sum())  # an upper bound: every pair of a seed that is left out
    print(f"second reading, {group_name(group)}: {seeds.shape[0]} seeds, {pairs} pairs, {skipped} left out near a level threshold, "
          f"{int(kept.sum())} costs, worst |oracle - reading| incc {w0:.3g} robust {w1:.3g} cost {w2:.3g}")
    assert pairs >= 1000 and skipped <= 0.01 * pairs, (pairs, skipped)
    assert kept.sum() >= 300
    assert ok0 and ok1 and ok2, (w0, w1, w2)
