"""The engine against the oracle on cameras off the arc (camera_scenes.py): two iterations of propagate / filter / updateThreshold with
Optim::check on, through parity_support.loop_two_iterations with its assertions as they are -- equal counters and removals, REL_TOL, more
than 99 % of the coordinates bit-equal -- on 4 views of 160 x 120 `multi`, make_seeds(stride=4).

What the arc never showed the sweep: footprints turned by 90, 180 and 37 degrees, also in a portrait image (`roll`); ipscale, the unit
and the SeedCam-style per-view tables differing by view, fx != fy, skew, an off-centre principal point (`intrinsics`); every float32
rounding of a projection amplified 170-fold at T = (300, -150, 500) (`far`); and all of it together at (12, -8, 16) (`mixed`), on which
the converged refiner also runs through the probe against its restatement."""
import pytest

import camera_scenes as cs
from mvskit_amd import synth
from parity_support import loop_two_iterations, pair, probe_vs_restatement

pytestmark = pytest.mark.gpu


def _loop(sc, what):
    o, e = pair(sc, minImageNum=3, enable_check=1, seed=11)
    loop_two_iterations(o, e, sc, synth.make_seeds(sc, stride=4), None, what)
    e.close()
    o.close()


@pytest.mark.parametrize("family", cs.FAMILIES)
def test_two_iterations(family):
    _loop(cs.family_scene(family, 4, 160, 120, 45.0, "multi"), family)


def test_two_iterations_roll_portrait():
    """98 x 130: the view turned by 90 degrees sees the scene's width along its short side"""
    _loop(cs.portrait_roll_scene(4, 45.0, "multi"), "roll, portrait")


def test_converged_refiner_on_mixed():
    """set_refiner("converged", max_evals=200, xtol=1e-3) through PROBE_REFINE / PROBE_REFINE_X on the `mixed` family against
    refiner_restatement.py on the oracle's cost_func, as tests/test_refiner_converged.py does on the arc.  With 200 evaluations the
    restatement itself converges on 57 % of these candidates (median 189 evaluations): the share that converges is held to the
    restatement's, not to the 90 % that the budget of 500 reaches."""
    probe_vs_restatement(cs.family_scene("mixed", 4, 160, 120, 45.0, "multi"), 3, 0, max_evals=200, xtol=1e-3)
