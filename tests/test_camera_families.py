"""The CPU oracle against the second reading on cameras off the arc (camera_scenes.py): rolled, with fx != fy, skew, an off-centre
principal point and per-view focal and distance, and in a world hundreds of units from the origin.  The checks are those of
tests/test_oracle_second_reading.py that involve a camera (reading_checks.py), 4 views of 160 x 120, kind `multi`, SUM_SEQ,
make_seeds(stride=9, seed=4).

Tolerances.  `roll` and `intrinsics` take the arc's unchanged, but for the patch axes' relative tolerance on `intrinsics`
(test_units_and_axes).  `far` (T = (300, -150, 500), kappa 173) misses eight of them unscaled and takes those eight times kappa:
the projection, the patch axes, the sampled texture (88 times its arc tolerance) and its normalised form, incc (21 times), the
cost (4.3), m_dscale / m_ascale (19) and the incc matrix (5.9); reading_checks.py says for each why kappa applies.  What holds
unscaled on `far` stays unscaled: unproject, the round trip, encode, decode, generate_patch, the unit, ipscale, the camera's axes.
`mixed` (T = (12, -8, 16), kappa 8.65) was to take the arc's tolerances too; two of them do not hold there, and only those two take
kappa: the patch axes, 1.14e-4 relative against 2e-5, a common factor on the three components of an axis, and get_tex, 4.1e-3
against an atol of 2e-3.  Both are the world's offset, not the intrinsics: the axes' length is a unit step over the distance of two
float32 projections one pixel apart, each of which rounds relative to |P[:, :3]| |X| + |P[:, 3]|, kappa times what it is on the arc
(arc kappa 1.4, worst 1.5e-5: times 8.65 / 1.4 gives 9e-5, as seen), and a texture sample moves with its position times the image
gradient, the position again a float32 projection (arc worst 1.2e-3: 7e-3 expected, 4.1e-3 seen).  Every other check on `mixed` runs
at the arc's tolerance (projection 0.76 of it, incc 0.65, scales and incc matrix 0.42, normalised texture 0.40, cost 0.25).

All three restatements (setup_camera, oracle/pmmvs_oracle.cpp, second_reading.RefCam) read the same matrices, so on the `intrinsics`
family ipscale is also held to fx + fy of the K the cameras were built from."""
import numpy as np
import pytest

import camera_scenes as cs
import reading_checks as rc

#: the quantities of reading_checks.py whose tolerance takes kappa, per family (none on `roll` and `intrinsics`)
SCALED = {"far": rc.PIXEL_QUANTITIES, "mixed": ("axes", "tex")}
#: the families whose patch axes take the derived relative tolerance instead of the arc's 2e-5 (test_units_and_axes)
DERIVED_AXES_RTOL = ("intrinsics", "mixed")


@pytest.fixture(scope="module", params=cs.FAMILIES)
def family(request):
    sc = cs.family_scene(request.param, 4, 160, 120, 45.0, "multi")
    k = {q: cs.kappa(sc) for q in SCALED.get(request.param, ())}
    print(f"{request.param}: kappa {cs.kappa(sc):.2f}, tolerances times kappa: {sorted(k) or 'none'}")
    setup = rc.make_setup(sc)
    yield setup, k, request.param
    setup[1].close()


def test_camera(family):
    rc.check_camera(*family[:2])


def test_units_and_axes(family):
    """The arc's 2e-5 on the patch axes does not hold on `intrinsics`: 2.28e-5, the same factor on all three components of one axis
    (the arc reaches 1.5e-5 on the same seeds, `roll` 1.47e-5).  An error common to the components is one of the axis' length, the
    one-pixel distance it is divided by, not a disagreement of the readings about its direction: reading_checks.FAMILY_AXES_RTOL,
    3.05e-5, is derived from the spacing of a float32 pixel coordinate in check_units_and_axes' docstring.  It is taken where 2e-5
    fails, on `intrinsics` and on `mixed`, which has the same intrinsics; `roll` and `far` keep 2e-5."""
    setup, k, name = family
    rc.check_units_and_axes(setup, k, axes_rtol=rc.FAMILY_AXES_RTOL if name in DERIVED_AXES_RTOL else 2e-5)


def test_texture_and_incc(family):
    rc.check_texture_and_incc(*family[:2])


def test_encode_decode_and_cost(family):
    rc.check_encode_decode_and_cost(*family[:2])


def test_scales_and_neighbours(family):
    rc.check_scales_and_neighbours(*family[:2])


def test_generate_patch(family):
    rc.check_generate_patch(*family[:2])


def test_set_inccs_matrix(family):
    rc.check_set_inccs_matrix(*family[:2])


def test_ipscale_is_fx_plus_fy():
    """Optim::setAxesScales (optim.cpp:43-65): ipscale = P_row0 . xaxis + P_row1 . yaxis.  With P = K [R | t] and rows r0, r1, r2 of R,
    yaxis = r2 x P_row0 normalised = (fx r1 - s r0) / n and xaxis = (fx r0 + s r1) / n with the skew s and n = sqrt(fx^2 + s^2), so
    ipscale = n + fx fy / n: fx + fy without skew, and with s = 0.02 fx, fy = 1.07 fx it is (fx + fy) (1 - 6.8e-6).  Held to fx + fy of
    the K the family was built from within 1e-5 relative, and more than 1 % away from 2 fx and 2 fy: a row mix-up or a doubled row in
    all three restatements at once would show here (an oracle with ipscale = 2 P_row0 . xaxis passes every test on the arc and fails
    this one by 3.4 %)."""
    sc = cs.family_scene("intrinsics", 4, 160, 120, 45.0, "multi")
    setup = rc.make_setup(sc)
    o, cams = setup[1], setup[2]
    for v in range(sc.nviews):
        fx, fy = sc.meta["K"][v, 0, 0], sc.meta["K"][v, 1, 1]
        for what, got in (("oracle", o.camera(v)["ipscale"]), ("second reading", cams[v].ipscale)):
            print(f"view {v} {what}: ipscale {got:.6f}, fx + fy {fx + fy:.6f}, off by {abs(got - (fx + fy)) / (fx + fy):.2e} of it")
            assert abs(got - (fx + fy)) <= 1e-5 * (fx + fy), (what, v, got, fx + fy)
            assert abs(got - 2 * fx) > 0.01 * (fx + fy) and abs(got - 2 * fy) > 0.01 * (fx + fy), (what, v, got, fx, fy)
    o.close()
