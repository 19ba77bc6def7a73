"""GPU parity tests: the HIP engine, called through the C ABI, against the CPU oracle on the same inputs.

The oracle runs in TREE64 summation mode (the wavefront butterfly order) so results are expected to be
bit-identical; every comparison also states the north-star tolerance (1e-3 relative depth, 1e-3 rad normal)."""
import numpy as np
import pytest

import oracle_binding as ob
from mvskit_amd import engine, synth
from parity_support import REL_TOL, cmp_records, dense_pool, maps_close, pair

pytestmark = pytest.mark.gpu


def test_math_probe_bit_exact(small_plane_scene):
    o, e = pair(small_plane_scene, minImageNum=2)
    x = np.concatenate([np.linspace(-1.5707, 1.5707, 4001), np.linspace(-1, 1, 2001), np.linspace(-30, 30, 1001)]).astype(np.float32)
    got = e.probe(engine.PROBE_MATH, values=x)
    L = ob.lib()
    exp = np.array([[L.orc_sinf(float(v)), L.orc_cosf(float(v)), L.orc_asinf(float(v)), L.orc_acosf(float(v)), L.orc_atanf(float(v))]
                    for v in x], dtype=np.float32)
    dom = np.abs(x) <= 1.5708
    np.testing.assert_array_equal(got[dom, 0], exp[dom, 0])
    np.testing.assert_array_equal(got[dom, 1], exp[dom, 1])
    unit = np.abs(x) <= 1.0
    np.testing.assert_array_equal(got[unit, 2], exp[unit, 2])
    np.testing.assert_array_equal(got[unit, 3], exp[unit, 3])
    np.testing.assert_array_equal(got[:, 4], exp[:, 4])


def test_pyramid_bit_exact(small_multi_scene):
    o, e = pair(small_multi_scene)
    for v in (0, 3):
        for level in range(3):
            np.testing.assert_array_equal(e.pyramid(v, level), o.pyramid(v, level))
    assert e.grid_dims(1) == o.grid_dims(1)


def test_ncc_batch(small_multi_scene):
    o, e = pair(small_multi_scene)
    seeds = synth.make_seeds(small_multi_scene, stride=6)
    assert seeds.shape[0] > 300
    _, got, _ = e.probe(engine.PROBE_NCC, seeds)
    exp = np.array([o.compute_ncc(s) for s in seeds], dtype=np.float32)
    assert np.isfinite(exp).all()
    np.testing.assert_allclose(got, exp, rtol=REL_TOL, atol=1e-5)
    assert (got == exp).mean() > 0.999, f"bit-exact fraction {(got == exp).mean()}"


def test_pre_refine_post_chain(small_multi_scene):
    o, e = pair(small_multi_scene)
    seeds = synth.make_seeds(small_multi_scene, stride=8, seed=31)[:200]
    pre_rec, _, pre_flag = e.probe(engine.PROBE_PREPROCESS, seeds)
    keep = []
    exact = 0
    for i, s in enumerate(seeds):
        f, r = o.preprocess(s)
        assert f == pre_flag[i], i
        if f == 0:
            cmp_records(pre_rec[i], r, f"pre {i}")
            keep.append(i)
    assert len(keep) > 50
    sub = pre_rec[keep]
    ref_rec, _, _ = e.probe(engine.PROBE_REFINE, sub)
    _, cost, _ = e.probe(engine.PROBE_COST, sub)
    post_in = []
    for j, i in enumerate(keep):
        x = o.encode(sub[j])
        assert abs(cost[j] - o.cost(sub[j], x)) <= 1e-6
        _, r = o.refine(sub[j], (0, 0, j, 0))
        cmp_records(ref_rec[j], r, f"refine {j}")
        exact += int(ref_rec[j]["coord"].tobytes() == r["coord"].tobytes() and ref_rec[j]["normal"].tobytes() == r["normal"].tobytes())
        post_in.append(r)
    assert exact >= 0.98 * len(keep), f"refine bit-exact {exact}/{len(keep)}"
    post_in = np.array(post_in, dtype=ob.PATCH_DTYPE)
    o.add_patches(seeds)
    e.upload_patches(seeds)
    post_rec, _, post_flag = e.probe(engine.PROBE_POSTPROCESS, post_in)
    npass = 0
    for j in range(post_in.shape[0]):
        f, r = o.postprocess(post_in[j])
        assert f == post_flag[j], j
        if f == 0:
            cmp_records(post_rec[j], r, f"post {j}")
            assert post_rec[j]["nvimages"] == r["nvimages"]
            npass += 1
    assert npass > 20


def test_propagate_two_iterations_matches_oracle(small_multi_scene):
    sc = small_multi_scene
    o, e = pair(sc, seed=7)
    seeds = synth.make_seeds(sc, stride=4, seed=5)
    o.add_patches(seeds)
    e.upload_patches(seeds)
    for it in range(2):
        co = o.propagate(it)
        ce = e.propagate(it)
        assert ce["patches"] > 1000
        for k in ("candidates", "prefiltered", "patches", "fail0", "fail1", "inserted", "replaced", "evals", "view_evals", "trimmed"):
            assert co[k] == ce[k], (it, k, co, ce)
        po, pe = o.patches(), e.patches()
        assert po.shape == pe.shape
        np.testing.assert_array_equal(po["nimages"], pe["nimages"])
        np.testing.assert_array_equal(po["images"], pe["images"])
        np.testing.assert_allclose(pe["coord"], po["coord"], rtol=REL_TOL, atol=1e-6)
        np.testing.assert_allclose(pe["normal"], po["normal"], rtol=0, atol=REL_TOL)
        np.testing.assert_allclose(pe["ncc"], po["ncc"], rtol=REL_TOL, atol=1e-6)
        assert (po["coord"].view(np.uint32) == pe["coord"].view(np.uint32)).all(axis=1).mean() > 0.999
    tot, bad = maps_close(o, e, sc.nviews)
    assert tot > 2000 and bad == 0


def test_check_stage_probe(small_multi_scene):
    """Optim::check (optim.cpp:300-323: computeGain, findNeighbors, filterQuad) through postProcess at m_depth = 2."""
    sc = small_multi_scene
    o, e = pair(sc, seed=11, enable_check=1)
    seeds = synth.make_seeds(sc, stride=2, seed=3)
    o.add_patches(seeds)
    e.upload_patches(seeds)
    co, ce = o.propagate(0), e.propagate(0)  # populate the grids (depth 1: no check yet)
    assert co["patches"] == ce["patches"]
    o.update_threshold()
    e.update_threshold()
    assert o.thresholds()[2] == 2 and e.thresholds()[2] == 2
    cand = o.patches()[::7][:400]
    post_rec, _, post_flag = e.probe(engine.PROBE_POSTPROCESS, cand)
    rejected = passed = 0
    for j in range(cand.shape[0]):
        f, r = o.postprocess(cand[j])
        assert f == post_flag[j], j
        if f == 0:
            cmp_records(post_rec[j], r, f"post+check {j}")
            np.testing.assert_allclose(post_rec[j]["tmp"], r["tmp"], rtol=REL_TOL, atol=1e-5)  # m_tmp = gain
            passed += 1
        else:
            rejected += 1
    assert passed > 50


def test_three_iterations_with_check(small_multi_scene):
    """PmMvps::run's loop (pmmvps.cpp:90-110) without Filter::run: m_depth 1, 2, 3 -- Optim::check active from iteration 1."""
    sc = small_multi_scene
    o, e = pair(sc, seed=13, enable_check=1)
    seeds = synth.make_seeds(sc, stride=4, seed=17)
    o.add_patches(seeds)
    e.upload_patches(seeds)
    for it in range(3):
        co, ce = o.propagate(it), e.propagate(it)
        for k in ("candidates", "prefiltered", "patches", "fail0", "fail1", "inserted", "replaced", "evals", "view_evals", "trimmed"):
            assert co[k] == ce[k], (it, k, co, ce)
        o.update_threshold()
        e.update_threshold()
    po, pe = o.patches(), e.patches()
    assert po.shape == pe.shape
    np.testing.assert_array_equal(po["images"], pe["images"])
    np.testing.assert_array_equal(po["vimages"], pe["vimages"])
    np.testing.assert_allclose(pe["coord"], po["coord"], rtol=REL_TOL, atol=1e-6)
    np.testing.assert_allclose(pe["normal"], po["normal"], rtol=0, atol=REL_TOL)
    np.testing.assert_allclose(pe["tmp"], po["tmp"], rtol=REL_TOL, atol=1e-5)
    tot, bad = maps_close(o, e, sc.nviews)
    assert tot > 2000 and bad == 0


def test_engine_rccl_exchange_world1_equals_local_commit(small_multi_scene):
    """The in-engine multi-GPU path of the C ABI (mvs_comm_unique_id / mvs_engine_comm_init / mvs_engine_exchange inside
    mvs_engine_propagate: RCCL count all-gather, in-place broadcast of the record and kill-id blocks behind the pool, commit
    of the union) with a communicator of one rank must give exactly the pool the local commit gives, Optim::check included."""
    sc = small_multi_scene
    seeds = synth.make_seeds(sc, stride=4, seed=23)
    kw = dict(level=0, csize=2, wsize=7, minImageNum=3, enable_check=1, seed=5)
    a = engine.Engine(sc.nviews, **kw)
    b = engine.Engine(sc.nviews, shard_index=0, shard_count=1, **kw)
    for e in (a, b):
        e.set_scene(sc)
        e.upload_patches(seeds)
    b.comm_init(b.comm_unique_id(), 0, 1)
    moved = 0
    for it in range(3):
        ca = a.propagate(it)
        cb = b.propagate(it)
        assert ca == cb, (it, ca, cb)
        t = b.timing()
        assert t["exchange_ms"] > 0.0 and t["exchange_bytes"] == 0  # one rank: nothing comes from elsewhere
        moved += cb["inserted"] + cb["replaced"]
        a.update_threshold()
        b.update_threshold()
    assert moved > 1000
    pa, pb = a.patches(), b.patches()
    assert pa.shape == pb.shape
    assert pa.tobytes() == pb.tobytes()
    # pass / exchange can also be driven one colour pass at a time
    c0 = b.engine_pass(3, 0)
    b.exchange()
    assert c0["patches"] > 0
    b.comm_release()
    with pytest.raises(engine.EngineError):
        b.engine_pass(3, 1)
        b.exchange()  # no communicator any more
    b.commit_local()
    a.close()
    b.close()


def _one_iteration_matches(sc, seeds, masks=None, **kw):
    o, e = pair(sc, **kw)
    if masks is not None:
        o.set_scene(sc, masks=masks)
        e.set_scene(sc, masks=masks)
    o.add_patches(seeds)
    e.upload_patches(seeds)
    co, ce = o.propagate(0), e.propagate(0)
    assert co == ce, (co, ce)
    po, pe = o.patches(), e.patches()
    assert po.shape == pe.shape
    np.testing.assert_array_equal(po["images"], pe["images"])
    np.testing.assert_allclose(pe["coord"], po["coord"], rtol=REL_TOL, atol=1e-6)
    np.testing.assert_allclose(pe["normal"], po["normal"], rtol=0, atol=REL_TOL)
    return co


def test_variant_level1(small_multi_scene):
    # Option::m_level = 1 (the reference's default, option.cpp:20): grids and projections one pyramid level down
    seeds = synth.make_seeds(small_multi_scene, level=1, stride=3, seed=2)
    c = _one_iteration_matches(small_multi_scene, seeds, level=1, seed=3)
    assert c["patches"] > 300


def test_variant_wsize5_csize1(small_plane_scene):
    # 5x5 windows (25 sample lanes) and csize 1 (MAX_NUM_OF_PATCHES = 2)
    seeds = synth.make_seeds(small_plane_scene, csize=1, stride=6, seed=4)
    c = _one_iteration_matches(small_plane_scene, seeds, minImageNum=2, wsize=5, csize=1, seed=9)
    assert c["patches"] > 300


@pytest.mark.parametrize("wsize", [6, 4, 3, 2])
def test_variant_window_sizes(small_plane_scene, wsize):
    """Every window size the class-lane layout deals differently: 36 = two full slots + a partly filled third, 16 = one slot,
    9 and 4 = one partly filled slot (7x7 = three slots + the extra sample and 5x5 = two slots are covered above)."""
    seeds = synth.make_seeds(small_plane_scene, stride=4, seed=14)
    c = _one_iteration_matches(small_plane_scene, seeds, minImageNum=2, wsize=wsize, seed=6)
    assert c["patches"] > 300


def test_variant_csize3(small_plane_scene):
    seeds = synth.make_seeds(small_plane_scene, csize=3, stride=2, seed=6)
    c = _one_iteration_matches(small_plane_scene, seeds, minImageNum=2, csize=3, seed=1)
    assert c["patches"] > 300


def test_variant_masks(small_plane_scene):
    # PhotoSet::getMask (photoSet.cpp:223-233): a patch that projects onto a zero mask pixel of any view is dropped
    sc = small_plane_scene
    masks = np.full((sc.nviews, sc.H, sc.W), 255, np.uint8)
    masks[:, :, : sc.W // 3] = 0
    masks[1, sc.H // 2:, :] = 90  # < 128: binarised to 0 (image.cpp:170-177)
    seeds = synth.make_seeds(sc, stride=4, seed=8)
    c = _one_iteration_matches(sc, seeds, masks=masks, minImageNum=2, seed=2)
    assert c["fail1"] > 50 and c["inserted"] > 50


def test_two_view_config(small_plane_scene):
    # BASELINE.json configs[0]: 2 views, minImageNum 2, one PatchMatch iteration
    sc = synth.Scene(W=small_plane_scene.W, H=small_plane_scene.H, P=small_plane_scene.P[[0, 2]], images=small_plane_scene.images[[0, 2]],
                     centers=small_plane_scene.centers[[0, 2]], points=small_plane_scene.points[[0, 2]], normals=small_plane_scene.normals[[0, 2]],
                     meta=small_plane_scene.meta)
    seeds = synth.make_seeds(sc, stride=4, seed=12)
    c = _one_iteration_matches(sc, seeds, minImageNum=2, seed=4)
    assert c["patches"] > 300 and c["inserted"] > 100


@pytest.mark.parametrize("min_image_num", [5, 8])
def test_variant_min_image_num(min_image_num):
    """m_minImageNum 5 and 8 (the engine's limit): tau = 10 and 16 views per cost evaluation -- three and four passes of the
    single evaluations, ten and sixteen frame lanes per proposal in the refinement steps -- on a 16-view scene whose views all
    see the plane."""
    sc = synth.make_scene(nviews=16, W=128, H=96, arc_deg=40.0, radius=4.0, kind="plane")
    seeds = synth.make_seeds(sc, stride=5, seed=23, views=range(0, 16, 3))
    c = _one_iteration_matches(sc, seeds, minImageNum=min_image_num, seed=8)
    assert c["patches"] > 200 and c["inserted"] > 50


@pytest.mark.parametrize("list_cap", [64, 32, 16])
def test_variant_48_views(list_cap):
    # BASELINE.json configs[3] has 48 views.  list_cap 64 = libmvskit_engine_cap64.so, what engine.Engine picks for more than 32
    # views: no list is cut, as in the reference (optim.cpp:165-205 pushes every qualifying view).  32 / 16 = the smaller builds
    # forced onto the same scene: more views than their records store or their lists keep, so addImages / sortImages / the
    # per-view lanes run past both limits; the oracle truncates alike.
    sc = synth.make_scene(nviews=48, W=96, H=72, arc_deg=141.0, radius=4.0, kind="plane")
    seeds = synth.make_seeds(sc, stride=6, seed=31, views=range(0, 48, 5))
    c = _one_iteration_matches(sc, seeds, seed=6, list_cap=list_cap)
    assert c["patches"] > 200 and c["inserted"] > 50


@pytest.mark.parametrize("list_cap,nviews", [(32, 20), (64, 40)])
def test_many_view_libraries_two_iterations_with_check_and_filter(list_cap, nviews):
    """libmvskit_engine_cap32.so (32-view lists: twice the setRefImage LDS, eight rounds of pair lanes, two patches per wave
    in filterExact) on a 20-view scene and libmvskit_engine_cap64.so (64-view lists, 192-byte records, one view per lane, one
    patch per wave in filterExact) on a 40-view scene, through the whole loop of PmMvps::run: counters, lists, maps and the four
    Filter::run removal counts equal to the oracle's with the same cap."""
    sc = synth.make_scene(nviews=nviews, W=160, H=120, arc_deg=120.0, radius=4.0, kind="multi")
    seeds = synth.make_seeds(sc, stride=4 if nviews <= 20 else 6, seed=3)
    o, e = pair(sc, seed=9, enable_check=1, list_cap=list_cap)
    assert e.list_cap == list_cap and e.dtype.itemsize == (192 if list_cap == 64 else 128)
    o.add_patches(seeds)
    e.upload_patches(seeds)
    longest = 0
    for it in range(2):
        co, ce = o.propagate(it), e.propagate(it)
        for k in ("candidates", "prefiltered", "patches", "fail0", "fail1", "inserted", "replaced", "evals", "view_evals", "trimmed"):
            assert co[k] == ce[k], (it, k, co, ce)
        fo, fe = o.filter(), e.filter()
        assert fo == fe, (it, fo, fe)
        o.update_threshold()
        e.update_threshold()
    po, pe = o.patches(), e.patches()
    assert po.shape == pe.shape and pe.shape[0] > seeds.shape[0]
    longest = int(pe["nimages"].max())
    assert longest > list_cap // 2  # lists beyond the next smaller cap are really in play
    np.testing.assert_array_equal(po["images"], pe["images"])
    np.testing.assert_array_equal(po["vimages"], pe["vimages"])
    np.testing.assert_allclose(pe["coord"], po["coord"], rtol=REL_TOL, atol=1e-6)
    tot, bad = maps_close(o, e, sc.nviews)
    # 20 overlapping views put several patches of nearly the same depth into a cell: where two of them lie within the
    # coordinate tolerance of each other the nearest one may differ (5 of 107 490 cells when this was written)
    assert tot > 2000 and bad <= tot * 1e-4, (tot, bad)


def test_view_propagation_matches_oracle(small_multi_scene):
    """the view-propagation branch the reference keeps commented out (propagate.cpp:110-120, design in
    trash/propagate_view_propagation_simiar_to_original.cpp:95-147), as an option of the engine schedule."""
    sc = small_multi_scene
    seeds = synth.make_seeds(sc, stride=4, seed=23, views=[0, sc.nviews // 2])
    o, e = pair(sc, seed=5, view_propagation=1)
    o0, _ = pair(sc, seed=5)
    for x in (o, e, o0):
        (x.add_patches if hasattr(x, "add_patches") else x.upload_patches)(seeds)
    for it in range(2):
        co, ce = o.propagate(it), e.propagate(it)
        assert co == ce, (it, co, ce)
        c0 = o0.propagate(it)
    assert co["patches"] > 1.3 * c0["patches"]  # patches of other views proposing themselves: more candidates per pass
    po, pe = o.patches(), e.patches()
    assert po.shape == pe.shape
    np.testing.assert_array_equal(po["images"], pe["images"])
    np.testing.assert_allclose(pe["coord"], po["coord"], rtol=REL_TOL, atol=1e-6)
    np.testing.assert_allclose(pe["normal"], po["normal"], rtol=0, atol=REL_TOL)


def test_empty_pool_and_reupload(small_plane_scene):
    o, e = pair(small_plane_scene, minImageNum=2)
    assert e.propagate(0)["patches"] == 0 and e.num_patches() == 0
    seeds = synth.make_seeds(small_plane_scene, stride=8, seed=1)
    ragged = seeds.copy()
    ragged["nimages"][::5] = 0          # records without images are dropped (patch_manager.cpp:457-459)
    e.upload_patches(ragged)
    assert e.num_patches() == int((ragged["nimages"] > 0).sum())
    e.clear_patches()
    assert e.num_patches() == 0


def test_filter_run_matches_oracle(small_multi_scene):
    """Filter::run (filter.cpp:25-49) after each Propagate::run, as PmMvps::run does (pmmvps.cpp:95-105)."""
    sc = small_multi_scene
    o, e = pair(sc, seed=21, enable_check=1)
    seeds = synth.make_seeds(sc, stride=3, seed=19)
    o.add_patches(seeds)
    e.upload_patches(seeds)
    for it in range(2):
        co, ce = o.propagate(it), e.propagate(it)
        assert co == ce, (it, co, ce)
        fo, fe = o.filter(), e.filter()
        assert fo == fe, (it, fo, fe)
        assert fo["outside"] + fo["exact"] > 0
        po, pe = o.patches(), e.patches()
        assert po.shape == pe.shape
        np.testing.assert_array_equal(po["images"], pe["images"])      # filterExact rewrites m_images and the reference view
        np.testing.assert_array_equal(po["nvimages"], pe["nvimages"])  # setDepthMapsVGridsVPGridsAddPatchV rebuilds m_vimages
        np.testing.assert_array_equal(po["vimages"], pe["vimages"])
        np.testing.assert_allclose(pe["coord"], po["coord"], rtol=REL_TOL, atol=1e-6)
        o.update_threshold()
        e.update_threshold()
    # Filter::run once more on the filtered pool: the engine does not recompute setRefImage for a patch whose list already is the
    # outcome of filterExact for its set of views and which keeps them all (DPatch flag bit 1); the oracle recomputes every patch
    # as the reference does (filter.cpp:148-209) -- lists and reference views must still agree
    evals_before = e.filter_stats()["exact_view_evals"]
    fo, fe = o.filter(), e.filter()
    assert fo == fe, (fo, fe)
    st = e.filter_stats()
    assert st["exact_view_evals"] < evals_before // 10, (st, evals_before)
    po, pe = o.patches(), e.patches()
    np.testing.assert_array_equal(po["images"], pe["images"])
    np.testing.assert_array_equal(po["vimages"], pe["vimages"])


def test_filter_packed_geometry_gives_what_the_records_give(small_multi_scene, monkeypatch):
    """Inside Filter::run the stages read the patches they meet from a 32-byte packed copy (DParams::geo, mvs_engine_filter.cpp pack_geometry)
    instead of the records.  The fault-injection build can switch the copy off (MVS_FAULT_NOPACK): both ways the same removals and the
    same pool, byte for byte, as the oracle's.  A pool with a seed whose coord.w is not 1 cannot be packed (the copy leaves w out): the
    engine must notice and read the records."""
    from mvskit_amd import build
    sc = small_multi_scene
    monkeypatch.setenv("MVS_ENGINE_LIB", build.FAULT_LIB_PATH)
    seeds = synth.make_seeds(sc, stride=3, seed=19)
    odd = seeds.copy()
    odd["coord"][::7, 3] = 1.0009765625  # homogeneous coordinates the reference would take as they are
    for variant, sd in (("packed", seeds), ("records", seeds), ("odd w", odd)):
        monkeypatch.setenv("MVS_FAULT_NOPACK", "1" if variant == "records" else "0")
        o, e = pair(sc, seed=21, enable_check=1)
        o.add_patches(sd)
        e.upload_patches(sd)
        for it in range(2):
            co, ce = o.propagate(it), e.propagate(it)
            assert co == ce, (variant, it, co, ce)
            fo, fe = o.filter(), e.filter()
            assert fo == fe, (variant, it, fo, fe)
            po, pe = o.patches(), e.patches()
            np.testing.assert_array_equal(po["images"], pe["images"])
            np.testing.assert_array_equal(po["vimages"], pe["vimages"])
            np.testing.assert_allclose(pe["coord"], po["coord"], rtol=REL_TOL, atol=1e-6)
            o.update_threshold()
            e.update_threshold()
        assert fo["neighbor"] + fo["outside"] > 0
        o.close()
        e.close()


def test_reserve_sizes_the_indexes_up_front(small_multi_scene):
    """mvs_engine_reserve: the cell indexes allocated once (default: MAX_NUM_OF_PATCHES entries per cell) -- the iterations that
    follow compute what they compute without it (two iterations with Optim::check and Filter::run against the oracle), a smaller
    request later changes nothing, a larger one between two calls replaces the buffers without harm, a negative one is refused."""
    sc = small_multi_scene
    seeds = synth.make_seeds(sc, stride=3, seed=19)
    o, e = pair(sc, seed=21, enable_check=1)
    e.reserve()
    o.add_patches(seeds)
    e.upload_patches(seeds)
    for it in range(2):
        co, ce = o.propagate(it), e.propagate(it)
        assert co == ce, (it, co, ce)
        e.reserve(1000)
        if it == 0:
            e.reserve(40_000_000)  # larger than what the indexes hold: the buffers are replaced (and written once), the lists in them are gone -- the calls that follow must rebuild them
        fo, fe = o.filter(), e.filter()
        assert fo == fe, (it, fo, fe)
        o.update_threshold()
        e.update_threshold()
    with pytest.raises(engine.EngineError):
        e.reserve(-1)
    o.close()
    e.close()


def test_min_image_num_above_eight():
    """Option::m_minImageNum 9 on a 12-view set: tau = min(2 minImageNum, nviews) = 12 views of a proposal still sit in the 16
    frame lanes (pmmvps.cpp:32; the engine's limit is on tau, not on minImageNum).  Two iterations with Optim::check and
    Filter::run on a narrow arc, where every view sees the surface: counters, lists and survivors equal the oracle's."""
    sc = synth.make_scene(nviews=12, W=160, H=120, arc_deg=22.0, radius=4.0, kind="multi")
    seeds = synth.make_seeds(sc, stride=4, seed=11)
    o, e = pair(sc, seed=13, enable_check=1, minImageNum=9)
    o.add_patches(seeds)
    e.upload_patches(seeds)
    for it in range(2):
        co, ce = o.propagate(it), e.propagate(it)
        assert co == ce, (it, co, ce)
        fo, fe = o.filter(), e.filter()
        assert fo == fe, (it, fo, fe)
        o.update_threshold()
        e.update_threshold()
    po, pe = o.patches(), e.patches()
    assert po.shape == pe.shape and pe.shape[0] > seeds.shape[0] // 4
    assert int(pe["nimages"].min()) >= 9
    np.testing.assert_array_equal(po["images"], pe["images"])
    np.testing.assert_array_equal(po["vimages"], pe["vimages"])
    np.testing.assert_allclose(pe["coord"], po["coord"], rtol=REL_TOL, atol=1e-6)
    with pytest.raises(engine.EngineError):
        engine.Engine(20, minImageNum=9)  # tau = 18 on a 20-view set: more than the frame lanes hold
    o.close()
    e.close()


@pytest.mark.parametrize("npatch", [0, 1, 3, 5, 63, 65, 130])
def test_filter_run_tiny_and_ragged_pools(small_plane_scene, npatch):
    """Filter::run on pools that do not fill a wave or a block of the per-patch kernels (four patches per wave in filterExact and
    setVImagesVGrids, 64 per block in the depth maps, four per block in filterSmallGroups' edge pass), down to the empty pool, and
    on pools a stage empties (a handful of patches has fewer than six neighbours each: filterNeighbor removes them all and
    filterSmallGroups meets nothing): the four removal counts and the survivors equal the oracle's."""
    sc = small_plane_scene
    seeds = synth.make_seeds(sc, stride=3, seed=41)[:npatch]
    o, e = pair(sc, seed=2, enable_check=1, minImageNum=2)
    if npatch:
        o.add_patches(seeds)
        e.upload_patches(seeds)
    for x in (o, e):
        x.update_threshold()  # m_depth 2: isVisible tests depths
    for _ in range(2):
        fo, fe = o.filter(), e.filter()
        assert fo == fe, (npatch, fo, fe)
        po, pe = o.patches(), e.patches()
        assert po.shape == pe.shape
        if po.shape[0]:
            np.testing.assert_array_equal(po["images"], pe["images"])
            np.testing.assert_array_equal(po["vimages"], pe["vimages"])
            np.testing.assert_array_equal(po["coord"], pe["coord"])
    o.close()
    e.close()


def test_filter_small_groups_literal_labelling():
    """mvs_config.literal_groups: Filter::filterSmallGroups with the reference's own breadth-first labelling in patch order over the
    directed relation (filter.cpp:432-524) instead of the connected components.  The GPU finds the sets joined by two-way edges and the
    one-way edges left between them, the host walks those few sets in the order of their first patches; the oracle runs the literal
    search patch by patch.  Same scene as tests/test_oracle_kat.py::test_small_groups_components_vs_literal_labelling, where the two
    labellings remove different patches: removal counts and surviving patches equal the literal oracle's in all three Filter::run
    calls, and differ from the default mode's at least once."""
    sc = synth.make_scene(nviews=5, W=256, H=160, arc_deg=60.0, radius=4.0, kind="multi")
    seeds = synth.make_seeds(sc, stride=3, seed=19)
    o, e = pair(sc, seed=21, enable_check=1, literal_groups=1)
    o1, _ = pair(sc, seed=21, enable_check=1)
    for x in (o, e, o1):
        (x.add_patches if x is not e else x.upload_patches)(seeds)
    differs = 0
    for it in range(3):
        co, ce = o.propagate(it), e.propagate(it)
        assert co == ce, (it, co, ce)
        o1.propagate(it)
        fo, fe, f1 = o.filter(), e.filter(), o1.filter()
        assert fo == fe, (it, fo, fe)
        differs += fo["groups"] != f1["groups"]
        po, pe = o.patches(), e.patches()
        assert po.shape == pe.shape
        np.testing.assert_array_equal(po["images"], pe["images"])
        np.testing.assert_allclose(pe["coord"], po["coord"], rtol=REL_TOL, atol=1e-6)
        for x in (o, e, o1):
            x.update_threshold()
    assert differs > 0
    for x in (o, e, o1):
        x.close()


def test_filter_neighbor_dense_cells_take_the_retry_launch(small_plane_scene):
    """Filter::filterNeighbor on cells that hold 30 patches each: a patch meets ~750 others in its 5x5 cells, more neighbours than the
    first launch's row buffer holds (576), so it goes to the second launch (16384-slot id set, 64 KB of LDS) -- the path the
    reference's unbounded findNeighbors (patch_manager.cpp:671-728) needs and no other test reaches.  Removal counts, lists and the
    surviving patches equal the oracle's, whose table-size rule is the same."""
    sc = small_plane_scene
    pool = dense_pool(sc, per_cell=30)
    assert pool.shape[0] > 4000
    o, e = pair(sc, seed=3, enable_check=1, minImageNum=2)
    o.add_patches(pool)
    e.upload_patches(pool)
    o.update_threshold()
    e.update_threshold()  # m_depth 2: isVisible tests depths
    fo, fe = o.filter(), e.filter()
    st = e.filter_stats()
    assert st["neighbor_retried"] > 1000, st
    assert fo == fe, (fo, fe)
    po, pe = o.patches(), e.patches()
    assert po.shape == pe.shape and pe.shape[0] > 1000
    np.testing.assert_array_equal(po["images"], pe["images"])
    np.testing.assert_array_equal(po["vimages"], pe["vimages"])
    np.testing.assert_array_equal(po["coord"], pe["coord"])
    o.close()
    e.close()


def test_check_second_tier_dense_cells(small_plane_scene):
    """Optim::check inside the sweep with neighbourhoods that do not fit a wave's LDS: cells that hold 30 patches (MAX_NUM_OF_PATCHES =
    max_propag * csize^2 = 32 here, so the trim leaves them alone) give a candidate ~750 neighbours in its 5x5 cells, more than the
    576 rows of the first tier.  Such destination cells give up in k_sweep and run again in k_sweep_retry with a 16384-slot id
    set in global memory; the reference's findNeighbors is unbounded (patch_manager.cpp:671-728) and the oracle's table-size rule
    is the same.  Counters, lists and coordinates equal the oracle's."""
    sc = small_plane_scene
    pool = dense_pool(sc, per_cell=30, window=5)
    o, e = pair(sc, seed=4, enable_check=1, minImageNum=2, max_propag=8)
    o.add_patches(pool)
    e.upload_patches(pool)
    o.update_threshold()
    e.update_threshold()  # m_depth 2: Optim::check runs
    co, ce = o.propagate(1), e.propagate(1)
    t = e.timing()
    assert t["check_retried_cells"] >= 5, t
    assert co == ce, (co, ce)
    assert co["patches"] > 1000 and co["replaced"] > 100
    po, pe = o.patches(), e.patches()
    assert po.shape == pe.shape
    np.testing.assert_array_equal(po["images"], pe["images"])
    np.testing.assert_array_equal(po["vimages"], pe["vimages"])
    np.testing.assert_allclose(pe["coord"], po["coord"], rtol=REL_TOL, atol=1e-6)
    assert (pe["coord"] == po["coord"]).all(axis=1).mean() > 0.99
    o.close()
    e.close()


RANDOM_CASES = [  # (nviews, W, H, arc, kind, level, csize, wsize, minImageNum, masks, view_propagation, stride, max_propag)
    (3, 200, 150, 25.0, "plane", 0, 2, 7, 2, False, 0, 4, 2),
    (4, 224, 160, 40.0, "multi", 0, 1, 5, 2, True, 0, 6, 2),
    (5, 256, 176, 55.0, "multi", 1, 2, 7, 3, False, 1, 3, 2),
    (6, 192, 144, 70.0, "multi", 0, 3, 3, 3, True, 0, 2, 1),
    (7, 160, 112, 60.0, "plane", 0, 2, 6, 4, False, 1, 6, 2),
    (8, 144, 104, 80.0, "multi", 0, 2, 7, 3, False, 0, 6, 3),
    (9, 176, 128, 65.0, "multi", 1, 1, 5, 4, True, 0, 3, 2),
    (10, 160, 120, 75.0, "multi", 0, 2, 4, 5, False, 0, 3, 2),
]


@pytest.mark.parametrize("case", range(len(RANDOM_CASES)))
def test_mixed_configurations(case):
    """A sweep over the configuration space -- views, image size, arc, pyramid level, cell size, window size, m_minImageNum, masks,
    view propagation, seed density, MAX_NUM_OF_PROPAG -- each through two or three iterations of PmMvps::run's loop with Optim::check and
    Filter::run: counters, lists and the removal counts equal to the oracle's, coordinates within the north-star tolerance."""
    nv, W, H, arc, kind, level, csize, wsize, mi, use_masks, vprop, stride, maxp = RANDOM_CASES[case]
    sc = synth.make_scene(nviews=nv, W=W, H=H, arc_deg=arc, radius=4.0, kind=kind)
    seeds = synth.make_seeds(sc, level=level, csize=csize, stride=stride, seed=100 + case)
    masks = None
    if use_masks:
        masks = np.full((nv, H, W), 255, np.uint8)
        masks[:, : H // 6, :] = 0
        masks[case % nv, :, : W // 5] = 60
    o, e = pair(sc, level=level, csize=csize, wsize=wsize, minImageNum=mi, seed=40 + case, enable_check=1, view_propagation=vprop, max_propag=maxp)
    if masks is not None:
        o.set_scene(sc, masks=masks)
        e.set_scene(sc, masks=masks)
    o.add_patches(seeds)
    e.upload_patches(seeds)
    total = 0
    for it in range(3 if case < 4 else 2):  # the larger cases stop after the first iteration with Optim::check (the oracle is the slow side)
        co, ce = o.propagate(it), e.propagate(it)
        assert co == ce, (case, it, co, ce)
        total += co["patches"]
        ro, re_ = o.filter(), e.filter()
        assert [ro[k] for k in ("outside", "exact", "neighbor", "groups")] == [re_[k] for k in ("outside", "exact", "neighbor", "groups")], (case, it, ro, re_)
        o.update_threshold()
        e.update_threshold()
    assert total > 200, total
    po, pe = o.patches(), e.patches()
    assert po.shape == pe.shape and po.shape[0] > 0
    np.testing.assert_array_equal(po["images"], pe["images"])
    np.testing.assert_array_equal(po["vimages"], pe["vimages"])
    np.testing.assert_allclose(pe["coord"], po["coord"], rtol=REL_TOL, atol=1e-6)
    np.testing.assert_allclose(pe["normal"], po["normal"], rtol=0, atol=REL_TOL)
