"""The shapes every other scene of the suite avoids: odd image sizes (pyramid levels that lose a column or a row), grids with an
odd width (the red-black job mapping has a job beyond the last cell in every other row), sizes csize does not divide (a narrower
last column and row of cells) and views of unequal size (per-view W, H, gw, gh and cell_base really differ) -- the HIP engine
against the CPU oracle, with the assertions of test_gpu_parity.py::test_mixed_configurations plus a floor on bit-equal coordinates.

Every case asserts its own raggedness from grid_dims / the pyramid shapes and its richness from the oracle's own numbers."""
import numpy as np
import pytest

from mvskit_amd import engine, synth
from parity_support import REL_TOL, cmp_records, grid_of, loop_two_iterations, pair, pair_sized, seeds_for_sizes
from ply_support import level_inputs, restate_ply
from second_reading import RefCam, ref_get_paxes, ref_project

pytestmark = pytest.mark.gpu
F = np.float32


# ------------------------------------------------------------------ 1. pyramids and grids
PYRAMID_SIZES = [(321, 243), (321, 244), (322, 243),  # (odd, odd), (odd, even), (even, odd)
                 (322, 246),                          # even, odd further down: 322 -> 161 -> 80, 246 -> 123 -> 61
                 (8, 8), (9, 9)]                      # the smallest size mvs_engine_set_views takes, and the next


@pytest.mark.parametrize("W,H", PYRAMID_SIZES)
def test_pyramids_and_grids_odd_sizes(W, H):
    """k_pyr_down on parents of odd width or height (the last output pixel's 2x + 2 tap is the parent's last column, which an even
    parent drops): every level that is built (level + 3), byte for byte against the oracle, whose odd levels
    tests/test_oracle_second_reading.py::test_pyramid_second_reading_odd_sizes checks against the numpy reading.  grid_dims for
    csize 1, 2, 3 against ceil((W >> level) / csize) (patch_manager.cpp:36-37)."""
    sc = synth.make_scene(nviews=2, W=W, H=H, arc_deg=20.0, radius=4.0, kind="plane", keep_geometry=False)
    level = 1
    for csize in (2, 1, 3):
        o, e = pair(sc, level=level, csize=csize, minImageNum=2)
        want = grid_of(W, H, level, csize)
        for v in range(2):
            assert e.grid_dims(v) == o.grid_dims(v) == want, (csize, v)
        if csize == 2:
            odd = 0
            for v in range(2):
                for l in range(level + 3):
                    pe, po = e.pyramid(v, l), o.pyramid(v, l)
                    assert pe.shape == po.shape == (H >> l, W >> l, 3), (v, l)
                    np.testing.assert_array_equal(pe, po, err_msg=f"view {v} level {l}")
                    odd += (l + 1 < level + 3) and ((W >> l) & 1 or (H >> l) & 1)
            assert odd > 0 or (W, H) == (8, 8)  # a parent level with an odd side: the case this test is for
        o.close()
        e.close()


@pytest.mark.parametrize("W,H", [(7, 16), (16, 7)])
def test_views_below_eight_pixels_are_refused(W, H):
    sc = synth.Scene(W=W, H=H, P=synth.make_cameras(2, W, H, 20.0, 4.0)[0], images=np.zeros((2, H, W, 3), np.uint8), centers=np.zeros((2, 3)))
    e = engine.Engine(2, level=0, minImageNum=2)
    with pytest.raises(engine.EngineError) as err:
        e.set_scene(sc)
    assert err.value.status == -1  # MVS_ERR_ARG
    with pytest.raises(engine.EngineError):
        e.propagate(0)  # no views: nothing runs
    e.close()


# ------------------------------------------------------------------ 2. masks below an odd level 0
def _one_iteration(sc, seeds, masks, **kw):
    o, e = pair_sized(sc, masks=masks, **kw)
    o.add_patches(seeds)
    e.upload_patches(seeds)
    co, ce = o.propagate(0), e.propagate(0)
    assert co == ce, (co, ce)
    po, pe = o.patches(), e.patches()
    assert po.shape == pe.shape and po.shape[0] > 0
    np.testing.assert_array_equal(po["nimages"], pe["nimages"])
    np.testing.assert_array_equal(po["images"], pe["images"])
    np.testing.assert_array_equal(po["nvimages"], pe["nvimages"])
    np.testing.assert_array_equal(po["vimages"], pe["vimages"])
    np.testing.assert_allclose(pe["coord"], po["coord"], rtol=REL_TOL, atol=1e-6)
    np.testing.assert_allclose(pe["normal"], po["normal"], rtol=0, atol=REL_TOL)
    o.close()
    e.close()
    return co, po


def test_masks_on_odd_sizes_at_level_one():
    """k_mask_down below a 203x151 level 0 (level 1: 101x75, 2 * 101 < 203 and 2 * 75 < 151).  The engine has no accessor for its
    mask pyramid, so it is read through Optim::postProcess' mask test (fail1).  (a) Masks whose only zeros are the last column and
    the last row of level 0: level 1 never reads them, the run equals the oracle's AND the run without masks.  Under the any-of-four
    rule one more zero tap clears nothing, so (a) alone would not notice a kernel that does read them; (c) is its complement, masks
    that are zero everywhere EXCEPT that column and row: a kernel that read them would set level-1 pixels, a correct one has an
    all-zero level 1 and every candidate fails the mask test -- nothing is inserted.  (b) A zero band with
    odd edges (columns 23..33, across W // 7 = 29): level-1 column 11 reads (22, 23) and stays set under the any-of-four rule,
    columns 12..16 are zero; fail1 grows over the unmasked run.  The oracle's level-1 masks are checked against the numpy reading of
    Image::buildMaskPyramid in tests/test_oracle_second_reading.py::test_mask_pyramid_second_reading_odd_sizes."""
    sc = synth.make_scene(nviews=4, W=203, H=151, arc_deg=45.0, radius=4.0, kind="multi")
    kw = dict(level=1, csize=1, wsize=5, minImageNum=2, seed=7)
    seeds = synth.make_seeds(sc, level=1, csize=1, stride=2, seed=5)
    o, e = pair(sc, **kw)
    assert e.grid_dims(0) == o.grid_dims(0) == (101, 75) and e.pyramid(0, 1).shape == (75, 101, 3)
    o.close()
    e.close()
    plain, pool_plain = _one_iteration(sc, seeds, None, **kw)
    edge = np.full((sc.nviews, sc.H, sc.W), 255, np.uint8)
    edge[:, :, sc.W - 1] = 0
    edge[:, sc.H - 1, :] = 0
    c_edge, pool_edge = _one_iteration(sc, seeds, edge, **kw)
    assert c_edge == plain and pool_edge.tobytes() == pool_plain.tobytes()
    band = np.full((sc.nviews, sc.H, sc.W), 255, np.uint8)
    assert sc.W // 7 == 29
    band[:, :, 23:34] = 0
    c_band, _ = _one_iteration(sc, seeds, band, **kw)
    assert c_band["fail1"] > 0 and c_band["fail1"] > plain["fail1"] + 100, (c_band, plain)
    assert c_band["inserted"] > 1000
    c_rim, pool_rim = _one_iteration(sc, seeds, 255 - edge, **kw)
    assert c_rim["patches"] > 10000 and c_rim["inserted"] == 0 and c_rim["replaced"] == 0, c_rim
    assert c_rim["fail1"] == c_rim["patches"] - c_rim["fail0"]  # whatever got as far as postProcess failed there
    assert pool_rim.shape[0] == seeds.shape[0] - c_rim["trimmed"]  # the seeds the trim left, nothing else


# ------------------------------------------------------------------ 3 + 4. the whole loop on ragged grids
# (nviews, W, H, arc, kind, level, csize, wsize, minImageNum, stride, view_propagation, max_propag,
#  (patches, inserted) of the oracle in iterations 0 and 1 when the case was chosen: the floors are half of these)
LOOP_CASES = [
    (3, 321, 243, 30.0, "plane", 0, 2, 7, 2, 4, 0, 2, ((14400, 11002), (89791, 82924))),   # grid 161x122: gw odd
    (3, 322, 246, 30.0, "plane", 0, 2, 7, 2, 4, 0, 2, ((14640, 11203), (91259, 84563))),   # 161x123: both odd, even image
    (5, 383, 217, 60.0, "multi", 1, 3, 7, 3, 3, 0, 2, ((8777, 6344), (35465, 28373))),     # 191x108 at level 1, 64x36 cells: 191 = 63 * 3 + 2
    (4, 250, 187, 45.0, "multi", 0, 3, 5, 2, 3, 0, 2, ((18362, 15126), (95358, 83583))),   # 84x63: 250 = 83 * 3 + 1, 187 = 62 * 3 + 1
    (4, 203, 151, 45.0, "multi", 1, 1, 5, 2, 2, 0, 2, ((23146, 11181), (14505, 9214))),    # 101x75 at level 1: both odd
    (4, 203, 151, 45.0, "multi", 1, 1, 5, 2, 2, 1, 2, ((23146, 11181), (14505, 9214))),    # + view propagation: a third source cell per job
    (4, 203, 151, 45.0, "multi", 1, 1, 5, 2, 2, 0, 3, ((23146, 11181), (14505, 9214))),    # + MAX_NUM_OF_PROPAG 3: staging of 2 * 3 * 3 per job
]


def _list_entries_in_outer_cells(sc, recs, level, csize, grids, field, nfield):
    """How many entries of the m_images (field "images") or m_vimages ("vimages") lists of `recs` fall into the last column or row of
    the listed view's grid: the cell of PatchManager::setGrids / setVGrids, floor(x + 0.5) / csize of the projection at `level`."""
    n = 0
    X = recs["coord"].astype(np.float64)
    for k in range(int(recs[nfield].max()) if recs.shape[0] else 0):
        for v in range(sc.nviews):
            sel = (k < recs[nfield]) & (recs[field][:, k] == v)
            if not sel.any():
                continue
            x = X[sel] @ sc.P[v].astype(np.float64).T
            ix = np.floor(x[:, 0] / x[:, 2] / (1 << level) + 0.5).astype(int) // csize
            iy = np.floor(x[:, 1] / x[:, 2] / (1 << level) + 0.5).astype(int) // csize
            inside = (ix >= 0) & (ix < grids[v][0]) & (iy >= 0) & (iy < grids[v][1])
            n += int((inside & ((ix == grids[v][0] - 1) | (iy == grids[v][1] - 1))).sum())
    return n


def _edge_counts(o, nviews):
    """What the outermost column and row of the oracle's grids hold: [kind 0, kind 1] numbers of non-empty cells of
    depth_normal_map in the last column or row, summed over the views (kind 0: the depth maps, which every view's projection of a
    patch reaches; kind 1: the best pool patch by its own cell in its reference view)."""
    out = []
    for kind in (0, 1):
        n = 0
        for v in range(nviews):
            d, _, _ = o.depth_normal_map(v, kind)
            n += int((~np.isnan(d[:, -1])).sum() + (~np.isnan(d[-1, :])).sum())
        out.append(n)
    return out


@pytest.mark.parametrize("case", range(len(LOOP_CASES)))
def test_whole_loop_on_ragged_grids(case):
    """Two iterations of PmMvps::run's loop (Propagate::run, Filter::run, updateThreshold; Optim::check from the second) on grids with
    an odd gw (job_cell's halfw = (gw + 1) / 2 gives one colour a job at cx == gw in every other row; njobs and the staging are
    sized with it) and on sizes csize does not divide (the ix < gw tests of the index, depth-map and Filter::run kernels are all
    that keeps a projection out of the next view's cells).  The left seventh of every mask and the last row of view 0's are zero.

    The outermost cells: in every case the oracle's depth maps (kind 0) have non-empty cells in the last column or row -- other
    views' projections reach them -- which is asserted.  A pool patch whose OWN cell is a partly filled last cell does not occur
    and cannot be made to: Propagate::propagatePatch creates patches at cell centres (propagate.cpp:147-148) and the centre of a
    last cell r < csize pixels wide lies csize k + (csize - 1) / 2 with W = csize k + r, while getTexSafe (optim.cpp:895-915)
    needs centre + wsize / 2 < W - 3 in the reference view, where the window is one pixel per sample: r > 4 + (csize - 1) / 2
    needs csize > 9 even at wsize 3, and the engine takes max_propag * csize^2 <= 32, csize <= 5.  So the kind-1 count is
    printed, not asserted; so are the numbers of m_pgrids and m_vpgrids entries (views listed in m_images / m_vimages) there."""
    nv, W, H, arc, kind, level, csize, wsize, mi, stride, vprop, maxp, table = LOOP_CASES[case]
    sc = synth.make_scene(nviews=nv, W=W, H=H, arc_deg=arc, radius=4.0, kind=kind)
    seeds = synth.make_seeds(sc, level=level, csize=csize, stride=stride, seed=5)
    masks = np.full((nv, H, W), 255, np.uint8)
    masks[:, :, : W // 7] = 0
    masks[0, H - 1, :] = 0
    o, e = pair_sized(sc, masks=masks, full_cells=csize == 3, level=level, csize=csize, wsize=wsize, minImageNum=mi, seed=7, enable_check=1,
                       view_propagation=vprop, max_propag=maxp)
    gw, gh = e.grid_dims(0)
    assert (gw, gh) == o.grid_dims(0)
    Wl, Hl = e.pyramid(0, level).shape[1], e.pyramid(0, level).shape[0]
    assert gw % 2 == 1 or gh % 2 == 1 or Wl % csize or Hl % csize, (gw, gh, Wl, Hl)
    po = loop_two_iterations(o, e, sc, seeds, table, f"case {case}")
    k0, k1 = _edge_counts(o, nv)
    grids = [o.grid_dims(v) for v in range(nv)]
    li = _list_entries_in_outer_cells(sc, po, level, csize, grids, "images", "nimages")
    lv = _list_entries_in_outer_cells(sc, po, level, csize, grids, "vimages", "nvimages")
    print(f"case {case}: outermost column/row of the grids: {k0} depth-map cells, {k1} cells with a pool patch of their own, "
          f"{li} m_pgrids entries, {lv} m_vpgrids entries")
    assert k0 > 0
    de = [e.depth_normal_map(v, 0)[0] for v in range(nv)]
    assert sum(int((~np.isnan(d[:, -1])).sum() + (~np.isnan(d[-1, :])).sum()) for d in de) == k0
    o.close()
    e.close()


# ------------------------------------------------------------------ 5. the window test at coarser levels of an odd image
def _border_seeds(sc, ref, target, n_along=110):
    """Patches on the plane z = 0 whose centres lie in the last 26 columns (and rows) of view `target`, listed as [ref, target]."""
    P = sc.P.astype(np.float64)
    M, p4 = P[target][:, :3], P[target][:, 3]
    C = sc.centers[target]
    uv = []
    for k, u in enumerate(np.linspace(sc.W - 26.0, sc.W - 1.0, n_along)):
        uv.append((u, 30.0 + (k * 37) % (sc.H - 60)))
    for k, v in enumerate(np.linspace(sc.H - 26.0, sc.H - 1.0, n_along)):
        uv.append((30.0 + (k * 53) % (sc.W - 60), v))
    recs = np.zeros(len(uv), dtype=synth.PATCH_DTYPE)
    for i, (u, v) in enumerate(uv):
        d = np.linalg.solve(M, np.array([u, v, 1.0]))
        t = -C[2] / d[2]
        X = C + t * d
        assert abs(X[2]) < 1e-9 and t > 0
        recs["coord"][i] = (X[0], X[1], 0.0, 1.0)
    recs["normal"][:, 2] = 1.0
    recs["ncc"] = -1.0
    recs["flags"] = 1
    recs["nimages"] = 2
    recs["images"][:, 0] = ref
    recs["images"][:, 1] = target
    recs["id"] = np.arange(len(uv))
    return recs


def _level_of(cams, rec, level):
    """The pyramid level Optim::getTex samples the record's second view at (optim.cpp:799-811), by the second reading."""
    X, N = rec["coord"].astype(F), rec["normal"].astype(F)
    px, py = ref_get_paxes(cams[int(rec["images"][0])], X, N, level)
    Pv = cams[int(rec["images"][1])].P[level]
    c = ref_project(Pv, X)
    dx = (ref_project(Pv, (X + px).astype(F)) - c).astype(F)
    dy = (ref_project(Pv, (X + py).astype(F)) - c).astype(F)
    ratio = (np.linalg.norm(dx).astype(F) + np.linalg.norm(dy).astype(F)) / F(2)
    ld = int(np.floor(np.log(float(ratio)) / np.log(2.0) + 0.5))
    return level + max(-level, min(2, ld))


def test_window_test_at_coarser_levels_of_an_odd_image():
    """make_frame takes the size of the level a view is sampled at as W0 >> newLevel; on a 383x217 image the levels are 191x108 and
    95x54, one column (level 1) and three columns and a row (level 2) short of W0 / 2^l, so getTexSafe's window test
    (optim.cpp:895-915) is tighter there than a rounded-up size would make it.  Cameras 2 units from the plane on an 80 degree arc:
    a patch near the plane's edge is far from the reference view and close to the view it is probed in, which therefore samples it
    at level 1 (about a quarter of the seeds; the level is computed here with the second reading's cameras and patch axes).  The
    centres walk across the last 26 columns and rows of that view in steps of a quarter pixel, so both outcomes occur at both
    levels: Optim::preProcess keeps a two-view patch only if the second view passes, and the flag must equal the oracle's for
    every seed."""
    sc = synth.make_scene(nviews=3, W=383, H=217, arc_deg=80.0, radius=2.0, kind="plane")
    o, e = pair(sc, level=0, minImageNum=2)
    assert [e.pyramid(2, l).shape[:2] for l in range(3)] == [(217, 383), (108, 191), (54, 95)]
    seeds = np.concatenate([_border_seeds(sc, 0, 2), _border_seeds(sc, 2, 0), _border_seeds(sc, 1, 2), _border_seeds(sc, 0, 1)[::3]])
    cams = [RefCam(sc.P[v], 0) for v in range(sc.nviews)]
    levels = np.array([_level_of(cams, s, 0) for s in seeds])
    pre_rec, _, pre_flag = e.probe(engine.PROBE_PREPROCESS, seeds)
    flags = np.zeros(len(seeds), np.int32)
    for i, s in enumerate(seeds):
        flags[i], r = o.preprocess(s)
        assert flags[i] == pre_flag[i], (i, levels[i], s["coord"], flags[i], pre_flag[i])
        if flags[i] == 0:
            cmp_records(pre_rec[i], r, f"pre {i}")
    coarse = levels >= 1
    print("seeds", len(seeds), "sampled at level >= 1:", int(coarse.sum()), "accepted", int((flags == 0).sum()), "rejected", int((flags != 0).sum()),
          "coarse accepted", int((coarse & (flags == 0)).sum()), "coarse rejected", int((coarse & (flags != 0)).sum()))
    assert (flags == 0).sum() >= 20 and (flags != 0).sum() >= 20
    assert (coarse & (flags == 0)).sum() >= 20 and (coarse & (flags != 0)).sum() >= 20
    _, got, _ = e.probe(engine.PROBE_NCC, seeds)
    exp = np.array([o.compute_ncc(s) for s in seeds], dtype=np.float32)
    assert np.isfinite(exp).all()
    np.testing.assert_allclose(got, exp, rtol=REL_TOL, atol=1e-5)
    assert (got == exp).mean() > 0.999, f"bit-exact fraction {(got == exp).mean()}"
    o.close()
    e.close()


# ------------------------------------------------------------------ 6. views of unequal size
# (W, H, arc, level, csize, seed stride, the views' sizes): 128x88, 128x88, 121x80, 128x86 cells; 64x44, 64x44, 60x40, 64x43 cells
# last: (patches, inserted) of the oracle in iterations 0 and 1 when the cases were chosen, with the seed lists of seeds_for_sizes
UNEQUAL_CASES = [
    (256, 176, 45.0, 0, 2, 3, [(256, 176), (255, 175), (241, 160), (256, 171)], ((34320, 33016), (101584, 81801))),
    (384, 264, 30.0, 1, 3, 1, [(384, 264), (383, 263), (361, 240), (384, 257)], ((59059, 46551), (51282, 35095))),
]


@pytest.mark.parametrize("case", range(len(UNEQUAL_CASES)))
def test_views_of_unequal_size(case):
    """Four views of one scene cropped top-left to four different sizes, two of them odd (a top-left crop leaves P valid):
    every view has its own pyramid sizes, its own gw x gh and a cell_base that is not a multiple of the others'.  A kernel that
    took W, gw or cell_base from the wrong view would pass every other test of the suite.  Pyramids and grids per view, the whole
    loop with the assertions of test_whole_loop_on_ragged_grids, every view the reference view of 1000 survivors, and the PLY export,
    whose colours are sampled per listed view, against the restatement of tests/test_gpu_ply_export.py."""
    W, H, arc, level, csize, stride, sizes, table = UNEQUAL_CASES[case]
    sc = synth.make_scene(nviews=4, W=W, H=H, arc_deg=arc, radius=4.0, kind="multi")
    o, e = pair_sized(sc, sizes=sizes, full_cells=csize == 3, level=level, csize=csize, wsize=7, minImageNum=2, seed=7, enable_check=1)
    grids = []
    for v, (w, h) in enumerate(sizes):
        for l in range(level + 3):
            pe, po = e.pyramid(v, l), o.pyramid(v, l)
            assert pe.shape == po.shape == (h >> l, w >> l, 3), (v, l)
            np.testing.assert_array_equal(pe, po, err_msg=f"view {v} level {l}")
        want = grid_of(w, h, level, csize)
        assert e.grid_dims(v) == o.grid_dims(v) == want, v
        grids.append(want)
    assert len(set(grids)) >= 3 and len({g[0] for g in grids}) >= 2 and len({g[1] for g in grids}) >= 2
    seeds = seeds_for_sizes(sc, synth.make_seeds(sc, level=level, csize=csize, stride=stride, seed=5), sizes, level)
    assert seeds.shape[0] > 1500
    po = loop_two_iterations(o, e, sc, seeds, table, f"unequal sizes, level {level}")
    refs = np.bincount(po["images"][:, 0], minlength=4)
    print("reference views of the survivors", refs)
    assert refs.min() >= 1000, refs
    shapes = {e.depth_normal_map(v, 0)[0].shape for v in range(4)}
    assert len(shapes) >= 3
    for v in range(4):
        assert e.depth_normal_map(v, 0)[0].shape == o.depth_normal_map(v, 0)[0].shape == (grids[v][1], grids[v][0])
    pe = e.patches()
    Pl, pyr = level_inputs(e, sc, level, sizes=sizes)
    assert e.export_ply() == restate_ply(pe, Pl, pyr)
    assert e.export_ply(binary=True) == restate_ply(pe, Pl, pyr, binary=True)
    pts = e.points()
    np.testing.assert_array_equal(pts["xyz"], pe["coord"][:, :3])
    assert len({tuple(c) for c in pts["rgb"][::50]}) > 10
    o.close()
    e.close()
