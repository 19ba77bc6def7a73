/*
 * mvskit_engine.h -- C ABI of the MI355X PatchMatch-MVS propagation/optimisation engine.
 *
 * This is the drop-in boundary for the hot path of imkaywu/MVSKit:
 *     PmMvps::run  ->  Propagate::run(iter)                       pmmvps/pmmvps.cpp:95
 *         -> propagatePmImage / propagatePatch / generatePatch    pmmvps/propagate.cpp:72-237
 *         -> Optim::preProcess / refinePatch / postProcess        pmmvps/optim.cpp:137-547
 *         -> PatchManager grid operations                         pmmvps/patch_manager.cpp:158-433
 * The reference has no FFI: its boundary is the C++ object graph PmMvps owns by value
 * (pmmvps/pmmvps.hpp:93-103).  A maintainer replaces the body of Propagate::run with calls to the
 * entry points below (INTEGRATION.md shows the patch); mvskit_amd/host/ holds a host-side mirror
 * of Option / PhotoSet / PatchManager / Propagate / PmMvps that does exactly that.
 *
 * Conventions: plain pointers and sizes, no C++ or torch types.  Every call returns 0 on success
 * and a negative mvs_status otherwise (never exit(); the reference exit(1)s, e.g.
 * pmmvps/propagate.cpp:39-42).  Host buffers stay owned by the caller; the engine owns all device
 * memory.  One host thread per handle.  All device work runs on one HIP stream per handle.
 */
#ifndef MVSKIT_ENGINE_H
#define MVSKIT_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef MVS_MAX_IMAGES
#define MVS_MAX_IMAGES 32 /* storage of Patch::m_images / m_vimages in a record; 64 for libmvskit_engine_cap64.so (compile callers with -DMVS_MAX_IMAGES=64) */
#endif
#define MVS_LIST_CAP 16   /* list length of the DEFAULT build (libmvskit_engine.so); the cap32 / cap64 builds hold 32 / 64 views per list.  A library
                           * that holds the data set's view count never cuts a list; ask the loaded one with mvs_list_cap() */

typedef enum mvs_status {
    MVS_OK = 0,
    MVS_ERR_ARG = -1,      /* bad argument / configuration */
    MVS_ERR_STATE = -2,    /* call out of order (views not set, ...) */
    MVS_ERR_HIP = -3,      /* HIP runtime error, see mvs_last_error() */
    MVS_ERR_CAPACITY = -4, /* patch pool or staging capacity exceeded */
    MVS_ERR_NO_DEVICE = -5
} mvs_status;

/* Patch record: pmmvps/patch.hpp:33-66.  coord.w = 1, normal.w = 0.  128 bytes (192 with MVS_MAX_IMAGES 64: mvs_patch_bytes()). */
typedef struct mvs_patch {
    float coord[4];   /* Patch::m_coord */
    float normal[4];  /* Patch::m_normal */
    float ncc;        /* Patch::m_ncc; < 0 = not computed yet (patch.cpp:12) */
    float dscale;     /* Patch::m_dscale */
    float ascale;     /* Patch::m_ascale */
    float tmp;        /* Patch::m_tmp */
    int32_t nimages;  /* m_images.size() */
    int32_t nvimages; /* m_vimages.size() */
    int32_t flags;    /* bit 0: alive; bit 1: the engine's own (the list is settled: Filter::filterExact need not recompute the reference
                       * view while the patch keeps its views; cleared on upload).  In exported "new" records bits 8.. hold the swept view */
    int32_t id;       /* pool index (download) / destination cell (exported "new" records) */
    uint8_t images[MVS_MAX_IMAGES];  /* Patch::m_images, [0] is the reference view */
    uint8_t vimages[MVS_MAX_IMAGES]; /* Patch::m_vimages */
} mvs_patch;

/* Option (pmmvps/option.hpp:20-73) + the engine's own knobs. */
typedef struct mvs_config {
    int32_t nviews;          /* Option::m_nimages */
    int32_t level;           /* Option::m_level */
    int32_t csize;           /* Option::m_csize */
    int32_t wsize;           /* Option::m_wsize (<= 7: the window's samples are dealt over the lanes of one wavefront) */
    int32_t minImageNum;     /* Option::m_minImageNum; tau = min(2 * minImageNum, nviews) must not exceed 16 */
    int32_t max_propag;      /* Propagate::MAX_NUM_OF_PROPAG, propagate.cpp:24 */
    float nccThreshold;      /* Option::m_nccThreshold */
    float maxAngleThreshold; /* Option::m_maxAngleThreshold, radians */
    float quadThreshold;     /* Option::m_quadThreshold */
    int32_t depth;           /* PmMvps::m_depth when Propagate::run is entered */
    uint32_t seed;           /* counter-based RNG seed */
    int32_t refine_steps;    /* halving steps of the refiner, four proposals each; 1 + 4*steps cost evaluations (default 6: 25) */
    float refine_rd0;        /* initial depth range in units of Patch::m_dscale */
    float refine_ra0;        /* initial angle range in units of pi/48 (optim.cpp:487) */
    int32_t enable_check;    /* Optim::check when depth >= 2 (optim.cpp:292) */
    int32_t view_begin;      /* views view_begin, view_begin+view_stride, ... are swept by this engine */
    int32_t view_stride;
    int32_t device;          /* HIP device ordinal */
    int32_t view_propagation;/* 1 = also run the view-propagation branch the reference keeps commented out (propagate.cpp:110-120) */
    int32_t shard_index;     /* shard_count > 1: this engine sweeps the shard_index-th of shard_count equal, contiguous */
    int32_t shard_count;     /*   ranges of the (view, cell) sequence instead of whole views (view_begin/view_stride ignored) */
    int32_t literal_groups;  /* Filter::filterSmallGroups: 0 = groups are the connected components of the symmetrised neighbour relation
                              * (one pass of a union-find; default), 1 = the reference's breadth-first labelling in patch order over the
                              * directed relation (filter.cpp:432-524), exactly: two passes and a small search on the host.
                              * (Sits in what was padding before max_patches: sizeof(mvs_config) is unchanged.) */
    int64_t max_patches;     /* patch pool capacity (0 = 4 * total cells, at most a sixth of the device's memory per pool buffer) */
} mvs_config;

/* The refiner of Optim::refinePatch (optim.cpp:470-547).  The reference minimises cost_func over (depth, angle1, angle2) with NLopt
 * LN_BOBYQA, at most TIME = 500 evaluations (optim.cpp:471) and xtol_rel 1e-7 (optim.cpp:511-524).  mvs_config has no room left, so
 * the choice is a call of its own, mvs_engine_set_refiner; it takes effect at the next mvs_engine_pass / propagate / probe.
 *   HALVING   (default, the engine's own search): refine_steps steps of four proposals, 1 + 4 * refine_steps evaluations, ranges
 *             refine_rd0 / refine_ra0 of mvs_config halved at every step.
 *   CONVERGED a bounded Nelder-Mead (one four-proposal pass per iteration) run until the tolerance holds or the budget is spent:
 *             start simplex x, x + refine_rd0 e0, x + refine_ra0 e1, x + refine_ra0 e2 from the clamped start x; the angle coordinates
 *             of every trial are clamped into [-23.99999, 23.99999] (optim.cpp:496-506), the depth coordinate is unbounded.
 *             Convergence: every coordinate's spread over the four vertices <= xtol * max(1, |x_best,i|); the patch then takes the
 *             best vertex.  Budget: every evaluated proposal counts, the first evaluation at the start included (so do the
 *             evals / view_evals counters); when the next pass would take the count beyond max_evals the run stops as NLopt's
 *             MAXEVAL_REACHED, which refinePatch treats as a failure (optim.cpp:530-545): the patch keeps its starting coordinate,
 *             normal and m_ncc, and the sweep carries on to postProcess as after a converged run.
 * Every rank of a multi-rank job must set the same refiner: the engine does not check it. */
typedef enum mvs_refine_mode { MVS_REFINE_HALVING = 0, MVS_REFINE_CONVERGED = 1 } mvs_refine_mode;
typedef struct mvs_refiner {
    int32_t mode;      /* mvs_refine_mode; HALVING = the search of refine_steps, refine_rd0 / refine_ra0 of mvs_config */
    int32_t max_evals; /* CONVERGED: cost evaluations per candidate, the first one included; default 500 (optim.cpp:471) */
    float xtol;        /* CONVERGED: stop when every coordinate's spread over the simplex <= xtol * max(1, |x_best,i|); default 1e-4, not
                        * the reference's relative 1e-7 (optim.cpp:513): that is about one float32 ulp of the engine's variables */
} mvs_refiner;

/* One view: PhotoSet::m_photos[i] (image/photoSet.hpp:62).  P is the row-major 3x4 level-0 projection
 * (`CONTOUR` camera text, image/camera.cpp:110-116); rgb is the level-0 image as Image::m_images[0]
 * holds it, interleaved uint8 RGB, H rows of W pixels (image/image.hpp:76); mask is H*W uint8 or NULL.
 *
 * Precondition on P: its third row has unit norm in its first three entries, |(P[8], P[9], P[10])| = 1, as K [R | t] with K's last
 * row (0, 0, 1) has (the `CONTOUR2` text always gives that, camera.cpp:117-134; a `CONTOUR` text holds any matrix).  The engine, like
 * the reference, takes P[8..11] . X for the depth along the optical axis without dividing by that norm, and these rely on it:
 *   - Propagate::generatePatch (propagate.cpp:220-237) computes depth = oaxis . X with the normalised axis and then
 *     unproject(depth * (u, v, 1)), whose third coordinate is P[8..11] . X: with another norm the new patch lies at another depth;
 *   - the depth arguments of mvs_engine_seed_random: a hypothesis at depth d is unproject(d * (px, py, 1));
 *   - mvs_engine_depth_ranges, which returns oaxis . X (normalised) and whose ranges are meant for seed_random;
 *   - ipscale = P_row0 . xaxis + P_row1 . yaxis (Optim::setAxesScales, optim.cpp:43-65), fx + fy only at that scale, and with it
 *     Optim::getUnit, the patch axes and every threshold in pixels.
 * mvs_engine_set_views does not check or rescale P.  A caller that holds a general `CONTOUR` matrix divides all twelve entries by
 * |(P[8], P[9], P[10])| first: a projection matrix is defined up to scale, so no pixel moves. */
typedef struct mvs_view_desc {
    int32_t width, height;
    float P[12];
    const uint8_t* rgb;
    const uint8_t* mask;
} mvs_view_desc;

/* Propagate's counters (pmmvps/propagate.hpp:63-69) plus work counts for the metric. */
typedef struct mvs_counters {
    int64_t candidates;  /* generatePatch returned a patch */
    int64_t prefiltered; /* cand.ncc < worst.ncc, propagate.cpp:170 */
    int64_t patches;     /* reached Optim::preProcess, propagate.cpp:182 -- the unit of "patches/s" */
    int64_t fail0;       /* m_fcount0 */
    int64_t fail1;       /* m_fcount1 */
    int64_t inserted;    /* pcount */
    int64_t replaced;    /* rcount */
    int64_t evals;       /* texture evaluations (one getPAxes + up to V getTex) */
    int64_t view_evals;  /* getTex calls that sampled: 588 algorithmic bytes each */
    int64_t trimmed;     /* removed by the MAX_NUM_OF_PATCHES trim */
} mvs_counters;

typedef struct mvs_engine mvs_engine;

const char* mvs_last_error(void);
int mvs_device_count(void);
/* Patch::m_images / m_vimages are unbounded in the reference (optim.cpp:165-205 pushes every qualifying view); the engine keeps
 * them in wavefront lanes, one view per lane.  Three builds of the same sources: libmvskit_engine.so holds 16 views per list,
 * libmvskit_engine_cap32.so 32, libmvskit_engine_cap64.so 64 (= the engine's view limit; 192-byte records).  Load the smallest one
 * whose mvs_list_cap() >= the data set's view count: then NO list is ever cut.  A smaller library on a larger data set keeps the
 * first mvs_list_cap() entries of a list (mvskit_amd.engine.Engine and the host mirror pick the library by view count). */
int mvs_list_cap(void);
int mvs_patch_bytes(void); /* sizeof(mvs_patch) in this build of the library: 128, or 192 in libmvskit_engine_cap64.so -- a caller checks it against its own */
void mvs_default_config(mvs_config* cfg); /* Option::Option, option.cpp:19-33 */
void mvs_default_refiner(mvs_refiner* r); /* HALVING, max_evals 500, xtol 1e-4 */

/* PmMvps::init (pmmvps.cpp:18-68): thresholds, tau = min(2*minImageNum, nviews), maxLevel = level+3.
 * LIMITS -- Option::init (pmmvps/option.cpp:53-116) takes any value; the engine returns MVS_ERR_ARG outside these:
 *     nviews            1 .. 64      one wavefront lane per view in the per-view stages (64-view lists need libmvskit_engine_cap64.so)
 *     wsize             1 .. 7       the wsize^2 samples of a window are dealt over 3 slots x 16 lanes + one extra sample (49)
 *     tau               <= 16        tau = min(2 * minImageNum, nviews) views of a proposal sit in 16 frame lanes: any minImageNum
 *                                    on <= 16 views, minImageNum <= 8 beyond
 *     max_propag*csize^2 <= 32       MAX_NUM_OF_PATCHES (propagate.cpp:24-25): a cell's live list is held in 32 lanes; max_propag <= 16
 *     level             0 .. 4       level + 3 pyramid levels, 7 at most
 *     images            >= 8 x 8 pixels at level 0 (mvs_engine_set_views)
 * and MVS_ERR_CAPACITY at run time beyond: max_patches records in the pool (default 4 per cell), 2^30 patches (ids of staged
 * records start at 0x40000000), and 14336 distinct patches / 4064 neighbours around one patch in Optim::check / filterNeighbor. */
int mvs_engine_create(const mvs_config* cfg, mvs_engine** out);
int mvs_engine_destroy(mvs_engine* e);
/* the refiner of every later pass / propagate / probe (see mvs_refiner); MVS_ERR_ARG on an unknown mode, max_evals outside 5..4096,
 * or xtol not finite or <= 0.  An engine that never calls it runs HALVING. */
int mvs_engine_set_refiner(mvs_engine* e, const mvs_refiner* r);

/* PhotoSet::init + Image::buildImagePyramid + Camera::updateCamera + Optim::setAxesScales +
 * PatchManager::init: uploads level 0, builds pyramids, cameras and grids on the device. */
int mvs_engine_set_views(mvs_engine* e, int nviews, const mvs_view_desc* views);
int mvs_engine_grid_dims(mvs_engine* e, int view, int* gw, int* gh); /* patch_manager.cpp:36-37 */
int mvs_engine_get_pyramid(mvs_engine* e, int view, int level, uint8_t* rgb_out, int* W, int* H);

/* thresholds: PmMvps::m_nccThreshold, m_nccThresholdBefore, m_depth */
int mvs_engine_set_thresholds(mvs_engine* e, float nccThreshold, float nccThresholdBefore, int depth);
int mvs_engine_get_thresholds(mvs_engine* e, float* nccThreshold, float* nccThresholdBefore, int* depth);
int mvs_engine_update_threshold(mvs_engine* e); /* PmMvps::updateThreshold + ++m_depth, pmmvps.cpp:70-74,105 */

/* PatchManager::readPatches tail (patch_manager.cpp:450-463): seeds -> pool */
int mvs_engine_upload_patches(mvs_engine* e, int64_t n, const mvs_patch* patches);
int mvs_engine_clear_patches(mvs_engine* e);
/* DepthNormInit::createPatches with isTest = 0 (pmmvps/depth_normal_init.cpp:34-91): the seed patches from a depth point cloud and one
 * photometric-stereo normal map per view, built on the device and appended to the pool in point order.  Per point: project into
 * every view at level 0 (PhotoSet::project), take the pixel floorf(x + 0.5f); a view takes part when that pixel lies inside the image
 * and its mask byte is foreground (> 127, the rule of mvs_engine_set_views); the views' normals at those pixels are summed in view
 * order, divided by the number of views, then by the norm (depth_normal_init.cpp:66-73), normal.w = -coord . n; the views are ordered
 * by Optim::sortImages(patch, 0) (optim.cpp:221-258).  No patch for a point with fewer than two views, a zero sum, or -- unlike the
 * reference, which keeps such a patch with an empty m_images in no grid cell -- fewer than two views left by sortImages.  A map pixel
 * outside the image is never read (the reference reads out of bounds there).  The record is what mvs_engine_upload_patches makes of
 * the mirror's: list cut to mvs_list_cap() after the sort, m_vimages empty, m_ncc = -1, m_tmp = score2, alive.
 *   xyz     3 * npoints float32, world coordinates (DepthNormInit::readDepths)
 *   views   one mvs_seed_view per view of mvs_engine_set_views, in that order, with that view's width and height:
 *           normals  H*W*3 float32 in world axes (what DepthNormInit::readNormals leaves: R * n), (0, 0, 0) = no normal there: the view
 *                    still counts; NULL: the view takes no part
 *           mask     H*W level-0 mask bytes as mvs_view_desc.mask (the engine itself keeps masks at Option::m_level only); NULL: the
 *                    view takes no part (PhotoSet::getMask = -1)
 *   n_added the number of patches appended (may be NULL)
 * LIMITS: npoints <= 2^31 - 4097 per call.  Device memory for the call, released before it returns: 44 bytes per point and 13 bytes
 * per pixel of the largest view (the views stream through one buffer, whatever their number).  Two calls on the same input give the
 * same pool bytes (positions come from a scan, not from atomics).  A second call appends.
 * MVS_ERR_ARG: npoints negative, xyz (with npoints > 0) or views NULL, no engine (checked in that order, before the handle is read);
 * MVS_ERR_STATE: views not set, or a pass waiting for its commit; MVS_ERR_HIP: an allocation or copy failed; MVS_ERR_CAPACITY: the
 * patches do not fit the pool.  After any error the pool is what it was. */
typedef struct mvs_seed_view {
    const float* normals;
    const uint8_t* mask;
} mvs_seed_view;
int mvs_engine_seed_patches(mvs_engine* e, int64_t npoints, const float* xyz, const mvs_seed_view* views, int64_t* n_added);
/* The cold start, for a caller who has images, masks and cameras but no depth point cloud: seed patches from random plane hypotheses
 * scored on the device (PatchMatch stereo's usual start; no reference counterpart -- it stands where DepthNormInit::createPatches
 * stands).  A job is a cell c = cy * gw + cx of a view v; the jobs run over all views and all cells, in (view, cell) order.
 *   1. mask gate   the cell centre (propagate.cpp:147-148) at Option::m_level, pixel floorf(ic + 0.5f): outside the image, or on the
 *                  background of a view that has a mask -> the job gives nothing.
 *   2. hypotheses  `hypotheses` planes, hypothesis k from five draws u_j in [-0.5, 0.5) of the call's own counter-based stream (`seed`,
 *                  the constant 0x5eed0001, v, c, k, j -- mvs_config.seed plays no part): the pixel (icx + csize u0, icy + csize u1);
 *                  the depth uniform in inverse depth, 1/d = 1/dmax + (u2 + 0.5)(1/dmin - 1/dmax), along the view's optical axis;
 *                  coord = Camera::unproject(d (px, py, 1)); the normal at the angle theta = max_tilt sqrt(u3 + 0.5) from the unit
 *                  vector r towards the camera centre, in the direction phi = 2 pi (u4 + 0.5) of Filter::ortho's frame of r, normalised;
 *                  normal.w = -coord . n.  The record: m_images = [v], no m_vimages, m_ncc = -1, scales and m_tmp 0, alive, id = k.
 *   3. score       every hypothesis through Optim::preProcess and, when that passes, PatchManager::computeNcc on its result; the winner
 *                  is the highest score, the lowest k among equals, and must score strictly above min_ncc -- else the job gives nothing.
 *   4. patch       the winner through Optim::refinePatch with the engine's refiner (mvs_engine_set_refiner; HALVING draws under the key
 *                  (0, 0, c, 0) as MVS_PROBE_REFINE does for record c; a CONVERGED run that spends its budget keeps its start), then
 *                  Optim::postProcess.  Optim::check does not run, whatever the depth.  A job whose postProcess passes gives one patch.
 *   5. append      the patches, in (view, cell) order, behind the pool: positions come from a scan, not from atomics, so two calls on
 *                  the same state give the same pool bytes.  Records are alive, not settled, id = the pool index.
 * Steps 3 and 4 are the functions behind mvs_engine_probe's ops 1, 0, 2 and 3, called as those call them: an appended record has the
 * bytes that chain of probes gives.  postProcess reads the depth maps when the engine's depth > 0: they are built from the pool as it is
 * at entry (nothing else of a pass's index build runs: no patch is scored or trimmed), so the patches of one call do not see each
 * other and the result does not depend on launch order.  One consequence: MVS_PROBE_POSTPROCESS runs the whole index build, which
 * kills the patches beyond MAX_NUM_OF_PATCHES of an over-full cell before the depth maps are made.  Over a pool with such a cell and
 * depth > 0 the maps of the two can differ, and the equality with the chain of probes holds only for a pool that build would not trim
 * (an empty pool, or one a pass has left).  Existing records are never modified; the cell indexes, the thresholds and the
 * mvs_config.seed stream stay as they were; a second call appends again.  Not a collective: every rank of a multi-rank job makes the same
 * call and ends with the same pool, as with mvs_engine_seed_patches.  Device memory for the call, released before it returns: one
 * record and eight bytes per cell of the largest view.
 * MVS_ERR_ARG: s null, hypotheses outside 1..64, a range pointer null, max_tilt not in (0, pi/3], no engine -- checked in that order,
 * before the handle is read -- then, with the engine's view count, a range entry that is not finite or not 0 < min < max.
 * MVS_ERR_STATE: views not set, or a pass waiting for its commit; MVS_ERR_HIP: an allocation or copy failed; MVS_ERR_CAPACITY: the patches
 * do not fit the pool (known before the pool is written).  After any error the pool is what it was. */
typedef struct mvs_seed_random {
    int32_t hypotheses;      /* K, 1..64 per cell */
    uint32_t seed;           /* own counter-based stream, independent of mvs_config.seed */
    float max_tilt;          /* radians, 0 < max_tilt <= pi/3: largest angle between a hypothesis normal and the direction to the camera */
    float min_ncc;           /* a winner must score above this; < 0 = the engine's nccThresholdBefore at the call */
    const float* depth_min;  /* [nviews] depth range along each view's optical axis (oaxis . X), 0 < min < max, finite */
    const float* depth_max;
} mvs_seed_random;           /* 32 bytes */
void mvs_default_seed_random(mvs_seed_random* s); /* K 8, seed 1, max_tilt pi/3, min_ncc -1, ranges NULL */
int mvs_engine_seed_random(mvs_engine* e, const mvs_seed_random* s, int64_t* n_added /* may be NULL */);
/* The diagnostic window of step 2: the hypotheses mvs_engine_seed_random builds -- by the same device function -- for the listed cells of
 * `view` (any cell of the grid, whatever the mask gate makes of it), hypothesis k of cells[i] at out[i * K + k].  Only reads engine state.
 * MVS_ERR_ARG as above, then: ncells negative, cells or out null (with ncells > 0), no engine; with the engine: view outside
 * 0..nviews-1, a range entry as above, a cell outside the view's grid.  MVS_ERR_STATE: views not set. */
int mvs_engine_seed_random_hypotheses(mvs_engine* e, const mvs_seed_random* s, int view, int64_t ncells, const int32_t* cells,
                                      mvs_patch* out /* ncells * K */);
/* The warm start, for a caller who has images, cameras and the sparse 3-D points of structure-from-motion -- no normals, no per-view maps:
 * a second front end to the cold start's chain (the PMVS-style start: the normal turned towards the reference camera, then optimised).
 * A job is point i of xyz, coord = (x, y, z, 1); the jobs run over the points in their order.
 *   1. gate        view v qualifies for the point when its depth d = oaxis . coord (the 4-vector product mvs_engine_depth_normal_map
 *                  calls depth) is > 0, the pixel floorf(ic + 0.5f) of its projection at Option::m_level lies inside the image at that
 *                  level and, where the view has a mask, on its foreground at that level (a view without a mask is foreground everywhere,
 *                  the cold start's rule).  A non-finite coordinate qualifies nowhere.
 *   2. hypotheses  the first min(`hypotheses`, qualifying views) views in ascending squared distance |center_v - X|^2, the lower view
 *                  index first among equals.  Hypothesis k: reference view v_k, the point's coordinate untouched, the normal the unit
 *                  vector r from the point to the centre of camera v_k, normal.w = -coord . r.  The record: m_images = [v_k], no
 *                  m_vimages, m_ncc = -1, scales and m_tmp 0, alive, id = k.
 *   3. score, 4. patch   as the cold start's steps 3 and 4, over the point's hypotheses; HALVING draws under the key (0, 0, i, 0) with
 *                  the point's index i in the call, as MVS_PROBE_REFINE does for record i.  Optim::check does not run.
 *   5. append      the patches, in point order, behind the pool: positions come from a scan, not from atomics, so two calls on the same
 *                  state give the same pool bytes.  Records are alive, not settled, id = the pool index.  No thinning: several points of
 *                  one cell give several patches, and the next pass's MAX_NUM_OF_PATCHES trim keeps the best.
 * An appended record has the bytes the chain of probes gives (ops 1, 0, 2, 3 over the hypotheses of the diagnostic window below).  The
 * depth maps postProcess reads when the engine's depth > 0 are built from the pool as it is at entry, with the cold start's caveat: over a
 * pool with an over-full cell (one an index build would trim) and depth > 0 the maps of MVS_PROBE_POSTPROCESS can differ, and the
 * equality with the chain holds only for a pool that build would not trim.  Existing records are never modified; the cell indexes, the
 * thresholds and the mvs_config.seed stream stay as they were; a second call appends again.  Not a collective: every rank of a multi-rank
 * job makes the same call and ends with the same pool.  The points stream through fixed buffers in chunks of 2^18 (the environment
 * variable MVS_SEED_POINTS_CHUNK, a positive integer read at the call and cut to 2^22, overrides it; the pool bytes do not depend on
 * it): device memory for the call, released before it returns, is one record and 20 bytes per point of a chunk.
 * LIMITS: npoints <= 2^30 per call.
 * MVS_ERR_ARG: s null, hypotheses outside 1..64, npoints negative, xyz null (with npoints > 0), no engine, npoints over the limit --
 * checked in that order, before the handle is read.  MVS_ERR_STATE: views not set, or a pass waiting for its commit; MVS_ERR_HIP: an
 * allocation or copy failed; MVS_ERR_CAPACITY: the patches do not fit the pool (the pool is written only after the last chunk).  After
 * any error the pool is what it was, and a refused call writes nothing through n_added.  npoints == 0 appends nothing. */
typedef struct mvs_seed_points {
    int32_t hypotheses;      /* K, 1..64: at most K reference-view hypotheses per point, nearest qualifying views first */
    float min_ncc;           /* a winner must score strictly above this; < 0 = the engine's nccThresholdBefore at the call */
} mvs_seed_points;           /* 8 bytes */
void mvs_default_seed_points(mvs_seed_points* s); /* K 4, min_ncc -1 */
int mvs_engine_seed_points(mvs_engine* e, const mvs_seed_points* s, int64_t npoints, const float* xyz, int64_t* n_added /* may be NULL */);
/* The diagnostic window of steps 1 and 2: the hypotheses the warm start builds -- by the same device function -- for every point:
 * count[i] of them for point i, hypothesis k at out[i * K + k], all-zero bytes in the slots behind.  Only reads engine state.
 * LIMITS: npoints * K <= 2^31 - 1.  MVS_ERR_ARG as above up to xyz, then: out or count null (with npoints > 0), no engine, the limit.
 * MVS_ERR_STATE: views not set. */
int mvs_engine_seed_points_hypotheses(mvs_engine* e, const mvs_seed_points* s, int64_t npoints, const float* xyz,
                                      mvs_patch* out /* npoints * K */, int32_t* count /* npoints */);
/* The depth range the same points give every view, as the cold start's depth_min / depth_max take it: count[v] = the number of points
 * that pass view v's gate (step 1 above, d > 0 included), and the smallest and largest d among them -- the exact float extremes, whatever
 * the order (an integer minimum / maximum over the bits of positive floats) -- widened on the host: depth_min = min / (1 + margin),
 * depth_max = max * (1 + margin).  A view with no qualifying point gets count 0 and the range 0, 0, which the cold start refuses.  Only
 * reads engine state.  LIMITS: npoints <= 2^30.
 * MVS_ERR_ARG: npoints negative, xyz null (with npoints > 0), depth_min, depth_max or count null, margin not finite or < 0, no engine,
 * npoints over the limit -- checked in that order, before the handle is read.  MVS_ERR_STATE: views not set.  A refused call writes
 * nothing through its output pointers. */
int mvs_engine_depth_ranges(mvs_engine* e, int64_t npoints, const float* xyz, float margin,
                            float* depth_min, float* depth_max, int64_t* count /* each [nviews] */);
/* Optional: sizes the two cell indexes (PatchManager::m_pgrids / m_vpgrids as lists, patch_manager.hpp) for `list_entries` memberships
 * each up front -- 0 = MAX_NUM_OF_PATCHES per cell of every view -- so that the calls below allocate nothing while the lists stay
 * below that.  Without it the buffers grow inside the first iterations of a run.  A buffer that the call allocates is written once
 * (the first use of fresh device memory is slow); a request the buffers already hold changes nothing. */
int mvs_engine_reserve(mvs_engine* e, int64_t list_entries);
int mvs_engine_num_patches(mvs_engine* e, int64_t* n_alive);
int mvs_engine_download_patches(mvs_engine* e, int64_t cap, mvs_patch* out, int64_t* n); /* collectPatches */

/* PatchManager::writePly (patch_manager.cpp:542-633): the whole PLY file of the alive pool, header included, vertices in the order of
 * mvs_engine_download_patches.  Per vertex: x y z nx ny nz (coord, normal) and diffuse_red / green / blue, the mean over m_images of a
 * bilinear sample of the level-`level` pyramid at the patch's projection; a listed view the point lies behind or projects outside of
 * [0, W-1) x [0, H-1) counts in the mean but adds nothing; 128 grey for an empty list.
 *   MVS_PLY_ASCII       "format ascii 1.0", one line "x y z nx ny nz r g b\n" per vertex with the floats as printf("%g", (double)v)
 *                       writes them -- byte for byte what std::ostream writes;
 *   MVS_PLY_BINARY_LE   "format binary_little_endian 1.0", 27 bytes per vertex: 6 float32, 3 uint8; the same numbers.
 * out == NULL or cap < the size: *nbytes = the exact size (MVS_ERR_CAPACITY when out != NULL; out is then not written).  The size of an
 * ASCII file costs one pass over the pool on the device; a call whose cap holds 90 bytes per vertex skips it.  The call only reads:
 * pool, indexes, thresholds and RNG state stay as they were; not a collective (every rank holds the whole pool).  Device memory: fixed
 * buffers of ~110 MB for the call, whatever the pool's size.  MVS_ERR_ARG: bad format, nbytes NULL, no engine (checked in that order,
 * before the handle is read); MVS_ERR_STATE: views not set, or a pass waiting for its commit. */
typedef enum mvs_ply_format { MVS_PLY_ASCII = 0, MVS_PLY_BINARY_LE = 1 } mvs_ply_format;
int mvs_engine_export_ply(mvs_engine* e, int format, int64_t cap, uint8_t* out, int64_t* nbytes);

/* Dense per-view maps and their cross-view fusion (no reference counterpart: the reference stops at the patches).  PatchMatch keeps a
 * plane per cell; the dense map of a view is that plane evaluated at every pixel of the cell, at the working resolution: L =
 * Option::m_level, view v has W_L x H_L pixels, the projection P_L, Minv (the inverse of its 3x3 block), the centre C and oaxis.
 *   1. selection   per cell of every view.  source 0: among the alive patches whose reference view (images[0]) is v, the one with the
 *                  highest m_ncc in the cell PatchManager::setGrids' rule gives it, the lowest id among equals (kind 1 of
 *                  mvs_engine_depth_normal_map); all views in one pass over the pool.  source 1: the cell's m_dpgrids entry (kind 0).
 *   2. render      pixel (x, y) of v, integers, lies in the cell (x / csize, y / csize); p = the cell's selection, n = p.normal.xyz, X0 =
 *                  p.coord.xyz.  dir = Minv (x, y, 1); t = n.(X0 - C) / (n.dir); X = C + t dir; depth = oaxis . (X, 1).  The pixel is
 *                  VALID when the cell has a selection, the view has no mask or its level-L mask is foreground at (x, y), n.dir is finite
 *                  and not zero, t > 0, and depth > 0 and finite (a NaN fails every one of these).  Per pixel: depth; normal = the
 *                  three floats of p.normal and conf = p.ncc, bit for bit; id = the pool index (what mvs_engine_download_patches calls
 *                  id as long as no patch is dead); invalid pixels: quiet NaN and id -1.
 *   3. agreement   a valid pixel of v with point X and normal n, against every view u != v: project X (Camera::project at level L), take
 *                  the pixel (floorf(ic.x + 0.5f), floorf(ic.y + 0.5f)).  Bit u of the pixel's 64-bit agree word is set when the third
 *                  homogeneous coordinate is > 0; that pixel lies inside u's image and is valid in u's render, with patch q;
 *                  |s - 1| <= depth_tol for s = n_q.(X0_q - C_u) / (n_q.(X - C_u)) -- the relative depth difference, along u's ray through
 *                  X, between X and q's plane (no depth map is read, the pixel size plays no part; a zero or non-finite denominator
 *                  fails); and n . n_q >= normal_cos (skipped when normal_cos <= -1).  Bit v is never set; agree = 0 on invalid pixels.
 *   4. fusion      a pixel is emitted when it is valid, popcount(agree) >= min_consistent and, with dedupe != 0, no bit u < v is set in
 *                  agree: the lowest view of an agreeing set speaks for the surface point.  The records come in (view, y, x) order at
 *                  positions from a scan, not from atomics: two calls on the same state give the same bytes.  rgb = the level-L pyramid
 *                  texel of view v at (x, y).
 * Both calls are stateless -- each renders what it needs and keeps nothing afterwards, so no map can go stale -- and only read engine
 * state: pool, cell indexes, thresholds and the RNG stream stay as they were (source 1 rebuilds m_dpgrids from the pool, as
 * mvs_engine_depth_normal_map does).  Neither is a collective: every rank holds the whole pool.  Output pointers may be host or device
 * memory (hipMemcpyDefault).  Device memory for a call, released before it returns: 16 bytes (an id and a point) per pixel of ALL views
 * -- and a flag byte more in mvs_engine_fused_points -- plus, per pixel of the LARGEST view, 8 bytes of agree words, 8 of scan and 20 of
 * output maps (32 per emitted pixel of one view instead of the maps in mvs_engine_fused_points): the views stream through those.  48
 * views of 4096 x 2160: 7.2 GB + 0.3 GB.
 * mvs_engine_render_maps: out[v] takes view v's maps (depth H*W, normal H*W*3, conf, ids, agree; any pointer NULL: not wanted; out NULL:
 *   none), n_valid[v] its number of valid pixels.
 * mvs_engine_fused_points: out == NULL or cap < the count: *n = the exact count (MVS_ERR_CAPACITY when out != NULL; out is then not
 *   written), mvs_engine_export_ply's convention.
 * MVS_ERR_ARG, checked in this order before the handle is read: config NULL, source outside 0..1, min_consistent < 0, depth_tol not
 * finite or <= 0, normal_cos not finite or > 1, (fused_points) cap < 0 or n NULL, no engine; then, with the engine's view count,
 * min_consistent > nviews - 1.  MVS_ERR_STATE: views not set, or a pass waiting for its commit; MVS_ERR_HIP: an allocation or copy
 * failed.  A refused call writes nothing through its output pointers. */
typedef struct mvs_maps_config {
    int32_t source;          /* 0: the best-NCC patch of the cell with reference view v; 1: the cell's m_dpgrids patch */
    int32_t min_consistent;  /* fusion: at least that many agreeing other views */
    float depth_tol;         /* agreement: |s - 1| <= depth_tol */
    float normal_cos;        /* agreement: n . n_q >= normal_cos; <= -1: no normal test */
    int32_t dedupe;          /* fusion: != 0 = only the lowest view of an agreeing set emits */
    int32_t pad;
} mvs_maps_config;           /* 24 bytes */
void mvs_default_maps_config(mvs_maps_config* c); /* source 0, min_consistent 1, depth_tol 0.01, normal_cos 0.9, dedupe 1 */
typedef struct mvs_view_maps {
    float* depth;     /* H*W */
    float* normal;    /* H*W*3 */
    float* conf;      /* H*W */
    int32_t* ids;     /* H*W */
    uint64_t* agree;  /* H*W */
} mvs_view_maps;      /* 40 bytes */
int mvs_engine_render_maps(mvs_engine* e, const mvs_maps_config* c, mvs_view_maps* out /* [nviews] or NULL */, int64_t* n_valid /* [nviews] or NULL */);
typedef struct mvs_fused_point {
    float xyz[3];
    float normal[3];
    float conf;
    uint8_t rgb[3];
    uint8_t view;
} mvs_fused_point;    /* 32 bytes */
int mvs_engine_fused_points(mvs_engine* e, const mvs_maps_config* c, int64_t cap, mvs_fused_point* out /* host or device */, int64_t* n);

/* Triangle mesh: a truncated signed distance volume over the dense maps, then marching tetrahedra (no reference counterpart).  The
 * volume is a lattice of nx x ny x nz points; point (i, j, k) has the linear index p = (k ny + j) nx + i and the position origin[c] +
 * (float)idx[c] * voxel (one multiplication, one addition).  fp32 throughout, IEEE division, no atomics: every position in an output
 * comes from a scan, so two calls give the same bytes.
 * mvs_engine_tsdf: renders and computes agreement exactly as mvs_engine_fused_points does (stateless, reads the engine only).  A pixel
 *   is USABLE when it is valid and popcount(agree) >= c->min_consistent; dedupe plays no part.  For lattice point X the views v = 0 ..
 *   nviews-1 are walked in ascending order:
 *     1. ic = Camera::project(v, (X, 1)) at level L; ic.z > 0; the pixel (floorf(ic.x + 0.5f), floorf(ic.y + 0.5f)) lies inside the
 *        image at level L and is usable, with patch q;
 *     2. den = n_q.(X - C_v), num = n_q.(X0_q - C_v) (the agreement step's expressions); den finite and not zero; s = num / den;
 *        dz = oaxis_v.(X, 1) > 0;
 *     3. sd = (s - 1.0f) * dz: the signed distance, in depth units, from X to q's plane along v's ray; positive in front of the
 *        surface, exact for a planar scene;
 *     4. when sd >= -trunc: sum = sum + fminf(sd / trunc, 1.0f), n = n + 1; otherwise the view says nothing about X.
 *   count[p] = n; tsdf[p] = sum / (float)n, a quiet NaN when n == 0.  A NaN fails every comparison above.  Device memory for the call:
 *   17 bytes per pixel of all views and 16 per pixel of the largest (the maps), 8 per lattice point.
 * mvs_engine_extract_mesh: marching tetrahedra over a caller's volume (tsdf and count: host or device, count may be NULL); needs a
 *   device but no views.
 *     OBSERVED   tsdf[p] is not NaN and count[p] >= min_count (count == NULL: every non-NaN point); INSIDE: observed and tsdf < 0 (an
 *                exact zero is outside).
 *     EDGES      cube corners are numbered c = dx + 2 dy + 4 dz; every cube is split into the six tetrahedra along its main diagonal,
 *                as corner tuples (0,1,3,7) (0,1,5,7) (0,2,3,7) (0,2,6,7) (0,4,5,7) (0,4,6,7).  Every tetrahedron edge is a lattice
 *                point p (the endpoint with the lower coordinates) plus a direction d = dx + 2 dy + 4 dz in 1..7; its slot is d - 1.
 *     VERTICES   one per edge (p, d) whose endpoints a = p and b = p + d lie in the lattice, are both observed, and of which exactly one
 *                is inside: t = Fa / (Fa - Fb), pos = pa + t * (pb - pa) per component, in that order of operations.  Vertices are
 *                numbered by ascending (p, slot).  A vertex on the rim of the observed region that no triangle uses may occur.
 *     TRIANGLES  only cubes whose eight corners are all observed give triangles: in ascending cube order (the linear index of corner
 *                0), tetrahedra in the order above, at most two each.  With the tetrahedron's corners in ascending position: one
 *                corner a differs from the other three b < c < d: (e(a,b), e(a,c), e(a,d)); two inside a < b and two outside c < d:
 *                (q0,q1,q2) and (q0,q2,q3) with q = e(a,c), e(a,d), e(b,d), e(b,c).  The normal (v1 - v0) x (v2 - v0) points from the
 *                inside corners to the outside ones (towards the cameras): a triangle that would not is emitted with its second and
 *                third vertex swapped.  Vertex ids are int32, three per triangle.
 *   Sizes follow mvs_engine_export_ply's convention: with verts == NULL, tris == NULL or a cap (in vertices / triangles) too small, *n_v
 *   and *n_t are the exact counts and nothing else is written; MVS_ERR_CAPACITY when a non-NULL output is too small.  Device memory for
 *   the call: 18 bytes per lattice point (two bytes of flags, a count, the vertex scan and the 64-bit triangle scan), 8 more for a
 *   volume that comes from the host, and the mesh itself (12 bytes a vertex, 12 a triangle).
 * mvs_engine_mesh: mvs_engine_tsdf, then mvs_engine_extract_mesh on its volume, which stays on the device; the same bytes.
 * LIMITS: each dimension 2..1024, nx ny nz <= 2^28.
 * MVS_ERR_ARG, checked in this order before the handle is read: (tsdf, mesh) the config checks of mvs_engine_fused_points; the volume
 * NULL; voxel, then trunc, not finite or <= 0; a dimension outside 2..1024; the product over 2^28; min_count < 1; (tsdf) tsdf or count
 * NULL; (extract_mesh) tsdf NULL; (extract_mesh, mesh) n_v or n_t NULL, a negative cap; no engine; then (tsdf, mesh) min_consistent >
 * nviews - 1.  MVS_ERR_STATE (tsdf, mesh): views not set, or a pass waiting for its commit; extract_mesh asks
 * for a device only, which every engine has (mvs_engine_create fails without one).  MVS_ERR_HIP: an allocation or copy
 * failed.  A refused call writes nothing. */
typedef struct mvs_volume {
    float origin[3];    /* world position of lattice point (0,0,0) */
    float voxel;        /* lattice spacing, > 0, finite */
    int32_t dims[3];    /* nx, ny, nz lattice points */
    float trunc;        /* truncation distance in depth units, > 0, finite */
    int32_t min_count;  /* a lattice point is OBSERVED when at least this many views contributed; >= 1 */
    int32_t pad;
} mvs_volume;           /* 40 bytes */
int mvs_engine_tsdf(mvs_engine* e, const mvs_maps_config* c, const mvs_volume* vol, float* tsdf /* [nz ny nx] */, int32_t* count /* alike */);
int mvs_engine_extract_mesh(mvs_engine* e, const mvs_volume* vol, const float* tsdf, const int32_t* count /* or NULL */, int64_t cap_v,
                            float* verts /* [cap_v][3] */, int64_t cap_t, int32_t* tris /* [cap_t][3] */, int64_t* n_v, int64_t* n_t);
int mvs_engine_mesh(mvs_engine* e, const mvs_maps_config* c, const mvs_volume* vol, int64_t cap_v, float* verts, int64_t cap_t, int32_t* tris,
                    int64_t* n_v, int64_t* n_t);

/* Vertex normals and colours of a triangle mesh (no reference counterpart): what a viewer needs to show the mesh shaded and coloured.
 * verts: n_v x 3 floats, tris: n_t x 3 int32 vertex ids -- those of mvs_engine_mesh, or any caller's.  Both calls are stateless and only
 * read the engine; all pointers may be host or device memory (hipMemcpyDefault).
 * mvs_engine_mesh_normals: area-weighted vertex normals as an ORDER-FREE INTEGER SUM: the result does not depend on the order in which the
 *   hardware meets the triangles or in which they are listed, two calls give the same bytes, and a vertex of any valence costs what any
 *   other costs per triangle (a fan of tens of thousands of triangles round one vertex included): no sorted float sum.  Needs a device
 *   but no views, like mvs_engine_extract_mesh.
 *     FACE VECTOR  e1 = v1 - v0, e2 = v2 - v0, f = e1 x e2 in fp32 without contraction, each component a*b - c*d as two products and one
 *                  subtraction.  A triangle with a non-finite component in f contributes nothing.
 *     SCALE        M = the largest |f_c| over all contributing triangles and components.  M == 0: every normal is (0, 0, 0).  Otherwise
 *                  E = floor(log2 M) (the frexp exponent minus one) and S = 2^(30 - E), so that every |f_c S| < 2^31.
 *     SUM          q = llrint((double)f_c * S), round-half-even (the product is exact); A_i = the sum of q over every corner occurrence of
 *                  vertex i, three int64 per vertex, by 64-bit integer atomic adds: integer addition is associative.  A face whose
 *                  components are all below 2^-31 M (an area 2^31 times smaller than the largest) rounds to zero and VANISHES from the sum.
 *     NORMALISE    in fp64: a = (double)A_i, len = sqrt(ax*ax + ay*ay + az*az) evaluated left to right without contraction, n =
 *                  (float)(a / len); len == 0 (a vertex no triangle uses, faces that cancel) gives (0, 0, 0).
 *   LIMITS: n_v, n_t in 0 .. 2^30.  Device memory for the call: 48 bytes a vertex (position, three int64, normal) and 12 a triangle.
 *   MVS_ERR_ARG, checked in this order before the handle is read: a negative count or a count over the limit; verts NULL with n_v > 0; tris
 *   NULL with n_t > 0; normals NULL with n_v > 0; no engine.  Then, after one validating pass on the device: an index outside 0 .. n_v - 1
 *   (nothing is written in that case).  MVS_ERR_HIP: an allocation or copy failed.  A refused call writes nothing.
 * mvs_engine_mesh_colours: renders and computes agreement exactly as mvs_engine_tsdf does; a pixel is USABLE when it is valid and
 *   popcount(agree) >= c->min_consistent.  For vertex X with normal n (normals == NULL or a zero normal: no facing test, weight 1) the views
 *   v = 0 .. nviews-1 are walked in ascending order:
 *     1. PROJECT  ic = Camera::project(v, (X, 1)) at level L; ic.z > 0; ic lies in mvs_engine_export_ply's sampling window, ic.x >= 0, ic.y
 *                 >= 0, ic.x < W-1, ic.y < H-1; the view has no mask, or its level-L mask is foreground at the nearest pixel
 *                 (floorf(ic.x + 0.5f), floorf(ic.y + 0.5f)) -- the render step's mask rule;
 *     2. FACING   d = C_v - X, w = n.d / sqrtf(d.d) (IEEE division and square root); w >= min_cos;
 *     3. SURFACE  at the nearest pixel.  Usable, with patch q: s = n_q.(X0_q - C_v) / (n_q.(X - C_v)), the tsdf step's expressions (a zero
 *                 or non-finite denominator fails); the view is CONFIRMED when |s - 1| <= occl_tol and skipped otherwise: X is occluded
 *                 behind that view's surface or floats in front of it.  Not usable: the view is UNCONFIRMED;
 *     4. SAMPLE   the bilinear sample of the level-L pyramid at (ic.x, ic.y), mvs_engine_export_ply's expressions in its order;
 *     5. per tier and channel: sw += w, sc += w * sample, and a count.
 *   A NaN fails every comparison above.  The confirmed tier is chosen if its count is > 0, otherwise the unconfirmed tier if its count is
 *   > 0: rgb_c = min(255, (int)floorf(sc / sw + 0.5f)) (0 where that is negative or a NaN, which takes a min_cos <= 0); used = count | 0x80
 *   for the confirmed tier, count for the unconfirmed one (a count is at most 64).  With no view at all rgb = (128, 128, 128), the grey of
 *   PatchManager::writePly for an empty list, and used = 0.  A pool without an alive patch has no surface to hold a vertex against: no
 *   view counts then, every vertex is grey with used = 0 (nothing is rendered).  Device memory for the call: the maps' 17 bytes per pixel of all views and 16
 *   per pixel of the largest, plus 28 bytes a vertex (position, normal, colour, used).
 *   LIMITS: n_v in 0 .. 2^30.
 *   MVS_ERR_ARG, checked in this order before the handle is read: the config checks of mvs_engine_fused_points; m NULL; occl_tol not finite
 *   or <= 0; min_cos not finite or outside [-1, 1]; n_v negative or over the limit; verts or rgb NULL with n_v > 0; no engine; then
 *   min_consistent > nviews - 1.  MVS_ERR_STATE: views not set, or a pass waiting for its commit.  MVS_ERR_HIP: an allocation or copy
 *   failed.  A refused call writes nothing. */
typedef struct mvs_mesh_colouring {
    float occl_tol;  /* surface test: |s - 1| <= occl_tol confirms the view; > 0, finite */
    float min_cos;   /* facing: n . ray >= min_cos; in [-1, 1] */
} mvs_mesh_colouring; /* 8 bytes */
void mvs_default_mesh_colouring(mvs_mesh_colouring* m); /* occl_tol 0.01, min_cos 0.1 */
int mvs_engine_mesh_normals(mvs_engine* e, int64_t n_v, const float* verts, int64_t n_t, const int32_t* tris, float* normals /* [n_v][3] */);
int mvs_engine_mesh_colours(mvs_engine* e, const mvs_maps_config* c, const mvs_mesh_colouring* m, int64_t n_v, const float* verts,
                            const float* normals /* or NULL */, uint8_t* rgb /* [n_v][3] */, uint8_t* used /* [n_v] or NULL */);

/* Mesh clean-up (no reference counterpart): connected components, the removal of small components and unused vertices, and Taubin
 * smoothing of a triangle mesh -- that of mvs_engine_mesh, or any caller's.  verts: n_v x 3 floats, tris: n_t x 3 int32 vertex ids.  The
 * three calls are stateless, only read the engine and need a device but no views, like mvs_engine_extract_mesh; all pointers may be host
 * or device memory (hipMemcpyDefault).  Every result is an integer or comes from an integer sum: it does not depend on the order in which
 * the triangles are listed or in which the hardware meets them, and two calls give the same bytes.  A refused call writes nothing.
 * mvs_engine_mesh_components:
 *     GRAPH         the vertices are 0 .. n_v-1; every triangle joins its three ids.  A triangle with repeated ids joins what it names and
 *                   still counts as a triangle.  Components are those of this graph: two pieces that touch in one vertex are one component.
 *     LABEL         label[i] = the smallest vertex id of i's component (a lock-free union-find in which the smaller id becomes the root,
 *                   then flattened): canonical.  A vertex that no triangle names is its own component.
 *     NTRIS         ntris[i] = the number of triangles of i's component; 0 for an unused vertex.
 *     n_components  the number of components with at least one triangle.
 *   label, ntris and n_components may each be NULL.  LIMITS: n_v, n_t in 0 .. 2^30.  Device memory for the call: 8 bytes a vertex and 12 a
 *   triangle.
 *   MVS_ERR_ARG, checked in this order before the handle is read: a negative count or a count over the limit; tris NULL with n_t > 0; no
 *   engine.  Then, after one validating pass on the device: an id outside 0 .. n_v - 1.  MVS_ERR_HIP: an allocation or copy failed.
 * mvs_engine_mesh_prune:
 *     KEEP          a triangle is kept when its component has ntris >= min_triangles and, with largest_only, is the component with the most
 *                   triangles (among equals the one with the smaller label: a 64-bit maximum over (ntris << 32) | (0xffffffff - label)).
 *     VERTICES      a vertex is kept when a kept triangle names it: min_triangles = 1 already drops the rim vertices of
 *                   mvs_engine_extract_mesh that no triangle uses.
 *     ORDER         kept vertices and kept triangles stay in their input order; the new ids are the exclusive scan of the keep flags.
 *                   Position bytes are copied unchanged; triangle ids are rewritten, their corner order unchanged.
 *     vmap          vmap[i] = the new id of vertex i, or -1; may be NULL.  Where whole components go, the normals of the pruned mesh are
 *                   the kept rows of the normals of the full mesh.
 *   Sizes follow mvs_engine_extract_mesh: with out_verts == NULL, out_tris == NULL or a cap (in vertices / triangles) too small, *n_v_out
 *   and *n_t_out are the exact counts and nothing else is written, vmap neither; MVS_ERR_CAPACITY when a non-NULL output is too small.  An
 *   output that ALIASES an input is not supported.  LIMITS: as above.  Device memory for the call: 16 bytes a vertex and 20 a triangle
 *   (labels, counts, flags and their scans), and with outputs the positions (12 bytes a vertex) and the pruned mesh (12 bytes a kept vertex, 12 a kept triangle).
 *   MVS_ERR_ARG, checked in this order before the handle is read: p NULL; min_triangles < 1; largest_only outside 0/1; a negative count or a
 *   count over the limit; verts NULL with n_v > 0; tris NULL with n_t > 0; n_v_out or n_t_out NULL; a negative cap; no engine.  Then, after
 *   the validating pass: an id outside 0 .. n_v - 1.
 * mvs_engine_mesh_smooth: Taubin lambda|mu smoothing as an ORDER-FREE INTEGER SUM.  An iteration is a STEP with factor lambda, then, when
 *   mu != 0, a STEP with factor mu (mu == 0: plain Laplacian smoothing, which shrinks).  A STEP with factor f on positions x:
 *     TERMS         for every corner occurrence of vertex i in a triangle (i, j, k) the two terms x_j - x_i and x_k - x_i, per component in
 *                   fp32: the other end of an interior edge counts twice, that of a boundary edge once (umbrella weights).  A term with a
 *                   non-finite component contributes nothing and is not counted.
 *     SCALE         M = the largest |component| over all contributing terms of this step.  M == 0: the step leaves every position as it
 *                   is.  Otherwise E = floor(log2 M) and S = 2^(30 - E), as for the normals.
 *     SUM           q = llrint((double)term_c * S), round-half-even; A_i = the int64 sum of q per component, by 64-bit integer atomic adds
 *                   (the two terms of a corner may be added first: integer addition is associative); c_i = the int32 count of contributing
 *                   terms.
 *     UPDATE        in fp64 without contraction: u = ((double)A_i * 2^(E-30)) / (double)c_i, x_i' = (float)((double)x_i + (double)f * u).  A
 *                   vertex with c_i == 0 keeps its bytes.
 *   The positions of a step are read from one buffer and written to another (Jacobi, not in place).  iterations == 0 copies.  Triangles
 *   are never changed, and boundaries are NOT PINNED: the rim of an open mesh shrinks.  out_verts may be verts itself.  The ids are
 *   validated once, before the first step.  LIMITS: as above.  Device memory for the call: 52 bytes a vertex (two position buffers, three
 *   int64, the count) and 12 a triangle.
 *   MVS_ERR_ARG, checked in this order before the handle is read: s NULL; iterations outside 0..1000; lambda not finite or outside (0, 1); mu
 *   not finite or outside (-1, 0]; a negative count or a count over the limit; verts or out_verts NULL with n_v > 0, or tris NULL with
 *   n_t > 0; no engine.  Then: an id outside 0 .. n_v - 1. */
typedef struct mvs_mesh_pruning {
    int64_t min_triangles;   /* keep a component with at least this many triangles; >= 1 */
    int32_t largest_only;    /* 1: keep only the component with most triangles (ties: the smaller label) */
    int32_t pad;
} mvs_mesh_pruning;          /* 16 bytes */
void mvs_default_mesh_pruning(mvs_mesh_pruning* p); /* min_triangles 1, largest_only 0 */
typedef struct mvs_mesh_smoothing {
    int32_t iterations;  /* 0 .. 1000 */
    float lambda;        /* shrinking step, in (0, 1) */
    float mu;            /* inflating step, in (-1, 0]; 0: plain Laplacian, no second step */
    int32_t pad;
} mvs_mesh_smoothing;    /* 16 bytes */
void mvs_default_mesh_smoothing(mvs_mesh_smoothing* s); /* 10, 0.5, -0.53 */
int mvs_engine_mesh_components(mvs_engine* e, int64_t n_v, int64_t n_t, const int32_t* tris, int32_t* label /* [n_v] or NULL */,
                               int32_t* ntris /* [n_v] or NULL */, int64_t* n_components /* or NULL */);
int mvs_engine_mesh_prune(mvs_engine* e, const mvs_mesh_pruning* p, int64_t n_v, const float* verts, int64_t n_t, const int32_t* tris,
                          int64_t cap_v, float* out_verts, int64_t cap_t, int32_t* out_tris, int32_t* vmap /* [n_v] or NULL */,
                          int64_t* n_v_out, int64_t* n_t_out);
int mvs_engine_mesh_smooth(mvs_engine* e, const mvs_mesh_smoothing* s, int64_t n_v, const float* verts, int64_t n_t, const int32_t* tris,
                           float* out_verts /* [n_v][3] */);

/* Mesh decimation (no reference counterpart): VERTEX CLUSTERING (Rossignac-Borrel) on a uniform grid the caller gives -- one output vertex
 * per occupied cell, the triangles that still join three different cells, each set of three cells once.  The marching-tetrahedra mesh has
 * a vertex count set by the voxel, not by the shape; this thins it out on the device.  verts: n_v x 3 floats, tris: n_t x 3 int32 vertex
 * ids.  The call is stateless, only reads the engine and needs a device but no views, like the clean-up calls; all pointers may be host or
 * device memory (hipMemcpyDefault).  Every result is an integer, comes from an integer sum or is a copy of input bytes: two calls give the
 * same bytes, whatever order the hardware meets the triangles in.  A refused call writes nothing.
 * mvs_engine_mesh_decimate:
 *     MEMBERS       vertex i is a member when at least one input triangle names it.  An unused vertex takes no part, and its bytes may be
 *                   anything, a NaN included.
 *     CELL          per component in fp32: g_c = floorf((x_c - origin_c) / cell), IEEE subtraction and division.  Every g_c of a member
 *                   must lie in -2^20 .. 2^20 - 1.  The cell of a member is the triple (g_x, g_y, g_z).
 *     CLUSTER       the members of one cell form one cluster; its representative rep is the smallest member id: canonical.
 *     TRIANGLES     a triangle (a, b, c) becomes (rep(a), rep(b), rep(c)), the corner order kept.  COLLAPSED: a triangle two of whose
 *                   corners fall into one cluster is dropped (a triangle with repeated ids is one).  DUPLICATE: of the surviving
 *                   triangles that name the same unordered set of three clusters only the one with the smallest input index is kept;
 *                   orientation plays no part.  Kept triangles stay in input order.
 *     VERTICES      a cluster becomes an output vertex when a kept triangle names it.  Output vertices are in ascending order of rep; the
 *                   new ids are the exclusive scan of those flags over 0 .. n_v - 1, as in mvs_engine_mesh_prune.
 *     POSITION, placement 0 (the mean), by the scheme of the normals and the smoothing: M = the largest |component| over all members'
 *                   positions, E = floor(log2 M), S = 2^(30 - E); q = llrint((double)x_c * S), round-half-even; A = the int64 sum of q
 *                   over the cluster's members, by 64-bit integer atomic adds; n = the int32 member count; p = (float)(((double)A *
 *                   2^(E-30)) / (double)n) in fp64 without contraction.  A cluster with n == 1 copies its member's bytes: a cell so
 *                   small that nothing merges gives back the input positions.  M == 0: every member is a zero of either sign, all of
 *                   them share one cell whatever the grid, and every triangle collapses.
 *     POSITION, placement 1 (a member): with p the placement-0 position in fp32, for every member d = x - p per component and d2 =
 *                   (dx*dx + dy*dy) + dz*dz in fp32 without contraction; the output is the bytes of the member with the smallest d2, among
 *                   equals the smallest id: one 64-bit unsigned minimum over (bits(d2) << 32) | id.
 *     vmap          vmap[i] = the output id of i's cluster; -1 for an unused vertex and for a member whose cluster no kept triangle names;
 *                   may be NULL.  It lets the caller carry attributes over; the call itself carries none.
 *   WHAT CLUSTERING DOES NOT PROMISE: the result of a closed manifold need not be manifold.  A surface that passes the same three cells
 *   twice (a thin wall, two sheets closer than a cell) leaves, once the duplicate is dropped, edges with one or three triangles; a
 *   cluster may join parts of the surface that were not neighbours.  No target count: the count follows from `cell`.  Whether a result
 *   is still closed, mvs_engine_mesh_boundaries says (below); the small holes that are loops, mvs_engine_mesh_fill closes.
 *   Sizes follow mvs_engine_mesh_prune: with out_verts == NULL, out_tris == NULL or a cap (in vertices / triangles) too small, *n_v_out
 *   and *n_t_out are the exact counts and nothing else is written, vmap neither; MVS_ERR_CAPACITY when a non-NULL output is too small.  An
 *   output that ALIASES an input is not supported.  LIMITS: n_v, n_t in 0 .. 2^30.  Device memory for the call: 36 bytes a vertex (position,
 *   used flag, cell key, representative, flag and scan), 32 a triangle (ids, key, table answer, flag and scan) and ONE TABLE of 12 bytes a
 *   slot with the power of two of slots that is >= 2 max(n_v, n_t) (24 to 48 bytes per vertex or triangle, whichever are more); with
 *   outputs 28 bytes a vertex more (three int64, the count), 8 more for placement 1, and the decimated mesh (12 bytes a kept vertex, 12 a
 *   kept triangle, 4 a vertex for vmap).
 *   MVS_ERR_ARG, checked in this order before the handle is read: d NULL; cell not finite or <= 0; an origin component not finite; placement
 *   outside 0/1; a negative count or a count over the limit; verts NULL with n_v > 0; tris NULL with n_t > 0; n_v_out or n_t_out NULL; a
 *   negative cap; no engine.  Then, after the validating pass on the device: an id outside 0 .. n_v - 1.  Then: a member with a non-finite
 *   component, or with a cell index outside the range.  MVS_ERR_HIP: an allocation or copy failed (or a probe of the table found no slot,
 *   which a correct build never does). */
typedef struct mvs_mesh_decimation {
    float origin[3];   /* a corner of the clustering grid; finite */
    float cell;        /* edge of a grid cell; finite, > 0 */
    int32_t placement; /* 0: the mean of the cell's members; 1: the member nearest to that mean */
    int32_t pad;
} mvs_mesh_decimation; /* 24 bytes */
void mvs_default_mesh_decimation(mvs_mesh_decimation* d); /* origin 0, cell 1, placement 0 */
int mvs_engine_mesh_decimate(mvs_engine* e, const mvs_mesh_decimation* d, int64_t n_v, const float* verts, int64_t n_t, const int32_t* tris,
                             int64_t cap_v, float* out_verts, int64_t cap_t, int32_t* out_tris, int32_t* vmap /* [n_v] or NULL */,
                             int64_t* n_v_out, int64_t* n_t_out);

/* Mesh hole filling (no reference counterpart): the BOUNDARY LOOPS of a triangle mesh and their filling with CENTROID FANS.  The TSDF mesh
 * is open wherever no usable pixel saw the surface; mvs_engine_mesh_boundaries says where and whether a mesh is closed at all, and
 * mvs_engine_mesh_fill closes the holes of up to max_edges edges.  verts: n_v x 3 floats, tris: n_t x 3 int32 vertex ids.  Both calls are
 * stateless, only read the engine and need a device but no views, like the clean-up calls; all pointers may be host or device memory
 * (hipMemcpyDefault).  Every result is an integer, comes from an integer sum or is a copy of input bytes: two calls give the same bytes,
 * whatever order the hardware meets the triangles in.  A refused call writes nothing.
 *     EDGES         a triangle (a, b, c) with three different ids has the directed edges a->b, b->c, c->a.  A triangle with a repeated
 *                   id has no edges here; mvs_engine_mesh_fill copies it through.  cnt(a,b) = the number of triangles with the directed
 *                   edge a->b.  Per unordered pair {a, b} with f = cnt(a,b), r = cnt(b,a): (1,1) is INTERIOR; (1,0) makes a->b a BOUNDARY
 *                   half-edge; anything else (a doubled triangle, a fin) is IRREGULAR: it marks both ends COMPLEX and is not a boundary
 *                   half-edge.
 *     VERTICES      out[v] / in[v] = the boundary half-edges leaving / entering v.  v is ON A BOUNDARY when out + in > 0, and SIMPLE when
 *                   out == 1, in == 1 and it is not complex.
 *     COMPONENTS    the boundary half-edges join their two ends (the union-find of mvs_engine_mesh_components, in which the smaller id
 *                   becomes the root); label = the smallest vertex id of the joined set: canonical.  A component all of whose vertices
 *                   are simple is a LOOP: one directed cycle with as many half-edges as vertices, at least 3.  Any other component is
 *                   COMPLEX; two holes that meet in one vertex are one complex component.
 * mvs_engine_mesh_boundaries:
 *     loop[i]       the label of i's component, -1 for a vertex on no boundary.
 *     length[i]     the number of half-edges of i's component, NEGATED when the component is complex; 0 where loop[i] is -1 (int32: exact
 *                   while a component has fewer than 2^31 half-edges).
 *     n_loops, n_complex   the components of each kind.     n_irregular   the irregular unordered pairs.
 *   Every output may be NULL.  A mesh is a closed edge-manifold exactly when all three counts are 0.  LIMITS: n_v, n_t in 0 .. 2^30.
 *   Device memory for the call: 36 bytes a vertex (parent, out, in, complex, next, two words a root, loop, length), 12 a triangle and ONE
 *   TABLE of 12 bytes a slot with the power of two of slots that is >= 6 n_t, one slot or more per directed edge (72 to 144 bytes a triangle).
 *   MVS_ERR_ARG, checked in this order before the handle is read: a negative count or a count over the limit; tris NULL with n_t > 0; no
 *   engine.  Then, after one validating pass on the device: an id outside 0 .. n_v - 1.
 * mvs_engine_mesh_fill:
 *     FILLED        a loop is filled when 3 <= length <= max_edges.  Complex components and longer loops stay as they are.  The outer rim
 *                   of an open surface is a loop too: max_edges is what keeps it open.  *n_filled = the number of filled loops.
 *     LENGTH 3      the loop a->b->c->a with a its label gets the one triangle (b, a, c).  No vertex is added: a single missing triangle
 *                   is put back.
 *     LENGTH >= 4   one new vertex w at the centroid, and for every half-edge a->b of the loop the triangle (b, a, w).  Every new directed
 *                   edge then has its reverse exactly once: a filled loop disappears from mvs_engine_mesh_boundaries, and nothing else
 *                   about the boundaries changes, not n_irregular, not the labels and lengths of what stays open.
 *     POSITION      by the scheme of the decimation's mean: M = the largest |component| over the vertices of the filled loops of length
 *                   >= 4, E = floor(log2 M), S = 2^(30 - E); q = llrint((double)x_c * S), round-half-even; A = the int64 sum of q over the
 *                   loop's vertices, by 64-bit integer atomic adds; p = (float)(((double)A * 2^(E-30)) / (double)length) in fp64 without
 *                   contraction.  M == 0 gives +0 in all three components.
 *     ORDER         out_verts = the n_v input rows unchanged, unused vertices included, then the new vertices in ascending order of their
 *                   loop's label.  out_tris = the n_t input rows unchanged, then the fill triangles in ascending order of their
 *                   half-edge's origin a (the triangle of a loop of 3 at its label): every simple vertex is the origin of exactly one
 *                   half-edge, so the rows are an exclusive scan over the vertices.  Ids never change: there is no vertex map, and
 *                   attributes of the input carry over row for row.
 *   Sizes follow mvs_engine_mesh_prune: with out_verts == NULL, out_tris == NULL or a cap (in vertices / triangles) too small, *n_v_out,
 *   *n_t_out and *n_filled are the exact counts and nothing else is written; MVS_ERR_CAPACITY when a non-NULL output is too small.  An
 *   output that ALIASES an input is not supported.  LIMITS: n_v, n_t in 0 .. 2^30; *n_v_out or *n_t_out over 2^30 is MVS_ERR_CAPACITY
 *   (nothing written).  Device memory for the call: that of mvs_engine_mesh_boundaries and 28 bytes a vertex more (position, two counts
 *   and their scans); with outputs 24 bytes a vertex more (three int64) and the fans (12 bytes a new vertex, 12 a new triangle).
 *   MVS_ERR_ARG, checked in this order before the handle is read: f NULL; max_edges < 3; a negative count or a count over the limit; verts
 *   NULL with n_v > 0; tris NULL with n_t > 0; n_v_out or n_t_out NULL (n_filled may be NULL); a negative cap; no engine.  Then, after the
 *   validating pass on the device: an id outside 0 .. n_v - 1.  Then: a vertex of a filled loop with a non-finite component
 *   ("loop vertex").  A NaN anywhere else is ignored: on an unused vertex, on an interior vertex, on a loop that is not filled.
 *   MVS_ERR_HIP: an allocation or copy failed (or a probe of the table found no slot, which a correct build never does).
 *   WHAT FILLING DOES NOT DO: no ear clipping or minimal-area triangulation, no refinement of a large fan (a long, bent loop gets a fan
 *   that may fold over itself), nothing for complex components, and the fan is flat until mvs_engine_mesh_smooth relaxes it. */
typedef struct mvs_mesh_filling {
    int32_t max_edges; /* fill the loops of 3 .. max_edges half-edges; >= 3 */
    int32_t pad;
} mvs_mesh_filling; /* 8 bytes */
void mvs_default_mesh_filling(mvs_mesh_filling* f); /* max_edges 64 */
int mvs_engine_mesh_boundaries(mvs_engine* e, int64_t n_v, int64_t n_t, const int32_t* tris, int32_t* loop /* [n_v] or NULL */,
                               int32_t* length /* [n_v] or NULL */, int64_t* n_loops /* or NULL */, int64_t* n_complex /* or NULL */,
                               int64_t* n_irregular /* or NULL */);
int mvs_engine_mesh_fill(mvs_engine* e, const mvs_mesh_filling* f, int64_t n_v, const float* verts, int64_t n_t, const int32_t* tris,
                         int64_t cap_v, float* out_verts, int64_t cap_t, int32_t* out_tris, int64_t* n_v_out, int64_t* n_t_out,
                         int64_t* n_filled /* or NULL */);

/* Mesh render (no reference counterpart): a triangle mesh SEEN FROM THE VIEWS -- per view the z-buffer depth and triangle row of every
 * pixel, per vertex the views that see it, and the colouring call that takes that visibility.  mvs_engine_mesh_colours decides occlusion
 * against the dense maps; after fill, smooth and decimate (or for a caller's own mesh) the maps say nothing where the vertices are, and
 * this is the occlusion test against the mesh itself.  verts: n_v x 3 floats, tris: n_t x 3 int32 vertex ids.  The three calls are
 * stateless and only read the engine; mesh_render and mesh_visibility need views but no pool; all pointers may be host or device memory
 * (hipMemcpyDefault; the array `out` itself is host memory).  Masks play no part in the render: the caller combines them.  Every result is
 * integer arithmetic or an fp64 chain without contraction behind an associative minimum: the same bytes in any triangle order and across
 * two calls.  A refused call writes nothing.
 * Per view v at level L = m_level (W x H = the view's size there):
 *     VERTEX        r0, r1, r2 = the three fp32 fma chains of Camera::project on P_L; inv = the correctly rounded 1 / r2; x = r0 inv,
 *                   y = r1 inv, each clamped to +-2^31 as Camera::project does (a NaN becomes +2^31).  d = r2 is the depth along the optical
 *                   axis under mvs_view_desc's precondition |P[2,:3]| = 1.  sx = llrint((double)x * 256), sy alike: the product is exact,
 *                   the rounding half-to-even.  The vertex is USABLE when d > 0, d is finite and |sx|, |sy| <= 2^24 (a NaN fails).
 *                   screen and vdepth return (sx, sy) -- saturated to int32 where the vertex is not usable -- and d for every vertex.
 *     TRIANGLE      one with an unusable vertex is SKIPPED and counted in n_skipped[v]: THERE IS NO NEAR-PLANE CLIPPING, a triangle that
 *                   crosses the camera plane is not drawn at all.  area = (x1-x0)(y2-y0) - (y1-y0)(x2-x0) in int64; area == 0 covers
 *                   nothing (and is not skipped); area < 0 swaps vertices 1 and 2.  Both faces render: there is no culling.
 *     COVERAGE      the centre of the integer pixel (px, py) inside the image is q = (256 px, 256 py).  For each directed edge a -> b with
 *                   (dx, dy) = b - a: E = dx (qy - ay) - dy (qx - ax), below 2^51 and exact.  The pixel is covered when every E > 0, or
 *                   E == 0 on a top-left edge (dy < 0, or dy == 0 and dx > 0): a pixel on a shared edge belongs to one triangle.
 *     DEPTH         in fp64, left to right, without contraction: w_i = 1.0 / (double)d_i; inv = ((double)E0 w0 + (double)E1 w1 +
 *                   (double)E2 w2) / (double)area with E_i the edge opposite vertex i; depth = (float)(1.0 / inv).  A depth that is
 *                   not finite is not written.
 *     Z-BUFFER      the pixel keeps the smallest 64-bit key (bits(depth) << 32) | t: the nearest depth, and on an exact tie the smallest
 *                   triangle row t.  n_covered[v] = the pixels with a key.
 * mvs_engine_mesh_render: out[v].depth (quiet NaN where no triangle covers the centre) and out[v].tri (-1 there), H x W each; out, either
 * pointer of a view, screen, vdepth, n_covered and n_skipped may be NULL: not wanted.
 * mvs_engine_mesh_visibility: bit v of visible[i] is set when vertex i is usable in view v, its nearest pixel ((sx + 128) >> 8,
 * (sy + 128) >> 8) (arithmetic shift) lies inside the image, and that pixel is empty or (double)d <= (double)z * (1.0 + (double)tol) for
 * its rendered depth z.  Bits at and above nviews are 0.
 * mvs_engine_mesh_colours_visible: mvs_engine_mesh_colours with one more gate -- view v takes part for vertex i only when bit v of
 * visible[i] is set.  With visible == NULL it is mvs_engine_mesh_colours, byte for byte; its checks and errors are that call's.
 * LIMITS: n_v, n_t in 0 .. 2^30.  Device memory for a render or visibility call: 16 bytes a vertex (and the 12 of the input), 12 a triangle
 * plus 4 for the list of the large ones, per pixel of the largest view 8 for the keys and 8 for the two maps; 8 a vertex more for the
 * visibility.  A triangle whose clipped bounding box holds more than 32 pixel centres is rasterised by a wave of its own, in tiles of
 * 8 x 8 pixels: one that spans the image costs that wave W H / 64 steps.  MVS_MRENDER_SMALL=<n> in the environment (read at every call of
 * the render, the visibility and the list counts; n >= 1) puts another number in the place of the 32: a tuning switch of
 * tools/mesh_render_probe.py.  No map, count or visibility bit depends on it.
 * mvs_engine_mesh_render_lists: n_listed[v] = the triangles of view v that went to the wave-per-triangle kernel (usable, area != 0, a
 * clipped box of more than 32 pixel centres), counted by the device as it renders; the maps are not made.  It is how a caller, the tests
 * and the probe see which of the two rasterising kernels a mesh runs on.  Arguments, state and errors as mvs_engine_mesh_render's, and
 * n_listed NULL is MVS_ERR_ARG behind the arrays.
 * MVS_ERR_ARG, checked in this order before the handle is read: (visibility: tol not finite or negative;) a negative count or a count
 * over the limit; verts NULL with n_v > 0; tris NULL with n_t > 0; (visibility: visible NULL with n_v > 0;) no engine.  MVS_ERR_STATE: the
 * views are not set, or a pass is waiting for its commit.  Then MVS_ERR_ARG after one validating pass on the device: an id outside
 * 0 .. n_v - 1.  MVS_ERR_HIP: an allocation or copy failed.
 * WHAT THE RENDER DOES NOT DO: near-plane clipping, back-face culling, masks, interpolation of attributes other than depth, a variant
 * sharded over GPUs.  A texture atlas is not the render's either: mvs_engine_mesh_face_views and mvs_engine_mesh_texture in
 * mvskit_texture.h build one from the render's vertices and this visibility. */
typedef struct mvs_mesh_view_render {
    float* depth; /* H_L*W_L: depth of the nearest triangle at the pixel centre; quiet NaN where none covers it */
    int32_t* tri; /* H_L*W_L: that triangle's row in tris; -1 */
} mvs_mesh_view_render; /* 16 bytes */
int mvs_engine_mesh_render(mvs_engine* e, int64_t n_v, const float* verts, int64_t n_t, const int32_t* tris,
                           mvs_mesh_view_render* out /* [nviews] or NULL; either pointer NULL: not wanted */,
                           int32_t* screen /* [nviews][n_v][2] or NULL */, float* vdepth /* [nviews][n_v] or NULL */,
                           int64_t* n_covered /* [nviews] or NULL */, int64_t* n_skipped /* [nviews] or NULL */);
int mvs_engine_mesh_render_lists(mvs_engine* e, int64_t n_v, const float* verts, int64_t n_t, const int32_t* tris, int64_t* n_listed /* [nviews] */);
int mvs_engine_mesh_visibility(mvs_engine* e, float tol, int64_t n_v, const float* verts, int64_t n_t, const int32_t* tris,
                               uint64_t* visible /* [n_v] */);
int mvs_engine_mesh_colours_visible(mvs_engine* e, const mvs_maps_config* c, const mvs_mesh_colouring* m, int64_t n_v, const float* verts,
                                    const float* normals, const uint64_t* visible /* [n_v] or NULL */, uint8_t* rgb, uint8_t* used);

/* Propagate::run(iter), propagate.cpp:28-64: two colour passes, each = index build + sweep + commit */
int mvs_engine_propagate(mvs_engine* e, int iter, mvs_counters* out);

/* Filter::run (pmmvps/filter.cpp:25-49): filterOutside, filterExact, filterNeighbor(1), filterSmallGroups with the
 * depth-map / m_vimages rebuilds in between; removed4 = patches removed by each of the four.  filterSmallGroups
 * groups by connected components of the symmetrised neighbour relation.
 * With a communicator attached (mvs_engine_comm_init / _attach) the call is collective: every rank runs the per-patch stages
 * on its share of the pool and the ranks exchange what the stages wrote; all ranks end with the same pool and the same counts. */
int mvs_engine_filter(mvs_engine* e, int64_t* removed4);
/* what the last mvs_engine_filter did: HIP-event time of each stage's kernel(s) and the work counts behind the
 * algorithmic-bytes model of DESIGN.md ("Filter::run"). */
typedef struct mvs_filter_stats {
    float outside_ms, exact_ms, neighbor_ms, groups_ms; /* the four filters */
    float rebuild_ms;                                   /* the five setDepthMapsVGridsVPGridsAddPatchV rebuilds together */
    float total_ms;
    int64_t patches_in;          /* alive patches when Filter::run started */
    int64_t exact_patches;       /* alive patches filterExact looked at */
    int64_t exact_view_evals;    /* getTex calls of its setRefImage (588 algorithmic bytes each) */
    int64_t neighbor_patches;    /* alive patches filterNeighbor looked at */
    int64_t neighbor_tasks;      /* (view, cell) lists opened by findNeighbors: 25 cells x m_images, two grids each */
    int64_t neighbor_entries;    /* list entries walked (4-byte ids) */
    int64_t neighbor_visited;    /* distinct patches met: one 48-byte geometry gather each */
    int64_t neighbor_accepted;   /* neighbours handed to filterQuad */
    int64_t neighbor_retried;    /* patches whose neighbourhood did not fit the first launch's id set (second launch, 16384 slots) */
    int64_t exchange_bytes;      /* multi-GPU: bytes this rank received from the others (kill bytes, rewritten records); the work counts
                                  * above then cover this rank's share of the pool only */
} mvs_filter_stats;
int mvs_engine_filter_stats(mvs_engine* e, mvs_filter_stats* out);

/* The same split for view-sharded runs: every rank holds the whole pool, sweeps its own views
 * (view_begin/view_stride) and exchanges what it created before every rank commits the union. */
int mvs_engine_pass(mvs_engine* e, int iter, int pass, mvs_counters* out); /* index build + sweep */
int mvs_engine_export_counts(mvs_engine* e, int64_t* n_new, int64_t* n_kill, int32_t* per_view_new /* [nviews] */);
/* device buffers owned by the caller (e.g. torch tensors): records ordered (view, cell, sequence) */
int mvs_engine_export_device(mvs_engine* e, void* d_new_records, int64_t cap_new, void* d_kill_ids, int64_t cap_kill);
int mvs_engine_commit_device(mvs_engine* e, const void* d_new_records, int64_t n_new, const void* d_kill_ids, int64_t n_kill);
int mvs_engine_commit_local(mvs_engine* e);

/* ---- multi-GPU through the C ABI (no reference counterpart: the reference is one thread on one CPU).
 * One engine per process and GPU; every engine is created with shard_index = rank, shard_count = world, holds the whole
 * pool and all pyramids, and sweeps its contiguous range of the (view, cell) job sequence.  The engines of a job share an
 * RCCL communicator; after each colour pass mvs_engine_exchange all-gathers, on the engine's own stream, (1) five int64 per
 * rank in ONE ncclAllGather -- {new records, evicted ids, this rank's status of the pass, pool headroom, kill-id capacity}: a rank
 * whose pass failed makes every rank give the pass up and return the same status from the same call -- (2) the new records
 * (sizeof(mvs_patch) bytes each), each rank's block broadcast straight into its
 * final place behind the pool (ranges are contiguous, so rank order IS the global (view, cell, creation) order), and
 * (3) the ids of evicted patches -- then commits the union, so all pools stay identical and equal to the 1-GPU result.
 * With a communicator attached, mvs_engine_propagate does pass + exchange itself: PmMvps::run needs no other change.
 * librccl is opened at run time (dlopen); without it these calls return MVS_ERR_STATE and everything else still works.
 * Environment: MVS_CCL_LIBRARY=<path> opens that library instead -- anything exporting ncclGetUniqueId, ncclCommInitRank,
 * ncclCommDestroy, ncclAllGather, ncclBroadcast, ncclGroupStart, ncclGroupEnd, ncclGetErrorString (a site's own RCCL build; the
 * shared-memory loopback of tests/loopback_ccl, with which several ranks can share the one GPU of a test box). */
#define MVS_COMM_ID_BYTES 128
int mvs_comm_unique_id(void* id_out /* MVS_COMM_ID_BYTES */); /* ncclGetUniqueId: rank 0 calls it and hands the bytes to the other ranks (file, socket, MPI ...) */
int mvs_engine_comm_init(mvs_engine* e, const void* id /* MVS_COMM_ID_BYTES */, int rank, int world); /* ncclCommInitRank on the engine's device; collective */
int mvs_engine_comm_attach(mvs_engine* e, void* nccl_comm /* ncclComm_t the host owns */, int rank, int world);
int mvs_engine_comm_release(mvs_engine* e); /* destroys the communicator comm_init made / forgets an attached one */
int mvs_engine_exchange(mvs_engine* e);     /* after mvs_engine_pass: all-gather + commit of the union; collective */
/* rank / world the engine was given (world 0: no communicator) and what the communicator itself reports (ncclCommCount,
 * ncclCommUserRank; -1 where the collective library does not export them) -- for a launcher that wants to see that N ranks really
 * share one communicator (bench.py --gpus N prints it as `rccl_world`) */
int mvs_engine_comm_info(mvs_engine* e, int* rank, int* world, int* comm_count, int* comm_rank);
/* FAILURES in a multi-rank job.  A failure on one rank (its pass overflowed, an allocation did not fit, a HIP error) reaches every
 * rank: mvs_engine_exchange's first all-gather and the agreement in front of every collective of mvs_engine_filter carry a status
 * word, all ranks give the call up together and return the same status; nobody waits.  Two things cannot be agreed on: no device
 * memory for the status word itself, and a failure of the collective library -- the rank returns MVS_ERR_HIP alone and the job
 * must be torn down by its launcher (torch.distributed.run and bench.py --gpus N both end the job when a rank exits non-zero).
 * After an error from mvs_engine_filter the stages that completed stand on every rank alike; the stage that was under way may
 * have rewritten lists of this rank's share only: re-upload the patches or stop. */

/* parity artefact: kind 0 = m_dpgrids patch, kind 1 = best-NCC patch of
 * m_pgrids[view][cell] whose reference view is `view`.  depth[gw*gh] = oaxis.coord, normal[gw*gh*3],
 * ids[gw*gh]; empty cells are NaN / -1.  Host buffers. */
int mvs_engine_depth_normal_map(mvs_engine* e, int view, int kind, float* depth, float* normal, int32_t* ids);

/* Batched single functions of the path, for parity tests and kernel benchmarks.
 * op: see mvs_probe_op.  in/out are host arrays of n records / values. */
typedef enum mvs_probe_op {
    MVS_PROBE_NCC = 0,        /* PatchManager::computeNcc      -> out_f[n] */
    MVS_PROBE_PREPROCESS = 1, /* Optim::preProcess             -> out_rec[n], out_i[n] = flag */
    MVS_PROBE_REFINE = 2,     /* Optim::refinePatch            -> out_rec[n]; key = (0,0,i,0); with the engine's refiner */
    MVS_PROBE_POSTPROCESS = 3,/* Optim::postProcess            -> out_rec[n], out_i[n] = flag */
    MVS_PROBE_COST = 4,       /* Optim::cost_func at encode(p) -> out_f[n] */
    MVS_PROBE_MATH = 5,       /* in_f[n] -> out_f[5n]: sin, cos, asin, acos, atan of each input */
    MVS_PROBE_REFINE_X = 6    /* Optim::refinePatch (optim.cpp:480-547) with the CONVERGED refiner (MVS_ERR_STATE under HALVING) -> out_rec[n]
                               * as MVS_PROBE_REFINE; out_f[4n] = the final (x0, x1, x2) -- the best vertex, in the input's encode frame --
                               * and the cost there; out_i[n] = cost evaluations used, negated when the budget ran out (out_rec[i] is
                               * then the input) */
} mvs_probe_op;
int mvs_engine_probe(mvs_engine* e, int op, int64_t n, const mvs_patch* in_rec, const float* in_f,
                     mvs_patch* out_rec, float* out_f, int32_t* out_i);

/* timing of the last mvs_engine_pass / mvs_engine_propagate, measured with HIP events on the engine's stream */
typedef struct mvs_timing {
    float index_ms;  /* index build (CSR, trim, depth maps) */
    float sweep_ms;  /* the sweep kernel(s) */
    float commit_ms; /* commit */
    int32_t sweep_launches;
    float exchange_ms;      /* mvs_engine_exchange: count all-gather + record / kill-id broadcasts (HIP events) */
    int32_t sweep_jobs_listed; /* destination cells the sweep's waves were handed: the jobs of this rank's range with a source entry that
                                * starts a trial (in the four bytes that were padding: the struct's size and the other offsets stand) */
    int64_t exchange_bytes; /* bytes this rank received in them */
    int64_t check_retried_cells; /* destination cells whose Optim::check met more patches than the wave's LDS id set holds and that ran
                                  * again on the second tier (a 16384-slot set in global memory); normally 0 */
} mvs_timing;
int mvs_engine_last_timing(mvs_engine* e, mvs_timing* t);

/* How the sweep refined its trials, summed over every pass since the engine was created.  A trial is a candidate that reached
 * Optim::refinePatch.  Two consecutive trials of a destination cell are refined together (one pass of the per-view arithmetic for both)
 * when the second is certain to find room in the cell and both lists have at most 8 views under tau; results do not depend on it.
 *   out[0] trials refined as one of a pair
 *   out[1] alone: no trial was left in the cell to join it       out[2] alone: the cell had no guaranteed room for a second one
 *   out[3] alone: the trial that would have joined it failed generatePatch / preProcess
 *   out[4] alone: one of the two lists was longer than 8 views
 *   out[5] trials that can pair, whether or not they did (MVS_SWEEP_PAIR=0 in the environment, or the CONVERGED refiner, refines every
 *          trial alone: out[0] is then 0 and out[5] says what would pair); out[1] + ... + out[5] = all trials */
int mvs_engine_sweep_pairs(mvs_engine* e, int64_t out[6]);

/* Trials of the sweep that reused what the trial before them had computed, summed over every pass since the engine was created.  A trial
 * into a FULL cell (the replace-worst branch) draws nothing before Optim::refinePatch: generatePatch, the pre-filter and preProcess
 * depend on the source patch, the cell's worst patch and the index alone, so while nothing is staged the next trial of the same source
 * entry would compute the same again.  Such trials are counted in every work counter (evals and view_evals included) as if they had run.
 *   out[0] trials skipped because the trial before them ended before the refinement (generatePatch failed, pre-filtered, preProcess
 *          failed): they end the same way
 *   out[1] trials that took the candidate the trial before them had brought through preProcess and went straight to their own
 *          refinement (always 0: this engine runs those trials in full) */
int mvs_engine_sweep_repeats(mvs_engine* e, int64_t out[2]);

/* Sweep launches by kernel, summed over every pass since the engine was created.  A window whose samples fill all three slots of every
 * class lane and leave one extra (3 x 16 + 1 samples: wsize 7) runs on an instantiation of the sweep without the slot-mask arithmetic;
 * results do not depend on it.  MVS_SWEEP_FULLWINDOW=0 in the environment (read at every launch) keeps such a window on the generic
 * kernel.  The CONVERGED refiner and the second tier of Optim::check always run generic kernels (the latter is not counted here).
 *   out[0] launches of a generic kernel      out[1] launches of the full-window kernel */
int mvs_engine_sweep_kernels(mvs_engine* e, int64_t out[2]);

/* Launches by the form of their texture samplers, since the engine was created.  The RGBA8 pyramids of all views lie in one device
 * allocation.  While it is below 4 GiB the full-window sweep kernel and the refine probe (mvs_engine_probe, MVS_PROBE_REFINE with the
 * default refiner) address a texel by the allocation's base, one value for the whole launch, plus a 32-bit byte offset per lane (the
 * narrow form); otherwise, and in every other kernel, by a 64-bit address per lane (the wide form).  The texels read are the same and
 * so are the results.  MVS_SAMPLER_WIDE=1 in the environment (read at every launch) keeps the wide form.
 *   out[0] sweep launches with wide samplers      out[1] sweep launches with narrow samplers
 *   out[2] refine probes with wide samplers       out[3] refine probes with narrow samplers */
int mvs_engine_sampler_launches(mvs_engine* e, int64_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* MVSKIT_ENGINE_H */
