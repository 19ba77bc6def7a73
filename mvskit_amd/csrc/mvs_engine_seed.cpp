// mvs_engine_seed.cpp -- the seeding front ends of the C ABI in include/mvskit_engine.h: seed patches from points and per-view normal
// maps (mvs_seed.hip), the cold start from random plane hypotheses (mvs_seed_random.hip), the warm start from a sparse point cloud
// (mvs_seed_points.hip) with its depth ranges, and the staged append that the last two share.
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "mvs_engine_impl.h"

using namespace mvseng;

namespace {

// xyz streams through a device buffer of `chunk` points: per chunk fn(first, n, d_xyz) with points [first, first + n) of the call in d_xyz.
// The next chunk overwrites the buffer in stream order.
template <typename Fn> int for_point_chunks(mvs_engine* e, const float* xyz, int64_t npoints, int64_t chunk, Fn&& fn) {
    DevBuf<float> d_xyz;
    if (d_xyz.ensure(3 * chunk)) return MVS_ERR_HIP;
    for (int64_t first = 0; first < npoints; first += chunk) {
        const int64_t n = std::min(chunk, npoints - first);
        HIPCHK(hipMemcpyAsync(d_xyz.p, xyz + 3 * first, sizeof(float) * 3 * (size_t)n, hipMemcpyHostToDevice, e->stream));
        if (int r = fn(first, n, (const float*)d_xyz.p)) return r;
    }
    return MVS_OK;
}

// what the launches of both seeding front ends share: min_ncc < 0 asks for nccThresholdBefore; the engine's refiner
SeedChainArgs seed_chain_args(const mvs_engine* e, int hypotheses, float min_ncc) {
    const RefineSel rs = refine_sel(e);
    return SeedChainArgs{hypotheses, min_ncc < 0.0f ? e->prm.nccThresholdBefore : min_ncc, rs.simplex, rs.max_evals, rs.xtol};
}

// The staged append of the seeding front ends (mvs_engine_seed_random: a batch is a view's cells; mvs_engine_seed_points: a chunk's
// points).  A launch stages the patch of job j, if it gives one, at stage[j] with keep[j] = 1; the keep flags are scanned and the kept
// records gathered behind those of the batches before -- into pool_alt, the commit's compaction target, which holds nothing between
// calls: the pool itself is written once, after the last batch, when the count is known to fit.
struct StagedAppend {
    mvs_engine* e;
    const char* who;
    DevBuf<DPatch> stage;
    DevBuf<int32_t> keep, base, scan;
    int64_t total = 0, room;
    StagedAppend(mvs_engine* e, const char* who) : e(e), who(who), room(e->pool.cap - e->pool_n) {}
    // the buffers for batches of up to max_jobs jobs, and what postProcess reads
    int begin(int64_t max_jobs) {
        if (stage.ensure(max_jobs) || keep.ensure(max_jobs + 1) || base.ensure(max_jobs + 1) || scan.ensure(max_jobs / 256 + 4096)) return MVS_ERR_HIP;
        // setVImagesVGrids reads m_dpgrids when depth > 0 (what MVS_PROBE_POSTPROCESS prepares): from the pool as it is now
        if (e->prm.depth > 0) if (int r = build_depth(e)) return r;
        return MVS_OK;
    }
    // one batch of n jobs: launch(stage, keep) starts its waves
    template <typename Launch> int batch(int64_t n, Launch&& launch) {
        HIPCHK(hipMemsetAsync(keep.p, 0, sizeof(int32_t) * ((size_t)n + 1), e->stream));
        launch(stage.p, keep.p);
        int64_t kept = 0;
        if (int r = scan_total(e, keep.p, base.p, scan.p, n, &kept)) return r;
        if (total + kept > room) { g_err = std::string(who) + ": patch pool capacity exceeded (raise mvs_config.max_patches)"; return MVS_ERR_CAPACITY; }
        mvsk_seed_gather(stage.p, keep.p, base.p, (int)n, e->pool_alt.p + total, (int32_t)(e->pool_n + total), e->stream);
        total += kept;
        return MVS_OK;
    }
    // the gathered records into the pool
    int commit(int64_t* n_added) {
        if (total > 0) {
            HIPCHK(hipMemcpyAsync(e->pool.p + e->pool_n, e->pool_alt.p, sizeof(DPatch) * (size_t)total, hipMemcpyDeviceToDevice, e->stream));
            HIPCHK(hipStreamSynchronize(e->stream));
            HIPCHK(hipGetLastError());
            e->pool_n += total;
        }
        if (n_added) *n_added = total;
        return MVS_OK;
    }
};

}  // namespace

extern "C" {

// DepthNormInit::createPatches with isTest = 0 (depth_normal_init.cpp:34-91) on the device: mvs_seed.hip.  The views stream one at a
// time through one map and one mask buffer (13 bytes per pixel of the largest view), so the float sum of a point's normals runs in the
// reference's order (image 0, 1, 2 ...) and the memory does not grow with the view count; per point 44 bytes (coordinates, sum,
// membership word, keep flag and its scan).  All of it is released on return.  The pool is written only after the count is known to fit.
namespace {
// The camera constants Optim::sortImages reads, as the host mirror's DepthNormInit derives them from the level-0 projection (Camera::
// getCameraCenter, camera.cpp:295-308; Optim::setAxesScales, optim.cpp:43-65): plain products and sums, each element of the inverse
// divided by the determinant before the sum.  DView::center / ipscale hold the same quantities in the sweep's fmaf-chain arithmetic,
// which can differ in the last bit; a seed record is to have the bits of the mirror's.
SeedCam seed_camera(const float* P) {
    SeedCam c;
    const double m[9] = {P[0], P[1], P[2], P[4], P[5], P[6], P[8], P[9], P[10]};
    const double det = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
    const double inv[9] = {(m[4] * m[8] - m[5] * m[7]) / det, (m[2] * m[7] - m[1] * m[8]) / det, (m[1] * m[5] - m[2] * m[4]) / det,
                           (m[5] * m[6] - m[3] * m[8]) / det, (m[0] * m[8] - m[2] * m[6]) / det, (m[2] * m[3] - m[0] * m[5]) / det,
                           (m[3] * m[7] - m[4] * m[6]) / det, (m[1] * m[6] - m[0] * m[7]) / det, (m[0] * m[4] - m[1] * m[3]) / det};
    const double q[3] = {P[3], P[7], P[11]};
    for (int r = 0; r < 3; ++r) c.center[r] = (float)-(inv[3 * r] * q[0] + inv[3 * r + 1] * q[1] + inv[3 * r + 2] * q[2]);
    c.center[3] = 1.0f;
    const float on = sqrtf(P[8] * P[8] + P[9] * P[9] + P[10] * P[10]);
    const float z[3] = {P[8] / on, P[9] / on, P[10] / on};
    float x[3] = {P[0], P[1], P[2]};
    float y[3] = {z[1] * x[2] - z[2] * x[1], z[2] * x[0] - z[0] * x[2], z[0] * x[1] - z[1] * x[0]};
    const float yn = sqrtf(y[0] * y[0] + y[1] * y[1] + y[2] * y[2]);
    for (int k = 0; k < 3; ++k) y[k] /= yn;
    x[0] = y[1] * z[2] - y[2] * z[1]; x[1] = y[2] * z[0] - y[0] * z[2]; x[2] = y[0] * z[1] - y[1] * z[0];
    c.ipscale = (P[0] * x[0] + P[1] * x[1] + P[2] * x[2]) + (P[4] * y[0] + P[5] * y[1] + P[6] * y[2]);
    return c;
}
}  // namespace

int mvs_engine_seed_patches(mvs_engine* e, int64_t npoints, const float* xyz, const mvs_seed_view* views, int64_t* n_added) {
    // the arguments first, the handle after them
    if (npoints < 0 || (npoints > 0 && !xyz) || !views) { g_err = "mvs_engine_seed_patches: negative npoints, or xyz / views null"; return MVS_ERR_ARG; }
    if (npoints > (int64_t)INT32_MAX - 4096) { g_err = "mvs_engine_seed_patches: more than 2^31 - 4097 points in one call"; return MVS_ERR_ARG; }
    if (int r = need_state(e, NEED_IDLE, "mvs_engine_seed_patches")) return r;
    if (n_added) *n_added = 0;
    if (npoints == 0) return MVS_OK;
    HIPCHK(hipSetDevice(e->cfg.device));
    Range rg("mvs:seed_patches");
    hipStream_t st = e->stream;
    const int nviews = e->cfg.nviews;
    const int64_t n = npoints;
    int64_t max_pix = 0;
    for (int v = 0; v < nviews; ++v)
        if (views[v].normals && views[v].mask) max_pix = std::max(max_pix, (int64_t)e->hviews[v].W[0] * e->hviews[v].H[0]);
    DevBuf<float> d_xyz, d_sum, d_map;
    DevBuf<unsigned long long> d_bits;
    DevBuf<int32_t> d_keep, d_base, d_scan;
    DevBuf<uint8_t> d_mask;
    DevBuf<SeedCam> d_cams;
    if (d_xyz.ensure(3 * n) || d_sum.ensure(3 * n) || d_bits.ensure(n) || d_keep.ensure(n + 1) || d_base.ensure(n + 1) || d_scan.ensure(n / 256 + 4096) ||
        d_cams.ensure(nviews) || (max_pix > 0 && (d_map.ensure(3 * max_pix) || d_mask.ensure(max_pix))))
        return MVS_ERR_HIP;
    std::vector<SeedCam> cams((size_t)nviews);
    for (int v = 0; v < nviews; ++v) cams[(size_t)v] = seed_camera(e->hviews[v].P[0]);
    HIPCHK(hipMemcpyAsync(d_cams.p, cams.data(), sizeof(SeedCam) * (size_t)nviews, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_xyz.p, xyz, sizeof(float) * 3 * (size_t)n, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d_sum.p, 0, sizeof(float) * 3 * (size_t)n, st));
    HIPCHK(hipMemsetAsync(d_bits.p, 0, sizeof(unsigned long long) * (size_t)n, st));
    for (int v = 0; v < nviews; ++v) {
        // a view without a mask is skipped (PhotoSet::getMask = -1); one without a map has nothing to add
        if (!views[v].normals || !views[v].mask) continue;
        const DView& vw = e->hviews[v];
        const size_t pix = (size_t)vw.W[0] * vw.H[0];
        SeedView sv;
        memcpy(sv.P, vw.P[0], sizeof sv.P);
        sv.W = vw.W[0]; sv.H = vw.H[0]; sv.view = v;
        HIPCHK(hipMemcpyAsync(d_map.p, views[v].normals, sizeof(float) * 3 * pix, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_mask.p, views[v].mask, pix, hipMemcpyHostToDevice, st));
        mvsk_seed_accumulate(sv, d_map.p, d_mask.p, d_xyz.p, n, d_sum.p, d_bits.p, st);
        HIPCHK(hipStreamSynchronize(st));  // the two buffers are reused by the next view
    }
    mvsk_seed_flags(d_cams.p, e->cfg.level, d_xyz.p, d_sum.p, d_bits.p, n, d_keep.p, st);
    int64_t total = 0;
    if (int r = scan_total(e, d_keep.p, d_base.p, d_scan.p, n, &total)) return r;
    if (e->pool_n + total > e->pool.cap) { g_err = "mvs_engine_seed_patches: patch pool capacity exceeded (raise mvs_config.max_patches)"; return MVS_ERR_CAPACITY; }
    if (total > 0) {
        // Optim::sortImages' threshold as the mirror writes it (optim.cpp:222), in float; Patch::m_ncc = -1 in mvs_engine_upload_patches' score2
        volatile float deg10 = 10.0f * (float)M_PI / 180.0f;
        const float thr = 1.0f - cosf(deg10);
        const float tmp_unit = std::max(0.0f, -1.0f - e->prm.nccThreshold);
        mvsk_seed_emit(d_cams.p, nviews, e->cfg.level, thr, tmp_unit, d_xyz.p, d_sum.p, d_bits.p, d_keep.p, d_base.p, n, e->pool.p + e->pool_n, st);
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipGetLastError());
        e->pool_n += total;
        e->ncc_dirty = true;
    }
    if (n_added) *n_added = total;
    return MVS_OK;
}

// The cold start (mvs_seed_random.hip): per view one launch of a wave per cell, a batch of the staged append (StagedAppend) with a staging
// buffer of one record per cell of the largest view.
namespace {
// the checks of both entry points that need no handle, in the header's order
int seed_random_args(const mvs_seed_random* s, const char* who) {
    if (!s) { g_err = std::string(who) + ": parameters null"; return MVS_ERR_ARG; }
    if (s->hypotheses < 1 || s->hypotheses > 64) { g_err = std::string(who) + ": hypotheses outside 1..64"; return MVS_ERR_ARG; }
    if (!s->depth_min || !s->depth_max) { g_err = std::string(who) + ": depth range null"; return MVS_ERR_ARG; }
    volatile double third = M_PI / 3.0;
    if (!(s->max_tilt > 0.0f) || !(s->max_tilt <= (float)third)) { g_err = std::string(who) + ": max_tilt not in (0, pi/3]"; return MVS_ERR_ARG; }
    return MVS_OK;
}
int seed_random_ranges(const mvs_engine* e, const mvs_seed_random* s, const char* who) {
    for (int v = 0; v < e->cfg.nviews; ++v) {
        const float lo = s->depth_min[v], hi = s->depth_max[v];
        if (!std::isfinite(lo) || !std::isfinite(hi) || !(0.0f < lo) || !(lo < hi)) {
            g_err = std::string(who) + ": depth range of view " + std::to_string(v) + " not finite or not 0 < min < max";
            return MVS_ERR_ARG;
        }
    }
    return MVS_OK;
}
SeedRandomArgs seed_random_launch(const mvs_engine* e, const mvs_seed_random* s, int view) {
    return SeedRandomArgs{seed_chain_args(e, s->hypotheses, s->min_ncc), s->seed, s->max_tilt, view, s->depth_min[view], s->depth_max[view]};
}
}  // namespace

void mvs_default_seed_random(mvs_seed_random* s) {
    if (!s) return;
    volatile double third = M_PI / 3.0;
    s->hypotheses = 8; s->seed = 1; s->max_tilt = (float)third; s->min_ncc = -1.0f; s->depth_min = nullptr; s->depth_max = nullptr;
}

int mvs_engine_seed_random(mvs_engine* e, const mvs_seed_random* s, int64_t* n_added) {
    const char* who = "mvs_engine_seed_random";
    if (int r = seed_random_args(s, who)) return r;
    if (int r = need_state(e, NEED_ENGINE, who)) return r;
    if (int r = seed_random_ranges(e, s, who)) return r;
    if (int r = need_state(e, NEED_IDLE, who)) return r;
    if (n_added) *n_added = 0;
    HIPCHK(hipSetDevice(e->cfg.device));
    Range rg("mvs:seed_random");
    const int nviews = e->cfg.nviews;
    int64_t max_cells = 0;
    for (int v = 0; v < nviews; ++v) max_cells = std::max(max_cells, (int64_t)e->hviews[v].gw * e->hviews[v].gh);
    StagedAppend sa(e, who);
    if (int r = sa.begin(max_cells)) return r;
    const DParams p = current_params(e);
    for (int v = 0; v < nviews; ++v) {
        const int n = e->hviews[v].gw * e->hviews[v].gh;
        if (int r = sa.batch(n, [&](DPatch* stage, int32_t* keep) { mvsk_seed_random(p, seed_random_launch(e, s, v), n, stage, keep, e->stream); })) return r;
    }
    return sa.commit(n_added);
}

int mvs_engine_seed_random_hypotheses(mvs_engine* e, const mvs_seed_random* s, int view, int64_t ncells, const int32_t* cells, mvs_patch* out) {
    const char* who = "mvs_engine_seed_random_hypotheses";
    if (int r = seed_random_args(s, who)) return r;
    if (ncells < 0 || (ncells > 0 && (!cells || !out))) { g_err = std::string(who) + ": negative ncells, or cells / out null"; return MVS_ERR_ARG; }
    if (ncells > (int64_t)INT32_MAX / 64) { g_err = std::string(who) + ": more than 2^25 cells in one call"; return MVS_ERR_ARG; }
    if (int r = need_state(e, NEED_ENGINE, who)) return r;
    if (view < 0 || view >= e->cfg.nviews) { g_err = std::string(who) + ": no such view"; return MVS_ERR_ARG; }
    if (int r = seed_random_ranges(e, s, who)) return r;
    if (int r = need_state(e, NEED_VIEWS, who)) return r;
    const int grid = e->hviews[view].gw * e->hviews[view].gh;
    for (int64_t i = 0; i < ncells; ++i)
        if (cells[i] < 0 || cells[i] >= grid) { g_err = std::string(who) + ": a cell outside the view's grid"; return MVS_ERR_ARG; }
    if (ncells == 0) return MVS_OK;
    HIPCHK(hipSetDevice(e->cfg.device));
    hipStream_t st = e->stream;
    const int64_t nrec = ncells * s->hypotheses;
    DevBuf<DPatch> d_out;
    DevBuf<int32_t> d_cells;
    if (d_out.ensure(nrec) || d_cells.ensure(ncells)) return MVS_ERR_HIP;
    HIPCHK(hipMemcpyAsync(d_cells.p, cells, sizeof(int32_t) * (size_t)ncells, hipMemcpyHostToDevice, st));
    mvsk_seed_random_hypotheses(current_params(e), seed_random_launch(e, s, view), ncells, d_cells.p, d_out.p, st);
    HIPCHK(hipMemcpyAsync(out, d_out.p, sizeof(mvs_patch) * (size_t)nrec, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    return MVS_OK;
}

// The warm start (mvs_seed_points.hip): the points stream in chunks through fixed buffers (for_point_chunks) -- per point of a chunk its
// coordinates, one staged record, the keep flag and its scan -- one launch of a wave per point, a batch of the staged append.
namespace {
constexpr int64_t SEED_POINTS_CHUNK = 1 << 18, SEED_POINTS_CHUNK_MAX = 1 << 22;
int64_t seed_points_chunk() {  // MVS_SEED_POINTS_CHUNK, read at the call: a positive integer (anything else: the default)
    const char* s = getenv("MVS_SEED_POINTS_CHUNK");
    if (!s || !*s) return SEED_POINTS_CHUNK;
    char* end = nullptr;
    const long long v = strtoll(s, &end, 10);
    if (*end || v <= 0) return SEED_POINTS_CHUNK;
    return std::min<int64_t>(v, SEED_POINTS_CHUNK_MAX);
}
// the checks that need no handle, in the header's order
int seed_points_args(const mvs_seed_points* s, int64_t npoints, const float* xyz, const char* who) {
    if (!s) { g_err = std::string(who) + ": parameters null"; return MVS_ERR_ARG; }
    if (s->hypotheses < 1 || s->hypotheses > 64) { g_err = std::string(who) + ": hypotheses outside 1..64"; return MVS_ERR_ARG; }
    if (npoints < 0) { g_err = std::string(who) + ": negative npoints"; return MVS_ERR_ARG; }
    if (npoints > 0 && !xyz) { g_err = std::string(who) + ": xyz null"; return MVS_ERR_ARG; }
    return MVS_OK;
}
}  // namespace

void mvs_default_seed_points(mvs_seed_points* s) {
    if (!s) return;
    s->hypotheses = 4; s->min_ncc = -1.0f;
}

int mvs_engine_seed_points(mvs_engine* e, const mvs_seed_points* s, int64_t npoints, const float* xyz, int64_t* n_added) {
    const char* who = "mvs_engine_seed_points";
    if (int r = seed_points_args(s, npoints, xyz, who)) return r;
    if (int r = need_state(e, NEED_ENGINE, who)) return r;
    if (npoints > ((int64_t)1 << 30)) { g_err = std::string(who) + ": more than 2^30 points in one call"; return MVS_ERR_ARG; }
    if (int r = need_state(e, NEED_IDLE, who)) return r;
    if (n_added) *n_added = 0;
    if (npoints == 0) return MVS_OK;
    HIPCHK(hipSetDevice(e->cfg.device));
    Range rg("mvs:seed_points");
    const int64_t chunk = std::min(seed_points_chunk(), npoints);
    StagedAppend sa(e, who);
    if (int r = sa.begin(chunk)) return r;
    const DParams p = current_params(e);
    SeedPointsArgs a{seed_chain_args(e, s->hypotheses, s->min_ncc), 0, 0};
    if (int r = for_point_chunks(e, xyz, npoints, chunk, [&](int64_t first, int64_t n, const float* d_xyz) {
            a.first = first; a.n = (int32_t)n;
            return sa.batch(n, [&](DPatch* stage, int32_t* keep) { mvsk_seed_points(p, a, d_xyz, stage, keep, e->stream); });
        }))
        return r;
    return sa.commit(n_added);
}

int mvs_engine_seed_points_hypotheses(mvs_engine* e, const mvs_seed_points* s, int64_t npoints, const float* xyz, mvs_patch* out, int32_t* count) {
    const char* who = "mvs_engine_seed_points_hypotheses";
    if (int r = seed_points_args(s, npoints, xyz, who)) return r;
    if (npoints > 0 && (!out || !count)) { g_err = std::string(who) + ": out or count null"; return MVS_ERR_ARG; }
    if (int r = need_state(e, NEED_ENGINE, who)) return r;
    if (npoints * s->hypotheses > (int64_t)INT32_MAX) { g_err = std::string(who) + ": more than 2^31 - 1 hypotheses in one call"; return MVS_ERR_ARG; }
    if (int r = need_state(e, NEED_VIEWS, who)) return r;
    if (npoints == 0) return MVS_OK;
    HIPCHK(hipSetDevice(e->cfg.device));
    hipStream_t st = e->stream;
    const int K = s->hypotheses;
    const int64_t chunk = std::min(std::max<int64_t>(seed_points_chunk() / K, 1), npoints);  // at most a chunk of records at a time
    DevBuf<DPatch> d_out;
    DevBuf<int32_t> d_count;
    if (d_out.ensure(chunk * K) || d_count.ensure(chunk)) return MVS_ERR_HIP;
    const DParams p = current_params(e);
    return for_point_chunks(e, xyz, npoints, chunk, [&](int64_t first, int64_t n, const float* d_xyz) -> int {
        mvsk_seed_points_hypotheses(p, K, n, d_xyz, d_out.p, d_count.p, st);
        HIPCHK(hipMemcpyAsync(out + first * K, d_out.p, sizeof(mvs_patch) * (size_t)(n * K), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(count + first, d_count.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));  // the buffers are reused by the next chunk
        HIPCHK(hipGetLastError());
        return MVS_OK;
    });
}

int mvs_engine_depth_ranges(mvs_engine* e, int64_t npoints, const float* xyz, float margin, float* depth_min, float* depth_max, int64_t* count) {
    const char* who = "mvs_engine_depth_ranges";
    if (npoints < 0) { g_err = std::string(who) + ": negative npoints"; return MVS_ERR_ARG; }
    if (npoints > 0 && !xyz) { g_err = std::string(who) + ": xyz null"; return MVS_ERR_ARG; }
    if (!depth_min || !depth_max || !count) { g_err = std::string(who) + ": depth_min, depth_max or count null"; return MVS_ERR_ARG; }
    if (!std::isfinite(margin) || !(margin >= 0.0f)) { g_err = std::string(who) + ": margin not finite or < 0"; return MVS_ERR_ARG; }
    if (int r = need_state(e, NEED_ENGINE, who)) return r;
    if (npoints > ((int64_t)1 << 30)) { g_err = std::string(who) + ": more than 2^30 points in one call"; return MVS_ERR_ARG; }
    if (int r = need_state(e, NEED_VIEWS, who)) return r;
    const int nviews = e->cfg.nviews;
    std::vector<uint32_t> lo((size_t)nviews, 0xffffffffu), hi((size_t)nviews, 0u);
    std::vector<unsigned long long> cnt((size_t)nviews, 0ull);
    if (npoints > 0) {
        HIPCHK(hipSetDevice(e->cfg.device));
        hipStream_t st = e->stream;
        DevBuf<uint32_t> d_lohi;
        DevBuf<unsigned long long> d_cnt;
        if (d_lohi.ensure(2 * nviews) || d_cnt.ensure(nviews)) return MVS_ERR_HIP;
        HIPCHK(hipMemsetAsync(d_lohi.p, 0xff, sizeof(uint32_t) * (size_t)nviews, st));
        HIPCHK(hipMemsetAsync(d_lohi.p + nviews, 0, sizeof(uint32_t) * (size_t)nviews, st));
        HIPCHK(hipMemsetAsync(d_cnt.p, 0, sizeof(unsigned long long) * (size_t)nviews, st));
        const DParams p = current_params(e);
        if (int r = for_point_chunks(e, xyz, npoints, std::min(seed_points_chunk(), npoints), [&](int64_t, int64_t n, const float* d_xyz) -> int {
                mvsk_depth_ranges(p, n, d_xyz, d_lohi.p, d_lohi.p + nviews, d_cnt.p, st);
                HIPCHK(hipStreamSynchronize(st));  // the buffer is reused by the next chunk
                return MVS_OK;
            }))
            return r;
        HIPCHK(hipMemcpyAsync(lo.data(), d_lohi.p, sizeof(uint32_t) * (size_t)nviews, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(hi.data(), d_lohi.p + nviews, sizeof(uint32_t) * (size_t)nviews, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(cnt.data(), d_cnt.p, sizeof(unsigned long long) * (size_t)nviews, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipGetLastError());
    }
    const float widen = 1.0f + margin;
    for (int v = 0; v < nviews; ++v) {
        count[v] = (int64_t)cnt[(size_t)v];
        depth_min[v] = depth_max[v] = 0.0f;
        if (cnt[(size_t)v] == 0) continue;
        float a, b;
        memcpy(&a, &lo[(size_t)v], 4); memcpy(&b, &hi[(size_t)v], 4);
        depth_min[v] = a / widen; depth_max[v] = b * widen;
    }
    return MVS_OK;
}

}  // extern "C"
