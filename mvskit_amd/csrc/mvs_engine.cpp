// mvs_engine.cpp -- the core of the C ABI in include/mvskit_engine.h: the engine and its device memory, camera set-up and the view
// pyramids, the patch pool's upload / download, and the probes.  The other host units (mvs_engine_impl.h is what they share):
// mvs_engine_pass.cpp (index build -> sweep -> commit), mvs_engine_comm.cpp (the exchange between ranks), mvs_engine_filter.cpp
// (Filter::run), mvs_engine_seed.cpp (the seeding front ends), mvs_engine_output.cpp (point cloud, maps), mvs_engine_mesh.cpp (mesh).
#include <dlfcn.h>

#include <cmath>
#include <cstring>

#include "mvs_engine_impl.h"

using namespace mvseng;

static_assert(sizeof(mvs_patch) == sizeof(DPatch), "mvs_patch and DPatch must be the same bytes");
static_assert((MVS_LISTCAP == 16 || MVS_LISTCAP == 32 || MVS_LISTCAP == 64) && MVS_LISTCAP <= MVS_MAXI && MVS_MAX_IMAGES == MVS_MAXI, "limits out of sync");

namespace mvseng {

thread_local std::string g_err;

Roctx& roctx() {
    static Roctx r;
    static bool tried = false;
    if (tried) return r;
    tried = true;
    void* h = nullptr;
    const char* names[] = {"libroctx64.so", "libroctx64.so.4", "/opt/rocm/lib/libroctx64.so.4"};
    for (const char* n : names) if (!h) h = dlopen(n, RTLD_NOW | RTLD_NOLOAD);
    for (const char* n : names) if (!h) h = dlopen(n, RTLD_NOW | RTLD_LOCAL);
    if (!h) return r;
    r.push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
    r.pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
    if (!r.push || !r.pop) { r.push = nullptr; r.pop = nullptr; }
    return r;
}

RefineSel refine_sel(const mvs_engine* e) {
    return RefineSel{e->refiner.mode == MVS_REFINE_CONVERGED ? 1 : 0, e->refiner.max_evals, e->refiner.xtol};
}

DParams current_params(mvs_engine* e) {
    DParams p = e->prm;
    p.views = e->dviews.p;
    p.pyr32 = e->pyr_narrow ? e->pyr.p : nullptr;
    p.pool = e->pool.p;
    p.pool_n = e->pool_n;
    p.total_cells = e->total_cells;
    p.csr_start = e->start.p; p.csr_cnt = e->cnt_alive.p; p.csr_key = e->key.p; p.csr_id32 = e->id32.p;
    p.vcsr_start = e->vstart.p; p.vcsr_cnt = e->vcnt_alive.p; p.vcsr_id32 = e->vid32.p;
    p.dpgrid = e->dpgrid.p;
    p.geo = e->geo_valid ? e->geo.p : nullptr;
    p.geo_ref = e->geo_valid ? e->geo_ref.p : nullptr;
    return p;
}

bool want_vgrid(const mvs_engine* e) { return e->prm.depth >= 2 && e->prm.enable_check; }

int need_state(const mvs_engine* e, Need need, const char* who) {
    if (!e) { g_err = std::string(who) + ": no engine"; return MVS_ERR_ARG; }
    if (need >= NEED_VIEWS && !e->have_views) { g_err = std::string(who) + ": views not set"; return MVS_ERR_STATE; }
    if (need >= NEED_IDLE && e->staged) { g_err = std::string(who) + ": a pass is waiting for its commit"; return MVS_ERR_STATE; }
    return MVS_OK;
}

int scan_total(mvs_engine* e, const int32_t* flags, int32_t* base, int32_t* scan, int64_t n, int64_t* count) {
    mvsk_exclusive_scan(flags, base, n, scan, e->stream);
    int32_t total = 0;
    if (int r = read_back(e, base + n, &total)) return r;
    HIPCHK(hipGetLastError());
    *count = total;
    return MVS_OK;
}

}  // namespace mvseng

namespace {

void derive_params(mvs_engine* e) {  // PmMvps::init, pmmvps.cpp:32-36,54-67
    const mvs_config& c = e->cfg;
    DParams& p = e->prm;
    p.nviews = c.nviews; p.level = c.level; p.csize = c.csize; p.wsize = c.wsize; p.wsz = c.wsize * c.wsize;
    p.minImageNum = c.minImageNum;
    p.tau = std::min(c.minImageNum * 2, c.nviews);
    p.max_propag = c.max_propag;
    p.cap = c.max_propag * c.csize * c.csize;
    p.depth = c.depth; p.enable_check = c.enable_check; p.view_propagation = c.view_propagation ? 1 : 0;
    p.seed = c.seed; p.refine_steps = c.refine_steps; p.rd0 = c.refine_rd0; p.ra0 = c.refine_ra0;
    p.nccThreshold = c.nccThreshold;
    p.nccThresholdBefore = c.nccThreshold - 0.3f;
    // volatile: the libm calls below run at run time (the same glibc the oracle calls), not folded by the compiler
    volatile float a0 = (float)(60.0f * M_PI / 180.0f), a1 = (float)(60.0f * M_PI / 180.0f);
    volatile double amin = (double)c.maxAngleThreshold, amax = (double)a1;
    volatile float typo = (float)(120.0f / M_PI * 180.0f);
    volatile double d120 = 120.0f * M_PI / 180.0f, d10 = 10.0f * M_PI / 180.0f;
    p.cosAngle0 = cosf(a0);
    p.cosAngle1 = cosf(a1);
    p.cosMinAngle = (float)cos(amin);
    p.cosMaxAngle = (float)cos(amax);
    p.cosNeighborTypo = cosf(typo);  // pmmvps.cpp:124 (deg/rad typo kept)
    p.cosNeighbor120 = (float)cos(d120);
    p.sortThreshold = (float)(1.0f - cos(d10));
    p.ascaleConst = (float)(M_PI / 48.0f);
    p.inv_sz = 1.0f / (float)(c.wsize * c.wsize);
    p.inv_3sz = 1.0f / (float)(3 * c.wsize * c.wsize);
    p.neighborThreshold = 0.5f; p.neighborThreshold1 = 1.0f;
    p.quadThreshold = c.quadThreshold;
    p.list_n = std::min<int>(MVS_LISTCAP, c.nviews);
    p.gram_ld = (p.list_n + 15) / 16 * 16;
}

void invert3(const float* P, float* Minv) {  // Matrix3f::inverse (camera.cpp:304,335), in double
    double a = P[0], b = P[1], c = P[2], d = P[4], e = P[5], f = P[6], g = P[8], h = P[9], i = P[10];
    double A = e * i - f * h, B = -(d * i - f * g), C = d * h - e * g;
    double det = a * A + b * B + c * C;
    double inv[9] = {A, -(b * i - c * h), b * f - c * e, B, a * i - c * g, -(a * f - c * d), C, -(a * h - b * g), a * e - b * d};
    for (int k = 0; k < 9; ++k) Minv[k] = (float)(inv[k] / det);
}
inline float hfma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
inline float hdot3(const float* a, const float* b) { return hfma(a[2], b[2], hfma(a[1], b[1], a[0] * b[0])); }
inline float hdot4(const float* a, const float* b) { return hfma(a[3], b[3], hfma(a[2], b[2], hfma(a[1], b[1], a[0] * b[0]))); }
inline void hcross(const float* a, const float* b, float* o) {
    o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}

// Camera::updateCamera (camera.cpp:65-100) + Optim::setAxesScales (optim.cpp:43-65)
void setup_camera(const mvs_engine* e, DView& vw, const float* P0) {
    const int maxLevel = e->cfg.level + 3;
    for (int k = 0; k < 12; ++k) vw.P[0][k] = P0[k];
    for (int l = 1; l < maxLevel; ++l) {
        for (int k = 0; k < 12; ++k) vw.P[l][k] = vw.P[l - 1][k];
        for (int k = 0; k < 8; ++k) vw.P[l][k] /= 2.0f;
    }
    invert3(vw.P[e->cfg.level], vw.Minv);
    const float* r2 = &vw.P[0][8];
    const float n = sqrtf(hdot3(r2, r2));
    for (int k = 0; k < 4; ++k) vw.oaxis[k] = r2[k] / n;
    {
        const float* P = vw.P[0];
        double a = P[0], b = P[1], c = P[2], d = P[4], ee = P[5], f = P[6], g = P[8], h = P[9], i = P[10];
        double A = ee * i - f * h, B = -(d * i - f * g), C = d * h - ee * g;
        double det = a * A + b * B + c * C;
        double inv[9] = {A, -(b * i - c * h), b * f - c * ee, B, a * i - c * g, -(a * f - c * d), C, -(a * h - b * g), a * ee - b * d};
        double q[3] = {P[3], P[7], P[11]};
        vw.center[0] = (float)(-(inv[0] * q[0] + inv[1] * q[1] + inv[2] * q[2]) / det);
        vw.center[1] = (float)(-(inv[3] * q[0] + inv[4] * q[1] + inv[5] * q[2]) / det);
        vw.center[2] = (float)(-(inv[6] * q[0] + inv[7] * q[1] + inv[8] * q[2]) / det);
        vw.center[3] = 1.0f;
    }
    for (int k = 0; k < 3; ++k) vw.zaxis[k] = vw.oaxis[k];
    float xa[3] = {vw.P[0][0], vw.P[0][1], vw.P[0][2]};
    hcross(vw.zaxis, xa, vw.yaxis);
    const float yn = sqrtf(hdot3(vw.yaxis, vw.yaxis));
    for (int k = 0; k < 3; ++k) vw.yaxis[k] /= yn;
    hcross(vw.yaxis, vw.zaxis, vw.xaxis);
    const float x4[4] = {vw.xaxis[0], vw.xaxis[1], vw.xaxis[2], 0.0f}, y4[4] = {vw.yaxis[0], vw.yaxis[1], vw.yaxis[2], 0.0f};
    vw.ipscale = hdot4(&vw.P[0][0], x4) + hdot4(&vw.P[0][4], y4);
}

}  // namespace

extern "C" {

const char* mvs_last_error(void) { return g_err.c_str(); }

int mvs_list_cap(void) { return MVS_LISTCAP; }
int mvs_patch_bytes(void) { return (int)sizeof(mvs_patch); }

int mvs_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

void mvs_default_refiner(mvs_refiner* r) {  // HALVING; CONVERGED's budget as Optim::refinePatch (optim.cpp:471)
    if (!r) return;
    r->mode = MVS_REFINE_HALVING; r->max_evals = 500; r->xtol = 1e-4f;
}

int mvs_engine_set_refiner(mvs_engine* e, const mvs_refiner* r) {
    if (!e || !r) { g_err = "mvs_engine_set_refiner: null argument"; return MVS_ERR_ARG; }
    if ((r->mode != MVS_REFINE_HALVING && r->mode != MVS_REFINE_CONVERGED) || r->max_evals < 5 || r->max_evals > 4096 ||
        !std::isfinite(r->xtol) || !(r->xtol > 0.0f)) {
        g_err = "mvs_engine_set_refiner: unknown mode, max_evals outside 5..4096, or xtol not finite and > 0";
        return MVS_ERR_ARG;
    }
    e->refiner = *r;
    return MVS_OK;
}

void mvs_default_config(mvs_config* c) {  // Option::Option, option.cpp:19-33
    memset(c, 0, sizeof *c);
    c->level = 1; c->csize = 2; c->wsize = 7; c->minImageNum = 3; c->max_propag = 2;
    c->nccThreshold = 0.7f; c->maxAngleThreshold = (float)(10.0f * M_PI / 180.0f); c->quadThreshold = 2.5f;
    c->depth = 1; c->seed = 1; c->refine_steps = 6; c->refine_rd0 = 4.0f; c->refine_ra0 = 4.0f; c->enable_check = 1;
    c->view_begin = 0; c->view_stride = 1; c->device = 0; c->max_patches = 0;
}

int mvs_engine_create(const mvs_config* cfg, mvs_engine** out) {
    if (!cfg || !out) { g_err = "mvs_engine_create: null argument"; return MVS_ERR_ARG; }
    if (cfg->shard_count > 1 && (cfg->shard_index < 0 || cfg->shard_index >= cfg->shard_count)) { g_err = "mvs_engine_create: bad shard_index"; return MVS_ERR_ARG; }
    if (cfg->nviews < 1 || cfg->nviews > MVS_MAXVIEWS || cfg->wsize < 1 || cfg->wsize > 7 || cfg->csize < 1 || cfg->level < 0 ||
        cfg->level > 4 || cfg->max_propag < 1 || cfg->max_propag > 16 || cfg->max_propag * cfg->csize * cfg->csize > MVS_CAPMAX ||
        cfg->view_stride < 1 || cfg->view_begin < 0 || cfg->minImageNum < 1 ||
        std::min(cfg->minImageNum * 2, cfg->nviews) > 16 /* tau (pmmvps.cpp:32) views of a proposal sit in 16 frame lanes */) {
        g_err = "mvs_engine_create: configuration out of range (nviews <= 64, wsize <= 7, min(2 minImageNum, nviews) <= 16, max_propag*csize^2 <= 32)";
        return MVS_ERR_ARG;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { g_err = "mvs_engine_create: no HIP device (the engine has no CPU path)"; return MVS_ERR_NO_DEVICE; }
    if (cfg->device < 0 || cfg->device >= ndev) { g_err = "mvs_engine_create: bad device ordinal"; return MVS_ERR_ARG; }
    HIPCHK(hipSetDevice(cfg->device));
    mvs_engine* e = new mvs_engine();
    e->cfg = *cfg;
    derive_params(e);
    hipError_t he = hipStreamCreate(&e->stream);
    if (he != hipSuccess) { g_err = std::string("hipStreamCreate: ") + hipGetErrorString(he); delete e; return MVS_ERR_HIP; }
    for (auto& ev : e->ev) (void)hipEventCreate(&ev);
    for (auto& ev : e->fev) (void)hipEventCreate(&ev);
    if (e->misc.ensure(misc::words) || e->counters.ensure(MVS_COUNTER_SLOTS) || e->error_flag.ensure(1)) { delete e; return MVS_ERR_HIP; }
    (void)hipMemset(e->misc.p, 0, misc::words * sizeof(unsigned long long));
    (void)hipMemset(e->error_flag.p, 0, sizeof(int32_t));
    *out = e;
    return MVS_OK;
}

int mvs_engine_destroy(mvs_engine* e) {
    if (!e) return MVS_OK;
    (void)hipSetDevice(e->cfg.device);
    (void)hipStreamSynchronize(e->stream);
    (void)mvs_engine_comm_release(e);
    for (auto& ev : e->ev) if (ev) (void)hipEventDestroy(ev);
    for (auto& ev : e->fev) if (ev) (void)hipEventDestroy(ev);
    (void)hipStreamDestroy(e->stream);
    delete e;  // the device memory goes with its DevBufs, the engine's device current
    return MVS_OK;
}

int mvs_engine_set_views(mvs_engine* e, int nviews, const mvs_view_desc* views) {
    if (!e || !views || nviews != e->cfg.nviews) { g_err = "mvs_engine_set_views: nviews must equal the configured number of views"; return MVS_ERR_ARG; }
    HIPCHK(hipSetDevice(e->cfg.device));
    hipStream_t st = e->stream;
    Range rg("mvs:set_views (upload + pyramids)");
    e->mask_bufs.clear();
    e->have_views = false;
    const int maxLevel = e->cfg.level + 3;
    e->hviews.assign(nviews, DView{});
    int cell_base = 0;
    size_t max_bytes = 0;
    for (int v = 0; v < nviews; ++v) {
        if (views[v].width < 8 || views[v].height < 8 || !views[v].rgb) { g_err = "mvs_engine_set_views: bad view"; return MVS_ERR_ARG; }
        max_bytes = std::max(max_bytes, (size_t)views[v].width * views[v].height * 3);
    }
    if (int r = e->tmp_bytes.ensure((int64_t)max_bytes)) return r;
    // The pyramids: every level of every view at a fixed offset (a multiple of 256 bytes) of ONE block, view after view, level after level.
    // A block below 4 GiB can be addressed by a 32-bit byte offset from its base (DView::img_off, the sweep's narrow samplers); their
    // 24-bit multiply of a row number by a row pitch in bytes is exact while both stay below 2^24.
    std::vector<uint64_t> level_off((size_t)nviews * maxLevel);
    uint64_t pyr_bytes = 0;
    bool narrow = true;
    for (int v = 0; v < nviews; ++v) {
        DView& vw = e->hviews[v];
        vw.W[0] = views[v].width; vw.H[0] = views[v].height;
        for (int l = 1; l < maxLevel; ++l) { vw.W[l] = vw.W[l - 1] / 2; vw.H[l] = vw.H[l - 1] / 2; }
        for (int l = 0; l < maxLevel; ++l) {
            level_off[(size_t)v * maxLevel + l] = pyr_bytes;
            pyr_bytes += (std::max<uint64_t>((uint64_t)vw.W[l] * vw.H[l], 1) * 4 + 255) / 256 * 256;
        }
        if ((int64_t)vw.W[0] * 4 >= (1 << 24) || vw.H[0] >= (1 << 24)) narrow = false;
    }
    if (pyr_bytes >= (1ull << 32)) narrow = false;
    if (int r = e->pyr.ensure((int64_t)pyr_bytes)) return r;
    e->pyr_narrow = narrow;
    for (int v = 0; v < nviews; ++v) {
        DView& vw = e->hviews[v];
        setup_camera(e, vw, views[v].P);
        const size_t n0 = (size_t)vw.W[0] * vw.H[0];
        HIPCHK(hipMemcpyAsync(e->tmp_bytes.p, views[v].rgb, n0 * 3, hipMemcpyHostToDevice, st));
        for (int l = 0; l < maxLevel; ++l) {
            const uint64_t off = level_off[(size_t)v * maxLevel + l];
            uint32_t* buf = reinterpret_cast<uint32_t*>(e->pyr.p + off);
            vw.img[l] = buf;
            vw.img_off[l] = (uint32_t)off;  // (cut short in a block of 4 GiB or more, where nothing reads it)
            if (l == 0) mvsk_rgb_to_rgba(e->tmp_bytes.p, buf, (int64_t)n0, st);
            else mvsk_pyr_down(vw.img[l - 1], vw.W[l - 1], vw.H[l - 1], buf, vw.W[l], vw.H[l], st);
        }
        vw.mask = nullptr;
        if (views[v].mask) {  // Image::alloc mask handling (image.cpp:166-183) + buildMaskPyramid (image.cpp:717-747)
            HIPCHK(hipStreamSynchronize(st));
            uint8_t* prev = nullptr;
            for (int l = 0; l <= e->cfg.level; ++l) {
                e->mask_bufs.emplace_back();
                if (int r = e->mask_bufs.back().ensure(std::max<int64_t>((int64_t)vw.W[l] * vw.H[l], 1))) return r;
                uint8_t* m = e->mask_bufs.back().p;
                if (l == 0) {
                    HIPCHK(hipMemcpyAsync(m, views[v].mask, n0, hipMemcpyHostToDevice, st));
                    mvsk_mask_binarise(m, (int64_t)n0, st);
                } else mvsk_mask_down(prev, vw.W[l - 1], vw.H[l - 1], m, vw.W[l], vw.H[l], st);
                prev = m;
            }
            vw.mask = prev;
        }
        HIPCHK(hipStreamSynchronize(st));  // tmp_bytes is reused by the next view
        vw.gh = (vw.H[e->cfg.level] + e->cfg.csize - 1) / e->cfg.csize;  // patch_manager.cpp:36-37
        vw.gw = (vw.W[e->cfg.level] + e->cfg.csize - 1) / e->cfg.csize;
        vw.cell_base = cell_base;
        cell_base += vw.gw * vw.gh;
    }
    e->total_cells = cell_base;
    if (int r = e->dviews.ensure(nviews)) return r;
    HIPCHK(hipMemcpyAsync(e->dviews.p, e->hviews.data(), sizeof(DView) * nviews, hipMemcpyHostToDevice, st));
    const int64_t nc = e->total_cells;
    if (e->cnt.ensure(nc + 2) || e->start.ensure(nc + 2) || e->cursor.ensure(nc + 2) || e->vcnt.ensure(nc + 2) || e->vstart.ensure(nc + 2) ||
        e->vcursor.ensure(nc + 2) || e->start_raw.ensure(nc + 2) || e->dpgrid.ensure(nc + 2) || e->best.ensure(nc + 2) || e->cnt_alive.ensure(nc + 2) || e->vcnt_alive.ensure(nc + 2))
        return MVS_ERR_HIP;
    // Pool capacity: mvs_config.max_patches, else 4 patches per cell (the 1080p runs settle near 1 per cell) -- but never
    // more than a sixth of the device's memory for each of the two pool buffers: the index, staging and scans grow with it.
    // The bound is taken from the TOTAL memory, not from what happens to be free: the ranks of a job must arrive at the same
    // capacity (what still differs -- an explicit max_patches per rank -- is settled collectively in mvs_engine_exchange).
    int64_t pool_cap = e->cfg.max_patches > 0 ? e->cfg.max_patches : 4 * nc;
    if (e->cfg.max_patches <= 0) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && total_b > 0) {
            pool_cap = std::max<int64_t>(std::min<int64_t>(pool_cap, (int64_t)(total_b / 6 / sizeof(DPatch))), std::min<int64_t>(pool_cap, nc));
            // ... and, on a card that is not empty (several ranks on one GPU in a rehearsal, another process, a second engine), no more
            // than fits what is free now: the pool-sized buffers below take 2.5 records + 17 bytes per patch, and the index comes on
            // top.  Ranks that arrive at different capacities this way are settled in mvs_engine_exchange (minimum headroom).
            const double per_patch = 2.5 * (double)sizeof(DPatch) + 17.0;
            const int64_t fit = (int64_t)(0.6 * (double)free_b / per_patch);
            if (fit < pool_cap) pool_cap = std::max<int64_t>(fit, std::min<int64_t>(pool_cap, nc / 4 + 1024));
        }
    }
    e->ids.headroom = e->key.headroom = e->id32.headroom = e->id32_raw.headroom = e->vid32.headroom = true;
    e->geo.headroom = e->geo_ref.headroom = true;
    if (e->pool.ensure(pool_cap) || e->pool_alt.ensure(pool_cap) || e->kill.ensure(pool_cap) || e->kill_cnt.ensure(pool_cap + 2) || e->kill_base.ensure(pool_cap + 2)) return MVS_ERR_HIP;
    HIPCHK(hipMemsetAsync(e->kill.p, 0, (size_t)pool_cap, st));
    // jobs of one colour pass over every view (upper bound, used to size the staging bookkeeping)
    int64_t njobs_max = 0;
    for (int v = 0; v < nviews; ++v) njobs_max += (int64_t)((e->hviews[v].gw + 1) / 2) * e->hviews[v].gh;
    const int maxstage = (e->prm.view_propagation ? 3 : 2) * e->prm.cap * e->prm.max_propag;
    if (e->job_stage.ensure(njobs_max * maxstage) || e->job_nstage.ensure(njobs_max + 2) || e->job_cnt.ensure(njobs_max + misc::job_list_pad) ||
        e->job_base_scan.ensure(njobs_max + misc::job_list_pad) || e->job_list.ensure(std::max<int64_t>(njobs_max, 16)))
        return MVS_ERR_HIP;
    const int64_t scan_n = std::max<int64_t>(std::max<int64_t>(nc, pool_cap), njobs_max);
    if (e->scan_tmp.ensure(scan_n / 256 + 4096)) return MVS_ERR_HIP;
    // Optim::check's second tier: its global-memory id sets and the list of cells to run again (16 MB + 4 B per job) -- here, not in the
    // first pass with check, so that no pass allocates
    if (e->big_tables.ensure((int64_t)256 * 16384) || e->retry_jobs.ensure(std::max<int64_t>(njobs_max, 16))) return MVS_ERR_HIP;
    // likewise what Filter::run needs per patch and per cell (union-find, retry list, the bit per depth-map cell)
    if (e->uf_parent.ensure(pool_cap) || e->uf_size.ensure(pool_cap) || e->dirty.ensure((nc + 31) / 32 + 1) || e->fstat_buf.ensure(fstat::words)) return MVS_ERR_HIP;
    if (e->staging.ensure(std::max<int64_t>(pool_cap / 2, 1024))) return MVS_ERR_HIP;
    if (e->tmp_rec_out.ensure(16)) return MVS_ERR_HIP;
    HIPCHK(hipStreamSynchronize(st));
    e->pool_n = 0;
    e->have_views = true;
    e->staged = false;
    return MVS_OK;
}

int mvs_engine_grid_dims(mvs_engine* e, int view, int* gw, int* gh) {
    if (!e || !e->have_views || view < 0 || view >= e->cfg.nviews) { g_err = "mvs_engine_grid_dims: bad view / views not set"; return MVS_ERR_STATE; }
    if (gw) *gw = e->hviews[view].gw;
    if (gh) *gh = e->hviews[view].gh;
    return MVS_OK;
}

int mvs_engine_get_pyramid(mvs_engine* e, int view, int level, uint8_t* rgb_out, int* W, int* H) {
    if (!e || !e->have_views || view < 0 || view >= e->cfg.nviews || level < 0 || level >= e->cfg.level + 3) { g_err = "mvs_engine_get_pyramid: bad argument"; return MVS_ERR_ARG; }
    HIPCHK(hipSetDevice(e->cfg.device));
    const DView& vw = e->hviews[view];
    if (W) *W = vw.W[level];
    if (H) *H = vw.H[level];
    if (!rgb_out) return MVS_OK;
    const int64_t n = (int64_t)vw.W[level] * vw.H[level];
    if (int r = e->tmp_bytes.ensure(n * 3)) return r;
    mvsk_rgba_to_rgb(vw.img[level], e->tmp_bytes.p, n, e->stream);
    HIPCHK(hipMemcpyAsync(rgb_out, e->tmp_bytes.p, (size_t)n * 3, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return MVS_OK;
}

int mvs_engine_set_thresholds(mvs_engine* e, float ncc, float before, int depth) {
    if (!e) return MVS_ERR_ARG;
    e->prm.nccThreshold = ncc; e->prm.nccThresholdBefore = before; e->prm.depth = depth;
    return MVS_OK;
}
int mvs_engine_get_thresholds(mvs_engine* e, float* ncc, float* before, int* depth) {
    if (!e) return MVS_ERR_ARG;
    if (ncc) *ncc = e->prm.nccThreshold;
    if (before) *before = e->prm.nccThresholdBefore;
    if (depth) *depth = e->prm.depth;
    return MVS_OK;
}
int mvs_engine_update_threshold(mvs_engine* e) {  // pmmvps.cpp:70-74 and :105
    if (!e) return MVS_ERR_ARG;
    e->prm.nccThreshold -= 0.05f; e->prm.nccThresholdBefore -= 0.05f; ++e->prm.depth;
    return MVS_OK;
}

int mvs_engine_upload_patches(mvs_engine* e, int64_t n, const mvs_patch* patches) {
    if (!e || !e->have_views) { g_err = "mvs_engine_upload_patches: views not set"; return MVS_ERR_STATE; }
    if (n < 0 || (n > 0 && !patches)) return MVS_ERR_ARG;
    if (e->staged) { g_err = "mvs_engine_upload_patches: a pass is waiting for its commit"; return MVS_ERR_STATE; }
    HIPCHK(hipSetDevice(e->cfg.device));
    Range rg("mvs:upload_patches");
    // readPatches (patch_manager.cpp:450-463): m_fix = 0, m_tmp = score2, m_vimages cleared, empty m_images dropped
    std::vector<mvs_patch> recs;
    recs.reserve((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        mvs_patch p = patches[i];
        p.nimages = std::min(p.nimages, MVS_LISTCAP);
        if (p.nimages <= 0) continue;
        memset(p.images + p.nimages, 0, sizeof p.images - (size_t)p.nimages);  // entries past the (truncated) list are not data
        p.nvimages = 0;
        memset(p.vimages, 0, sizeof p.vimages);
        p.tmp = std::max(0.0f, p.ncc - e->prm.nccThreshold) * p.nimages;
        p.flags = 1;
        p.id = 0;
        recs.push_back(p);
    }
    if (e->pool_n + (int64_t)recs.size() > e->pool.cap) { g_err = "mvs_engine_upload_patches: patch pool capacity exceeded (raise mvs_config.max_patches)"; return MVS_ERR_CAPACITY; }
    if (!recs.empty()) HIPCHK(hipMemcpyAsync(e->pool.p + e->pool_n, recs.data(), recs.size() * sizeof(mvs_patch), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    e->pool_n += (int64_t)recs.size();
    e->ncc_dirty = true;
    return MVS_OK;
}

// Sizes the buffers of both cell indexes for `list_entries` memberships each (0: MAX_NUM_OF_PATCHES per cell of every view, what
// m_pgrids holds after the trim), so that Propagate::run / Filter::run allocate nothing while the lists stay below that: the first
// iterations of a run otherwise grow them inside the call (free + allocate, gigabytes at a time).  A reserve that fails may leave
// some of these buffers replaced or emptied; nothing reads the lists across calls (every pass and Filter::run builds its own index).
int mvs_engine_reserve(mvs_engine* e, int64_t list_entries) {
    if (!e || !e->have_views || list_entries < 0) { g_err = "mvs_engine_reserve: views not set, or a negative size"; return MVS_ERR_ARG; }
    HIPCHK(hipSetDevice(e->cfg.device));
    int64_t n = list_entries > 0 ? list_entries : e->total_cells * (int64_t)(e->cfg.max_propag * e->cfg.csize * e->cfg.csize);
    // a buffer that is allocated here is also written once: the first use of fresh device memory is slow in a process that has just
    // come up (the first m_vpgrids build of the first process on a box took 95 ms instead of 21), and this call is the set-up
    auto take = [&](auto& buf, int64_t want) -> int {
        const int64_t before = buf.cap;
        if (int r = buf.ensure(want)) return r;
        if (buf.cap != before && hipMemsetAsync(buf.p, 0, (size_t)buf.cap * sizeof(*buf.p), e->stream) != hipSuccess) { (void)hipGetLastError(); return MVS_ERR_HIP; }
        return MVS_OK;
    };
    if (take(e->ids, n + 16) || take(e->key, n + 16) || take(e->id32, n + 16) || take(e->id32_raw, n + 16) || take(e->vid32, n + 16)) return MVS_ERR_HIP;
    HIPCHK(hipStreamSynchronize(e->stream));
    return MVS_OK;
}

int mvs_engine_clear_patches(mvs_engine* e) {
    if (!e) return MVS_ERR_ARG;
    HIPCHK(hipSetDevice(e->cfg.device));
    if (e->kill.p) HIPCHK(hipMemsetAsync(e->kill.p, 0, (size_t)e->kill.cap, e->stream));
    e->pool_n = 0; e->staged = false; e->counted = false;
    return MVS_OK;
}

int mvs_engine_num_patches(mvs_engine* e, int64_t* n_alive) {
    if (!e || !n_alive) return MVS_ERR_ARG;
    HIPCHK(hipSetDevice(e->cfg.device));
    return count_pool(e, Count::alive, n_alive);
}

int mvs_engine_download_patches(mvs_engine* e, int64_t cap, mvs_patch* out, int64_t* n) {
    if (!e || !n) return MVS_ERR_ARG;
    int64_t alive = 0;
    if (int r = mvs_engine_num_patches(e, &alive)) return r;  // count_pool: kill_base = the scan of the alive flags
    *n = alive;
    if (!out || alive == 0) return MVS_OK;
    const int64_t m = std::min(cap, alive);
    if (int r = e->tmp_rec_out.ensure(alive)) return r;
    mvsk_alive_gather(e->pool.p, e->pool_n, e->kill_base.p, e->tmp_rec_out.p, alive, e->stream);
    HIPCHK(hipMemcpyAsync(out, e->tmp_rec_out.p, (size_t)m * sizeof(mvs_patch), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return MVS_OK;
}

int mvs_engine_sweep_pairs(mvs_engine* e, int64_t out[6]) {
    if (!e || !out) return MVS_ERR_ARG;
    for (int k = 0; k < 6; ++k) out[k] = e->sweep_pairs[k];
    return MVS_OK;
}

int mvs_engine_sweep_repeats(mvs_engine* e, int64_t out[2]) {
    if (!e || !out) return MVS_ERR_ARG;
    for (int k = 0; k < 2; ++k) out[k] = e->sweep_repeats[k];
    return MVS_OK;
}

int mvs_engine_sweep_kernels(mvs_engine* e, int64_t out[2]) {
    if (!e || !out) return MVS_ERR_ARG;
    for (int k = 0; k < 2; ++k) out[k] = e->sweep_kernels[k];
    return MVS_OK;
}

int mvs_engine_sampler_launches(mvs_engine* e, int64_t out[4]) {
    if (!e || !out) return MVS_ERR_ARG;
    for (int k = 0; k < 4; ++k) out[k] = e->sampler_launches[k];
    return MVS_OK;
}

int mvs_engine_last_timing(mvs_engine* e, mvs_timing* t) {
    if (!e || !t) return MVS_ERR_ARG;
    *t = e->timing;
    return MVS_OK;
}

int mvs_engine_depth_normal_map(mvs_engine* e, int view, int kind, float* depth, float* normal, int32_t* ids) {
    if (!e || !e->have_views || view < 0 || view >= e->cfg.nviews || kind < 0 || kind > 1) { g_err = "mvs_engine_depth_normal_map: bad argument"; return MVS_ERR_ARG; }
    HIPCHK(hipSetDevice(e->cfg.device));
    hipStream_t st = e->stream;
    const DView& vw = e->hviews[view];
    const int ncells = vw.gw * vw.gh;
    const DParams p = current_params(e);
    const unsigned long long* sel = nullptr;
    if (kind == 0) {
        HIPCHK(hipMemsetAsync(e->dpgrid.p, 0xff, (size_t)e->total_cells * sizeof(unsigned long long), st));
        mvsk_depth_maps(p, e->dpgrid.p, nullptr, st);
        sel = e->dpgrid.p + vw.cell_base;
    } else {
        HIPCHK(hipMemsetAsync(e->best.p, 0, (size_t)ncells * sizeof(unsigned long long), st));
        mvsk_best_ncc_map(p, view, e->best.p, st);
        sel = e->best.p;
    }
    if (e->tmp_f_out.ensure((int64_t)ncells * 4) || e->tmp_i.ensure(ncells)) return MVS_ERR_HIP;
    mvsk_map_extract(p, view, kind, sel, e->tmp_f_out.p, e->tmp_f_out.p + ncells, e->tmp_i.p, ncells, st);
    if (depth) HIPCHK(hipMemcpyAsync(depth, e->tmp_f_out.p, (size_t)ncells * sizeof(float), hipMemcpyDeviceToHost, st));
    if (normal) HIPCHK(hipMemcpyAsync(normal, e->tmp_f_out.p + ncells, (size_t)ncells * 3 * sizeof(float), hipMemcpyDeviceToHost, st));
    if (ids) HIPCHK(hipMemcpyAsync(ids, e->tmp_i.p, (size_t)ncells * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return MVS_OK;
}

int mvs_engine_probe(mvs_engine* e, int op, int64_t n, const mvs_patch* in_rec, const float* in_f, mvs_patch* out_rec, float* out_f, int32_t* out_i) {
    if (!e || !e->have_views || n < 0 || op < 0 || op > 6) { g_err = "mvs_engine_probe: bad argument / views not set"; return MVS_ERR_ARG; }
    const RefineSel rs = refine_sel(e);
    if (op == MVS_PROBE_REFINE_X && !rs.simplex) { g_err = "mvs_engine_probe: MVS_PROBE_REFINE_X needs the CONVERGED refiner"; return MVS_ERR_STATE; }
    if (n == 0) return MVS_OK;
    HIPCHK(hipSetDevice(e->cfg.device));
    hipStream_t st = e->stream;
    if (op == MVS_PROBE_POSTPROCESS && e->prm.depth > 0) if (int r = build_index(e, nullptr)) return r;  // setVImagesVGrids reads m_dpgrids
    const int64_t nf_out = op == MVS_PROBE_MATH ? 5 * n : ((op == MVS_PROBE_REFINE || op == MVS_PROBE_REFINE_X) && rs.simplex ? 4 * n : n);
    if (e->tmp_rec_in.ensure(n) || e->tmp_rec_out.ensure(n) || e->tmp_f_in.ensure(n) || e->tmp_f_out.ensure(nf_out) || e->tmp_i.ensure(n + 1)) return MVS_ERR_HIP;
    if (op == MVS_PROBE_MATH) {
        if (!in_f || !out_f) return MVS_ERR_ARG;
        HIPCHK(hipMemcpyAsync(e->tmp_f_in.p, in_f, (size_t)n * sizeof(float), hipMemcpyHostToDevice, st));
    } else {
        if (!in_rec) return MVS_ERR_ARG;
        HIPCHK(hipMemcpyAsync(e->tmp_rec_in.p, in_rec, (size_t)n * sizeof(mvs_patch), hipMemcpyHostToDevice, st));
    }
    HIPCHK(hipMemsetAsync(e->tmp_i.p, 0, (size_t)(n + 1) * sizeof(int32_t), st));
    const DParams p = current_params(e);
    const KernelVariant probe_kernel = mvsk_probe(p, op, n, e->tmp_rec_in.p, e->tmp_f_in.p, e->tmp_rec_out.p, e->tmp_f_out.p, e->tmp_i.p, rs, st);
    if (probe_kernel.launched) e->sampler_launches[probe_kernel.narrow ? 3 : 2] += 1;
    if (out_rec && (op == MVS_PROBE_PREPROCESS || op == MVS_PROBE_REFINE || op == MVS_PROBE_POSTPROCESS || op == MVS_PROBE_REFINE_X))
        HIPCHK(hipMemcpyAsync(out_rec, e->tmp_rec_out.p, (size_t)n * sizeof(mvs_patch), hipMemcpyDeviceToHost, st));
    if (out_f && (op == MVS_PROBE_NCC || op == MVS_PROBE_COST || op == MVS_PROBE_MATH || op == MVS_PROBE_REFINE_X))
        HIPCHK(hipMemcpyAsync(out_f, e->tmp_f_out.p, (size_t)nf_out * sizeof(float), hipMemcpyDeviceToHost, st));
    if (out_i) HIPCHK(hipMemcpyAsync(out_i, e->tmp_i.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    return MVS_OK;
}

}  // extern "C"
