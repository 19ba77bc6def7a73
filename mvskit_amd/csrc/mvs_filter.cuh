// mvs_filter.cuh (part of the unit mvs_patch.hip) -- pool upkeep (kill flags, appended records, the alive pool) and Filter::run: setVImagesVGrids, filterOutside,
// filterExact, filterNeighbor and filterSmallGroups; kernels first, their launchers behind them.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include "mvs_patch_common.cuh"
#include "mvs_check.cuh"
#include "mvs_kernels.h"

using namespace mvsdev;

// PatchManager::sortPatches head (patch_manager.cpp:411-415): patches with m_ncc < 0 get their score.
// One wave looks at 64 patches (a lane each) and then scores, one after the other, those that need it: in steady state
// none does, and the launch is 64 times smaller than one wave per patch.
__global__ __launch_bounds__(64) void k_fill_ncc(DParams prm, unsigned long long* evals) {
    WaveCtx wc = make_wave_ctx(prm);
    const int64_t mine = (int64_t)blockIdx.x * 64 + wc.lane;
    bool need = false;
    if (mine < prm.pool_n) need = (prm.pool[mine].flags & 1) && (prm.pool[mine].ncc < 0.0f);
    unsigned long long todo = ballot(need);
    while (todo) {
        const int l = __ffsll((long long)todo) - 1;
        todo &= todo - 1ull;
        DPatch* p = prm.pool + ((int64_t)blockIdx.x * 64 + l);
        Cand c;
        load_cand(p, wc, c);
        const float ncc = compute_ncc(prm, wc, c.coord, c.normal, c.img, c.nimg);
        if (wc.lane == 0) p->ncc = ncc;
    }
    if (wc.lane == 0 && wc.evals) { atomicAdd(evals, (unsigned long long)wc.evals); atomicAdd(evals + 1, (unsigned long long)wc.view_evals); }
}
__global__ void k_kill_count(const uint8_t* __restrict__ kill, int64_t n, int32_t* __restrict__ cnt) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) cnt[i] = kill[i] ? 1 : 0;
}
__global__ void k_kill_export(const uint8_t* __restrict__ kill, int64_t n, const int32_t* __restrict__ base, int32_t* __restrict__ ids, int64_t cap) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && kill[i] && base[i] < cap) ids[base[i]] = (int32_t)i;
}
__global__ void k_apply_kill_flags(DPatch* pool, uint8_t* kill, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && kill[i]) { pool[i].flags &= ~1; kill[i] = 0; }
}
__global__ void k_apply_kill_ids(DPatch* pool, const int32_t* __restrict__ ids, int64_t n, int64_t pool_n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && ids[i] >= 0 && ids[i] < pool_n) pool[ids[i]].flags &= ~1;
}
__global__ void k_append_records(DPatch* pool, int64_t pool_n, const DPatch* __restrict__ recs, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint4* s4 = reinterpret_cast<const uint4*>(recs + i);
    uint4* d4 = reinterpret_cast<uint4*>(pool + pool_n + i);
    for (int w = 0; w < (int)MVS_REC_U4; ++w) d4[w] = s4[w];
    pool[pool_n + i].flags = 1;
    pool[pool_n + i].id = 0;
}
__global__ void k_alive_count(const DPatch* __restrict__ pool, int64_t n, int32_t* __restrict__ cnt) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) cnt[i] = pool[i].flags & 1;
}
__global__ void k_alive_gather(const DPatch* __restrict__ pool, int64_t n, const int32_t* __restrict__ base, DPatch* __restrict__ out, int64_t cap) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !(pool[i].flags & 1) || base[i] >= cap) return;
    const uint4* s4 = reinterpret_cast<const uint4*>(pool + i);
    uint4* d4 = reinterpret_cast<uint4*>(out + base[i]);
    for (int w = 0; w < (int)MVS_REC_U4; ++w) d4[w] = s4[w];
    out[base[i]].id = (int32_t)i;
}

// =================================================================== Filter::run (pmmvps/filter.cpp:25-49)
DEV void set_vgrids(const DParams& prm, const WaveCtx& wc, Cand& c) {  // PatchManager::setVGrids, patch_manager.cpp:252-261
    c.vgx = 0; c.vgy = 0;
    if (wc.lane < c.nvimg) cell_of(prm, prm.views + c.vimg, c.coord, c.vgx, c.vgy);
}
DEV void store_lists(DPatch* p, const WaveCtx& wc, const Cand& c) {
    if (wc.lane == 0) { p->nimages = c.nimg; p->nvimages = c.nvimg; }
    if (wc.lane < MVS_MAXI) {
        p->images[wc.lane] = (uint8_t)(wc.lane < c.nimg ? c.img : 0);
        p->vimages[wc.lane] = (uint8_t)(wc.lane < c.nvimg ? c.vimg : 0);
    }
}
// Filter::setVGridsVPGrids (filter.cpp:657-664): m_vimages cleared (additive == 0) or kept, then setVImagesVGrids
// (all Filter::run kernels take a patch range [first, last): a rank of a multi-GPU job filters its share of the pool)
// GL lanes per patch (a lane per view; GL >= the views and >= the list cap), 64 / GL patches per wave: with 12 views a wave per
// patch leaves 52 lanes idle through the two dependent gathers of isVisible.
template <int GL>
__global__ __launch_bounds__(64) void k_filter_vimages(DParams prm, int additive, int64_t first, int64_t last, const uint32_t* __restrict__ dirty) {
    __shared__ int s_new[64];
    const int lane = (int)threadIdx.x, g = lane / GL, i = lane % GL;
    const int64_t id = first + (int64_t)blockIdx.x * (64 / GL) + g;
    const bool have = id < last;
    DPatch* p = prm.pool + (have ? id : first);
    const bool act = have && (p->flags & 1);
    const int nimg = act ? min(p->nimages, MVS_LISTCAP) : 0;
    const int nv0 = act && additive ? min(p->nvimages, MVS_LISTCAP) : 0;
    const int my_img = i < MVS_MAXI ? (int)p->images[i] : 0, my_vimg = i < MVS_MAXI ? (int)p->vimages[i] : 0;
    // the views the patch is listed in, as a mask shared by the group
    unsigned long long listed = (i < nimg ? 1ull << my_img : 0ull) | (i < nv0 ? 1ull << my_vimg : 0ull);
#pragma unroll
    for (int d = 1; d < GL; d <<= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)listed, d), hi = (unsigned)__shfl_xor((int)(unsigned)(listed >> 32), d);
        listed |= ((unsigned long long)hi << 32) | lo;
    }
    bool q = false;
    if (act && i < prm.nviews && !((listed >> i) & 1ull)) {
        Cand c;
        c.coord = ld4(p->coord); c.normal = ld4(p->normal);
        int ix, iy;
        const DView* vw = prm.views + i;
        cell_of(prm, vw, c.coord, ix, iy);
        // additive pass after removals only (`dirty`): the view was tested and found hidden when the lists were last brought up to
        // date, and the answer can only change where the depth map did -- in a cell whose nearest patch has been removed
        bool test = true;
        if (dirty && !(ix < 0 || vw->gw <= ix || iy < 0 || vw->gh <= iy)) { const int cell = vw->cell_base + iy * vw->gw + ix; test = (dirty[cell >> 5] >> (cell & 31)) & 1u; }
        q = test && is_visible(prm, c, i, ix, iy, prm.neighborThreshold) != 0;
    }
    const unsigned long long all = __ballot(q);
    const unsigned long long gm = GL == 64 ? all : (all >> (GL * g)) & ((1ull << (GL & 63)) - 1ull);
    const int added = (int)__popcll(gm), pos = (int)__popcll(gm & ((1ull << i) - 1ull));
    if (q) s_new[GL * g + pos] = i;  // the r-th view added, in ascending order
    __syncthreads();
    const int nv = min(MVS_LISTCAP, nv0 + added);
    if (act) {
        if (i == 0) { p->nimages = nimg; p->nvimages = nv; }
        if (i < MVS_MAXI) {
            p->images[i] = (uint8_t)(i < nimg ? my_img : 0);
            p->vimages[i] = (uint8_t)(i < nv0 ? my_vimg : (i < nv ? s_new[GL * g + (i - nv0)] : 0));
        }
        for (int k = i + GL; k < MVS_MAXI; k += GL) { p->images[k] = 0; p->vimages[k] = 0; }  // storage beyond the list cap (GL >= MVS_LISTCAP)
    }
}
// Filter::filterOutside, filter.cpp:51-106: gain < 0 -> removed
__global__ __launch_bounds__(64) void k_filter_outside(DParams prm, uint8_t* kill, int64_t first) {
    __shared__ int s_dummy[1];
    __shared__ int s_gain[MVS_LISTCAP];
    const int64_t pid = first + (int64_t)blockIdx.x;
    const DPatch* p = prm.pool + pid;
    if (!(p->flags & 1)) return;
    WaveCtx wc = make_wave_ctx(prm);
    Cand c;
    load_cand(p, wc, c);
    set_grids(prm, wc, c);
    set_vgrids(prm, wc, c);
    const CheckCtx cx{prm.pool, -1, -1, 0, s_dummy, nullptr};
    const float gain = prm.geo ? compute_gain<true>(prm, wc, cx, c, s_gain) : compute_gain<false>(prm, wc, cx, c, s_gain);
    if (wc.lane == 0 && gain < 0.0f) kill[pid] = 1;
}
// The packed geometry of Filter::run's stages (DParams::geo, geo_ref): a lane per pool record.  *bad becomes 1 when an alive record's
// coord.w is not 1 or its normal.w not 0 -- the packed form leaves them out, so the stages then read the records as before.
__global__ void k_geo_pack(const DPatch* pool, int64_t n, float4* geo, uint8_t* ref, int* bad) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const DPatch* p = pool + i;
    const F4 c = ld4(p->coord), nr = ld4(p->normal);
    geo[2 * i] = make_float4(c.x, c.y, c.z, p->dscale);
    geo[2 * i + 1] = make_float4(nr.x, nr.y, nr.z, p->ncc);
    ref[i] = p->images[0];
    if ((p->flags & 1) && !(c.w == 1.0f && nr.w == 0.0f)) *bad = 1;
}
// Filter::filterExact, filter.cpp:148-263.
// Visibility phase (filterExactSub: PatchManager::isVisible in the patch's cell and its four neighbours, per view of
// m_images): FOUR patches per wave, lane 16 q + i = view i of patch 4 * block + q.  The five depth-map cells of a lane are
// loaded together, then the five patches they name, then the five tests run on one ray / unit / factor -- two dependent
// gathers per lane instead of ten, at four times the lanes per instruction of the one-patch-per-wave form.
// Then, patch by patch: the surviving views in ascending order and Optim::setRefImage with the whole wave.
#define MVS_FE_LANES (MVS_LISTCAP <= 16 ? 16 : (MVS_LISTCAP <= 32 ? 32 : 64))  // lanes per patch in the visibility phase
#define MVS_FE_PATCHES (64 / MVS_FE_LANES)
__global__ __launch_bounds__(64) void k_filter_exact(DParams prm, uint8_t* kill, unsigned long long* evals, unsigned long long* stage, int64_t first, int64_t last) {
    __shared__ int s_scratch[192];
    extern __shared__ float s_texs[];
    WaveCtx wc = make_wave_ctx(prm);
#ifdef MVS_STAGE_TIMING
    const unsigned long long fe_begin = (unsigned long long)__builtin_amdgcn_s_memtime();
    WC_T0(wc)
#endif
    const int q = wc.lane / MVS_FE_LANES, i = wc.lane % MVS_FE_LANES;
    const int64_t id = first + (int64_t)blockIdx.x * MVS_FE_PATCHES + q;
    const bool have = id < last;
    const DPatch* pl = prm.pool + (have ? id : 0);
    const bool alive_l = have && (pl->flags & 1);
    const int nimg_l = alive_l ? min(pl->nimages, MVS_LISTCAP) : 0;
    const bool act = i < nimg_l;
    const int image = act ? (int)pl->images[i] : 0;
    const F4 coord = ld4(pl->coord), normal = ld4(pl->normal);
    WC_ADD(wc, 5)
    bool safe = false;
    {
        const DView* vw = prm.views + image;
        const int w = vw->gw, h = vw->gh, cbase = vw->cell_base;
        const F4 ctr = ld4(vw->center);
        const float ips = vw->ipscale;
        int x, y;
        cell_of(prm, vw, coord, x, y);  // PatchManager::setGrids
        const bool in = act && !(x < 0 || w <= x || y < 0 || h <= y);
        // the five cells of filterExactSub, each behind its guard (filter.cpp:221-251)
        const int dxs[5] = {0, -1, 1, 0, 0}, dys[5] = {0, 0, 0, -1, 1};
        bool ok[5];
        unsigned long long dp[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const int xx = x + dxs[k], yy = y + dys[k];
            ok[k] = in && 0 <= xx && xx < w && 0 <= yy && yy < h;  // the guards 0 < x, x < w-1, ... and isVisible's own range test
            dp[k] = prm.dpgrid[cbase + (ok[k] ? yy * w + xx : 0)];
        }
        F4 qc[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) qc[k] = ld4((prm.pool + (dp[k] == ~0ull ? 0u : (uint32_t)(dp[k] & 0xffffffffull)))->coord);
        // PatchManager::isVisible, patch_manager.cpp:335-376: everything but the depth difference is the same for the five
        const F4 ray = nrm4(sub4(coord, ctr));
        const float factor = fminf(2.0f, 2.0f + dot4(ray, normal));  // a float in the reference (patch_manager.cpp:366), see is_visible
        float unit = 1.0f;  // get_unit
        if (ips != 0.0f) unit = (2.0f * norm4(sub4(coord, ctr)) * (float)(1 << prm.level)) / ips;
        const float rhs = (unit * (float)prm.csize * prm.neighborThreshold1) * factor;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const float diff = dot4(ray, sub4(coord, qc[k]));
            const bool vis = prm.depth == 0 || dp[k] == ~0ull || diff < rhs;
            safe |= ok[k] && vis;
        }
    }
    WC_ADD(wc, 6)
    const unsigned long long safe_b = ballot(safe);
    const unsigned long long alive_b = ballot(alive_l);
    const int tstride = prm.wsz;  // odd for 7x7 / 5x5 windows: the lane-per-pair reads of setRefImage fall in distinct banks
    // The sampling frames of setRefImage for all patches of the wave side by side, in the lanes of the visibility phase (lane
    // MVS_FE_LANES q + i = view i of patch q): getPAxes from the patch's first surviving view in ascending order, i.e. its smallest,
    // and make_frame per surviving view -- once per wave, where patch by patch it ran MVS_FE_PATCHES times with a handful of lanes
    // at work (a third of this kernel's wave time).  The loop below hands each patch's frames to its view lanes.
    Frame fpre = {};
    {
        const unsigned long long gbits = MVS_FE_LANES == 64 ? ~0ull : ((1ull << (MVS_FE_LANES & 63)) - 1ull) << ((MVS_FE_LANES * q) & 63);
        const bool skip_l = (pl->flags & MVS_FLAG_SETTLED) && (int)__popcll(safe_b & gbits) == nimg_l;  // settled and keeps every view
        if (ballot(alive_l && !skip_l)) {
            int vmin = safe ? image : INT_MAX;
            for (int d = 1; d < MVS_FE_LANES; d <<= 1) vmin = min(vmin, __shfl_xor(vmin, d));
            F4 px, py;
            get_paxes(prm, prm.views + (vmin == INT_MAX ? 0 : vmin), coord, normal, px, py);
            fpre = make_frame(prm, coord, px, py, normal, image, safe);
        }
    }
    WC_ADD(wc, 1)
    for (int g = 0; g < MVS_FE_PATCHES; ++g) {
        if (!((alive_b >> ((MVS_FE_LANES * g) & 63)) & 1ull)) continue;
        DPatch* p = prm.pool + (first + (int64_t)blockIdx.x * MVS_FE_PATCHES + g);
        const int pflags = p->flags;
        Cand c;
        load_cand(p, wc, c);
        const vmask_t sm = (vmask_t)((safe_b >> ((MVS_FE_LANES * g) & 63)) & (MVS_FE_LANES == 64 ? ~0ull : (1ull << (MVS_FE_LANES & 63)) - 1ull));  // bit i: view m_images[i] of patch g survives
        // A patch whose list IS the outcome of this stage's setRefImage for its set of views (MVS_FLAG_SETTLED, set below) and which
        // keeps every view: the outcome is a function of the position, the normal, the set of views and the pyramids alone (the
        // survivors are taken in ascending view order, the axes from the first of them), so it would come out as it stands.
        if ((pflags & MVS_FLAG_SETTLED) && (int)vpop(sm) == c.nimg) continue;
        // the survivors in ascending view order (the image-major loop of filterExactSub)
        __syncthreads();
        if (wc.lane < MVS_MAXVIEWS) s_scratch[wc.lane] = 0;
        __syncthreads();
        if (wc.lane < c.nimg && ((sm >> wc.lane) & 1u)) s_scratch[c.img] = 1 + MVS_FE_LANES * g + wc.lane;  // where this view's frame lies
        __syncthreads();
        const int src1 = s_scratch[wc.lane];
        const bool present = src1 != 0;
        const unsigned long long pm = ballot(present);
        const int pos = __popcll(pm & ((1ull << wc.lane) - 1ull));
        __syncthreads();
        if (present && pos < MVS_LISTCAP) { s_scratch[64 + pos] = wc.lane; s_scratch[128 + pos] = src1 - 1; }
        __syncthreads();
        c.nimg = min((int)__popcll(pm), MVS_LISTCAP);
        c.img = s_scratch[64 + wc.lane];
        if (prm.minImageNum <= c.nimg) {
            // view lane k < nimg takes the frame of its view; the other lanes a harmless one (the origin of some view's image, ok = 0)
            Frame f;
            {
                const bool mine = wc.lane < c.nimg;
                const int src = mine ? s_scratch[128 + wc.lane] : MVS_FE_LANES * g;
                f.tlx = __shfl(fpre.tlx, src); f.tly = __shfl(fpre.tly, src);
                f.dxx = __shfl(fpre.dxx, src); f.dxy = __shfl(fpre.dxy, src); f.dyx = __shfl(fpre.dyx, src); f.dyy = __shfl(fpre.dyy, src);
                f.w = __shfl(fpre.w, src); f.ok = __shfl(fpre.ok, src);
                f.a_lo = (unsigned)__shfl((int)fpre.a_lo, src); f.a_hi = (unsigned)__shfl((int)fpre.a_hi, src);
                if (!mine) { f.tlx = f.tly = f.dxx = f.dxy = f.dyx = f.dyy = 0.0f; f.ok = 0; }
            }
            WC_ADD(wc, 7)
            set_ref_image(prm, wc, s_texs, tstride, c, nullptr, &f);  // a patch that gets here made the wave compute fpre
            store_lists(p, wc, c);
            if (wc.lane == 0) p->flags = pflags | MVS_FLAG_SETTLED;
            WC_ADD(wc, 7)
        } else {
            if (wc.lane == 0) kill[first + (int64_t)blockIdx.x * MVS_FE_PATCHES + g] = 1;
        }
    }
    // the two work counts as 1024 partial sums (the host adds them): 1.5 M waves adding to one address queue up behind each other
    if (wc.lane == 0 && wc.evals) { atomicAdd(evals + 2 * (blockIdx.x & 1023u), (unsigned long long)wc.evals); atomicAdd(evals + 2 * (blockIdx.x & 1023u) + 1, (unsigned long long)wc.view_evals); }
#ifdef MVS_STAGE_TIMING
    if (stage && wc.lane == 0) {
        atomicAdd(stage, (unsigned long long)__builtin_amdgcn_s_memtime() - fe_begin);
        for (int k = 1; k < 8; ++k) atomicAdd(stage + k, wc.st_acc[k]);
    }
#endif
}
// Filter::filterNeighbor(1), filter.cpp:265-327: fewer than 6 neighbours, or a bad quadric fit.
// First launch (todo == nullptr): every patch, with a hash set / row buffer that fits 2 waves per SIMD; a patch that
// does not fit is appended to `retry`.  Second launch: only those patches, with the large configuration.
template <int HCAP, int RCAP>
__global__ __launch_bounds__(64) void k_filter_neighbor(DParams prm, uint8_t* kill, const int32_t* todo, int32_t ntodo, int32_t* retry, int32_t* nretry,
                                                        int32_t* overflow, unsigned long long* stats /* [1024][4], spread over blocks */, int64_t first) {
    extern __shared__ float s_lds[];
    int* const s_dummy = reinterpret_cast<int*>(s_lds);  // the live list of a destination cell: none here (live_view = -1), never read
    const int64_t id = todo ? (blockIdx.x < (unsigned)ntodo ? todo[blockIdx.x] : -1) : first + (int64_t)blockIdx.x;
    if (id < 0 || id >= prm.pool_n) return;
    const DPatch* p = prm.pool + id;
    if (!(p->flags & 1)) return;
    WaveCtx wc = make_wave_ctx(prm);
#ifdef MVS_STAGE_TIMING  // wave cycles: stats[4096 + k], k = 0 whole wave, 1 load + grids, 9 / 10 findNeighbors' two phases, 11 filterQuad
    unsigned long long st_acc[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const unsigned long long st_begin = CK_NOW();
    auto st_flush = [&]() { st_acc[0] = CK_NOW() - st_begin; if (wc.lane == 0) for (int k = 0; k < 12; ++k) if (st_acc[k]) atomicAdd(stats + 4096 + k, st_acc[k]); };
#endif
    Cand c;
    load_cand(p, wc, c);
    set_grids(prm, wc, c);
#ifdef MVS_STAGE_TIMING
    const CheckCtx cx{prm.pool, -1, -1, 0, s_dummy, st_acc};
    st_acc[1] = CK_NOW() - st_begin;
#else
    const CheckCtx cx{prm.pool, -1, -1, 0, s_dummy, nullptr};
#endif
    int* table = reinterpret_cast<int*>(s_lds);
    unsigned st4[4] = {0u, 0u, 0u, 0u};
    const bool pk = prm.geo != nullptr;
    // the first launch keeps the marks of the row walk behind its set (64 dwords more than the set needs); the second launch's table
    // fills the 64 KB a block may have, and it walks its rows by the binary search
    constexpr bool MK = HCAP == MVS_FILTER_HASH_CAP;
    int* const marks = reinterpret_cast<int*>(s_lds) + MVS_SET_LDS_FLOATS(HCAP, RCAP);
    const int n = pk ? find_neighbors<HCAP, false, true, MK>(prm, wc, cx, c, table, 4.0f, 2, st4, marks) : find_neighbors<HCAP, false, false, MK>(prm, wc, cx, c, table, 4.0f, 2, st4, marks);
    if (n < 0 || n > RCAP) {
        if (wc.lane == 0) {
            if (retry) retry[atomicAdd(nretry, 1)] = (int32_t)id;
            else atomicOr(overflow, 4);
        }
#ifdef MVS_STAGE_TIMING
        st_flush();
#endif
        return;
    }
    if (wc.lane < 4) atomicAdd(stats + 4 * (blockIdx.x & 1023u) + wc.lane, (unsigned long long)(wc.lane == 0 ? st4[0] : wc.lane == 1 ? st4[1] : wc.lane == 2 ? st4[2] : st4[3]));
    const bool reject = n < 6 || (pk ? filter_quad<false, true>(prm, wc, cx, c, table, n, s_lds + rows_offset(n)) : filter_quad<false, false>(prm, wc, cx, c, table, n, s_lds + rows_offset(n))) != 0;
    if (wc.lane == 0 && reject) kill[id] = 1;
#ifdef MVS_STAGE_TIMING
    st_acc[11] = CK_NOW() - st_begin - st_acc[1] - st_acc[9] - st_acc[10];
    st_flush();
#endif
}
// Filter::filterSmallGroups, filter.cpp:432-578, as connected components of the symmetrised relation: lock-free
// union-find, the smaller id becomes the root (uf_find / uf_union, mvs_common.cuh).
__global__ void k_groups_init(int* parent, int* size, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { parent[i] = (int)i; size[i] = 0; }
}
// The relation of Filter::filterSmallGroups: q hangs on p when q is listed (m_pgrids or m_vpgrids) in the 3x3 cells around p in p's
// reference view and isNeighbor(p, q).  MODE 0: every edge joins its two ends (connected components of the symmetrised relation).
// MODE 1 (first pass of the literal labelling): only an edge whose reverse exists too joins them -- q -> p exists iff p is listed in
// q's reference view w (w in p's m_images or m_vimages, p's cell there inside the grid) within one cell of q's own cell; isNeighbor is
// symmetric.  MODE 2 (second pass): the edges that still run between two different sets, as (root of p, root of q) pairs.
// One wave per patch: the 18 lists (3x3 cells, m_pgrids and m_vpgrids) are laid end to end and the lanes take consecutive entries, so
// a wave reads its 48-byte entries as contiguous runs (a lane per patch reads one cache line per lane and load, and 2048 lanes per
// CU evict each other's lines between the three loads of an entry: 23.7 ms per call at 1080p against 13.5 for this form).
template <int MODE>
__global__ __launch_bounds__(256) void k_groups_edges(DParams prm, int* parent, int2* edges, int* nedges, int cap) {
    const int64_t id = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = (int)(threadIdx.x & 63u);
    if (id >= prm.pool_n) return;
    const DPatch* p = prm.pool + id;
    if (!(p->flags & 1)) return;
    const PGeo me = load_geo(p);
    const DView* vw = prm.views + me.ref;
    unsigned long long listed = 0ull;  // the views p is listed in
    if (MODE == 1) {
        for (int i = 0; i < min(p->nimages, MVS_LISTCAP); ++i) listed |= 1ull << p->images[i];
        for (int i = 0; i < min(p->nvimages, MVS_LISTCAP); ++i) listed |= 1ull << p->vimages[i];
    }
    int gx, gy;
    cell_of(prm, vw, me.coord, gx, gy);
    // lane l < 18: list l = (kind, dy, dx); its start and length, and the running total before it
    csr_off_t lstart = 0;
    int ln = 0;
    if (lane < 18) {
        const int kind = lane / 9, yt = gy + (lane % 9) / 3 - 1, xt = gx + lane % 3 - 1;
        if (!(yt < 0 || vw->gh <= yt || xt < 0 || vw->gw <= xt)) {
            const int g = vw->cell_base + yt * vw->gw + xt;
            lstart = kind == 0 ? prm.csr_start[g] : prm.vcsr_start[g];
            ln = kind == 0 ? prm.csr_cnt[g] : prm.vcsr_cnt[g];
        }
    }
    int before = ln;  // inclusive running total over the lanes, then exclusive
    for (int d = 1; d < 32; d <<= 1) { const int o = __shfl_up(before, d); if (lane >= d) before += o; }
    const int total = __builtin_amdgcn_readlane(before, 17);
    before -= ln;
    int myroot = -1;
    // entry k of the 18 lists laid end to end: the list it falls in is the last lane whose list begins at or before k (lanes 18.. hold the
    // total; an empty list never wins)
    auto entry_at = [&](int k, int& eid) -> bool {
        int lo = 0;
#pragma unroll
        for (int step = 16; step >= 1; step >>= 1) { const int pc = __shfl(before, lo + step); if (pc <= k) lo += step; }
        const int l_first = __shfl(before, lo);
        const csr_off_t l_start = __shfl(lstart, lo);
        if (k >= total) return false;
        eid = (lo >= 9 ? prm.vcsr_id32 : prm.csr_id32)[l_start + (k - l_first)];  // the lists hold ids; edge() fetches the geometry from the record
        return true;
    };
    auto edge = [&](const int eid) {
        if (eid == (int)id) return;
        // two patches that hang on the same node are in one set already: one load instead of the predicate and the two root searches
        // of a union -- the common case once the large component has formed and its paths are short
        if (MODE != 2 && __atomic_load_n(&parent[eid], __ATOMIC_RELAXED) == __atomic_load_n(&parent[id], __ATOMIC_RELAXED)) return;
        // (only for the entries the same-set test lets through)  A listed patch may be dead: the m_pgrids lists are not rebuilt after
        // Filter::filterNeighbor's handful of removals (mvs_engine_filter) -- its flags lie in the line that holds its geometry
        if (!(prm.pool[eid].flags & 1)) return;
        const PGeo q = load_geo(prm.pool + eid);
        if (!is_neighbor(prm, me, q, 1.0f /* m_neighborThreshold2, pmmvps.cpp:61 */)) return;
        if (MODE == 0) uf_union(parent, (int)id, eid);
        else if (MODE == 1) {
            if (!((listed >> q.ref) & 1ull)) return;
            const DView* qw = prm.views + q.ref;
            int px, py, qx, qy;
            cell_of(prm, qw, me.coord, px, py);
            cell_of(prm, qw, q.coord, qx, qy);
            if (px < 0 || qw->gw <= px || py < 0 || qw->gh <= py) return;
            if (abs(px - qx) <= 1 && abs(py - qy) <= 1) uf_union(parent, (int)id, eid);
        } else {
            if (myroot < 0) myroot = uf_find(parent, (int)id);
            const int rq = uf_find(parent, eid);
            if (rq != myroot) {
                const int k2 = atomicAdd(nedges, 1);
                if (k2 < cap) edges[k2] = make_int2(myroot, rq);
            }
        }
    };
    for (int k0 = 0; k0 < total; k0 += 128) {  // two rounds of entries in flight (a patch meets ~120)
        int e0 = -1, e1 = -1;
        const bool h0 = entry_at(k0 + lane, e0), h1 = entry_at(k0 + 64 + lane, e1);
        if (h0) edge(e0);
        if (h1) edge(e1);
    }
}
// `sat`: a set's size is only ever compared with the removal threshold, so counting stops there (a plain load first) -- the one giant
// component drew 94 k adds to one address per call.  INT_MAX where the sizes themselves are used (the literal labelling).
__global__ void k_groups_count(DParams prm, int* parent, int* size, int sat) {
    const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= prm.pool_n || !(prm.pool[id].flags & 1)) return;
    const int r = uf_find(parent, (int)id);
    parent[id] = r;
    // one giant component holds almost every patch: lanes that share the first active lane's root add once
    const int r0 = __builtin_amdgcn_readfirstlane(r);
    const unsigned long long same = __ballot(r == r0);
    if (r == r0) { if ((int)(threadIdx.x & 63u) == __ffsll((long long)same) - 1 && __atomic_load_n(&size[r0], __ATOMIC_RELAXED) < sat) atomicAdd(&size[r0], (int)__popcll(same)); }
    else if (__atomic_load_n(&size[r], __ATOMIC_RELAXED) < sat) atomicAdd(&size[r], 1);
}
__global__ void k_groups_kill(DParams prm, const int* parent, const int* size, int threshold, uint8_t* kill) {
    const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= prm.pool_n || !(prm.pool[id].flags & 1)) return;
    if (size[parent[id]] < threshold) kill[id] = 1;
}

// =================================================================== host-callable launchers
void mvsk_fill_ncc(const DParams& prm, unsigned long long* evals, hipStream_t st) {
    if (prm.pool_n > 0) hipLaunchKernelGGL(k_fill_ncc, dim3((unsigned)((prm.pool_n + 63) / 64)), dim3(64), MVS_FRAME_LDS_BYTES, st, prm, evals);
}
void mvsk_kill_count(const uint8_t* kill, int64_t n, int32_t* cnt, hipStream_t st) { if (n > 0) hipLaunchKernelGGL(k_kill_count, dim3(nblk(n, 256)), dim3(256), 0, st, kill, n, cnt); }
void mvsk_kill_export(const uint8_t* kill, int64_t n, const int32_t* base, int32_t* ids, int64_t cap, hipStream_t st) {
    if (n > 0) hipLaunchKernelGGL(k_kill_export, dim3(nblk(n, 256)), dim3(256), 0, st, kill, n, base, ids, cap);
}
void mvsk_apply_kill_flags(DPatch* pool, uint8_t* kill, int64_t n, hipStream_t st) { if (n > 0) hipLaunchKernelGGL(k_apply_kill_flags, dim3(nblk(n, 256)), dim3(256), 0, st, pool, kill, n); }
void mvsk_apply_kill_ids(DPatch* pool, const int32_t* ids, int64_t n, int64_t pool_n, hipStream_t st) {
    if (n > 0) hipLaunchKernelGGL(k_apply_kill_ids, dim3(nblk(n, 256)), dim3(256), 0, st, pool, ids, n, pool_n);
}
void mvsk_append_records(DPatch* pool, int64_t pool_n, const DPatch* recs, int64_t n, hipStream_t st) {
    if (n > 0) hipLaunchKernelGGL(k_append_records, dim3(nblk(n, 256)), dim3(256), 0, st, pool, pool_n, recs, n);
}
void mvsk_alive_count(const DPatch* pool, int64_t n, int32_t* cnt, hipStream_t st) { if (n > 0) hipLaunchKernelGGL(k_alive_count, dim3(nblk(n, 256)), dim3(256), 0, st, pool, n, cnt); }
void mvsk_alive_gather(const DPatch* pool, int64_t n, const int32_t* base, DPatch* out, int64_t cap, hipStream_t st) {
    if (n > 0) hipLaunchKernelGGL(k_alive_gather, dim3(nblk(n, 256)), dim3(256), 0, st, pool, n, base, out, cap);
}
void mvsk_filter_vimages(const DParams& prm, int additive, int64_t first, int64_t last, const uint32_t* dirty, hipStream_t st) {
    if (last <= first) return;
    const int gl = std::max(prm.nviews <= 16 ? 16 : (prm.nviews <= 32 ? 32 : 64), (int)MVS_LISTCAP);
    const unsigned nb = (unsigned)((last - first + 64 / gl - 1) / (64 / gl));
    if (gl == 16) hipLaunchKernelGGL(k_filter_vimages<16>, dim3(nb), dim3(64), 0, st, prm, additive, first, last, dirty);
    else if (gl == 32) hipLaunchKernelGGL(k_filter_vimages<32>, dim3(nb), dim3(64), 0, st, prm, additive, first, last, dirty);
    else hipLaunchKernelGGL(k_filter_vimages<64>, dim3(nb), dim3(64), 0, st, prm, additive, first, last, dirty);
}
void mvsk_geo_pack(const DPatch* pool, int64_t n, float4* geo, uint8_t* ref, int* bad, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_geo_pack, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, pool, n, geo, ref, bad);
}
void mvsk_filter_outside(const DParams& prm, uint8_t* kill, int64_t first, int64_t last, hipStream_t st) {
    if (last > first) hipLaunchKernelGGL(k_filter_outside, dim3((unsigned)(last - first)), dim3(64), 0, st, prm, kill, first);
}
// Filter::filterExact needs the LDS of setRefImage only (frames + the textures of a list), not Optim::check's id set: 7.9 KB instead of
// 9.5 KB per wave at 12 views -- the kernel waits on dependent gathers (vector ALU busy 37 %), so resident waves are what it lacks
size_t mvsk_texs_lds_bytes(const DParams& prm) {
    const size_t texs = texs_gram_lds_bytes(prm);
    return texs > (size_t)MVS_FRAME_LDS_BYTES ? texs : (size_t)MVS_FRAME_LDS_BYTES;
}
void mvsk_filter_exact(const DParams& prm, uint8_t* kill, unsigned long long* evals, unsigned long long* stage, int64_t first, int64_t last, hipStream_t st) {
    if (last > first) hipLaunchKernelGGL(k_filter_exact, dim3((unsigned)((last - first + MVS_FE_PATCHES - 1) / MVS_FE_PATCHES)), dim3(64), mvsk_texs_lds_bytes(prm), st, prm, kill, evals, stage, first, last);
}
void mvsk_filter_neighbor(const DParams& prm, uint8_t* kill, int32_t* retry, int32_t* nretry, int32_t* overflow, unsigned long long* stats, int64_t first, int64_t last, hipStream_t st) {
    if (last <= first) return;
    hipLaunchKernelGGL((k_filter_neighbor<MVS_FILTER_HASH_CAP, MVS_FILTER_ROW_CAP>), dim3((unsigned)(last - first)), dim3(64),
                       (size_t)(MVS_SET_LDS_FLOATS(MVS_FILTER_HASH_CAP, MVS_FILTER_ROW_CAP) + 64) * sizeof(float), st, prm, kill, (const int32_t*)nullptr, 0, retry, nretry, overflow, stats, first);
}
void mvsk_filter_neighbor_retry(const DParams& prm, uint8_t* kill, const int32_t* todo, int32_t ntodo, int32_t* overflow, unsigned long long* stats, hipStream_t st) {
    if (ntodo <= 0) return;
    hipLaunchKernelGGL((k_filter_neighbor<MVS_FILTER2_HASH_CAP, MVS_FILTER2_ROW_CAP>), dim3((unsigned)ntodo), dim3(64),
                       (size_t)MVS_SET_LDS_FLOATS(MVS_FILTER2_HASH_CAP, MVS_FILTER2_ROW_CAP) * sizeof(float), st, prm, kill, todo, ntodo, (int32_t*)nullptr, (int32_t*)nullptr, overflow, stats, (int64_t)0);
}
void mvsk_groups(const DParams& prm, int* parent, int* size, int threshold, uint8_t* kill, hipStream_t st) {
    if (prm.pool_n <= 0) return;
    hipLaunchKernelGGL(k_groups_init, dim3(nblk(prm.pool_n, 256)), dim3(256), 0, st, parent, size, prm.pool_n);
    hipLaunchKernelGGL(k_groups_edges<0>, dim3(nblk(prm.pool_n, 4)), dim3(256), 0, st, prm, parent, (int2*)nullptr, (int*)nullptr, 0);
    hipLaunchKernelGGL(k_groups_count, dim3(nblk(prm.pool_n, 256)), dim3(256), 0, st, prm, parent, size, threshold);
    hipLaunchKernelGGL(k_groups_kill, dim3(nblk(prm.pool_n, 256)), dim3(256), 0, st, prm, parent, size, threshold, kill);
}
// the literal labelling in three steps (mvs_engine.cpp does the middle one on the host): sets joined by edges that run both ways and
// the edges left between different sets; then, with the sizes of the literal groups written over the sets' sizes, the removal
void mvsk_groups_literal_edges(const DParams& prm, int* parent, int* size, int* edges2, int* nedges, int cap, hipStream_t st) {
    if (prm.pool_n <= 0) return;
    hipLaunchKernelGGL(k_groups_init, dim3(nblk(prm.pool_n, 256)), dim3(256), 0, st, parent, size, prm.pool_n);
    hipLaunchKernelGGL(k_groups_edges<1>, dim3(nblk(prm.pool_n, 4)), dim3(256), 0, st, prm, parent, (int2*)nullptr, (int*)nullptr, 0);
    hipLaunchKernelGGL(k_groups_count, dim3(nblk(prm.pool_n, 256)), dim3(256), 0, st, prm, parent, size, INT_MAX);  // also flattens parent[] to the roots
    hipLaunchKernelGGL(k_groups_edges<2>, dim3(nblk(prm.pool_n, 4)), dim3(256), 0, st, prm, parent, reinterpret_cast<int2*>(edges2), nedges, cap);
}
void mvsk_groups_kill(const DParams& prm, const int* parent, const int* size, int threshold, uint8_t* kill, hipStream_t st) {
    if (prm.pool_n > 0) hipLaunchKernelGGL(k_groups_kill, dim3(nblk(prm.pool_n, 256)), dim3(256), 0, st, prm, parent, size, threshold, kill);
}
