// mvs_cand.cuh -- a candidate patch in registers and Optim's stages around the refinement: weights and INCC / NCC, the upkeep of the view
// lists, preProcess, postProcess with setRefImage and the visibility lists, the record to and from registers, generatePatch.
#pragma once
#include <limits.h>
#include "mvs_eval.cuh"

namespace mvsdev {

// ------------------------------------------------------------------ candidate patch (registers)
// Uniform scalars plus view-lane arrays: lane j holds m_images[j], m_grids[j], m_vimages[j], m_vgrids[j].
struct Cand {
    F4 coord, normal;
    float ncc, dscale, ascale, tmp;
    int nimg, nvimg;
    int img, gx, gy;     // view lanes
    int vimg, vgx, vgy;  // view lanes
};

// Optim::computeUnits + computeWeights, optim.cpp:109-132, 942-948: returns the view-lane weight array
DEV float compute_weights(const DParams& prm, const WaveCtx& wc, F4 coord, F4 normal, int img, int n) {
    float unit = 1.0f;
    {
        const DView* vw = prm.views + (wc.lane < n ? img : 0);
        const F4 ctr = ld4(vw->center);
        const float ips = vw->ipscale;
        const F4 dc = sub4(coord, ctr);
        float u = 1.0f;  // get_unit
        if (ips != 0.0f) u = div_rn(2.0f * norm4(dc) * (float)(1 << prm.level), ips);
        const F4 ray = nrm4(sub4(ctr, coord));
        const float d = dot4(ray, normal);
        u = (0.0f < d) ? div_rn(u, d) : (float)(INT_MAX / 2);
        if (wc.lane < n) unit = u;
    }
    const float w0 = rlf(unit, 0);
    float w = fminf(1.0f, div_rn(w0, unit));
    if (wc.lane == 0) w = 1.0f;
    return w;
}

// Optim::computeINCC, optim.cpp:630-706
template <class WC>
DEV float compute_incc(const DParams& prm, WC& wc, F4 coord, F4 normal, int img, int n, float weights, int robust) {
    if (n < 2) return 2.0f;
    const int ref = rli(img, 0);
    F4 px, py;
    get_paxes(prm, prm.views + ref, coord, normal, px, py);
    const int sz = min(prm.tau, n);
    wc.evals++;
    const Frame f = make_frame<WC::narrow>(prm, coord, px, py, normal, img, wc.lane < sz);
    vmask_t okm[1];
    float incc_l;
    eval_views(prm, wc, f, sz, okm, incc_l);
    if (!(okm[0] & 1u)) return 2.0f;
    const float val_l = robust ? robustincc(incc_l) : incc_l;
    float score = 0.0f, total = 0.0f;
    for (int i = 1; i < sz; ++i) {
        if (!((okm[0] >> i) & 1u)) continue;
        const float w = rlf(weights, i);
        total += w;
        score += rlf(val_l, i) * w;
    }
    if (total == 0.0f) return 2.0f;
    return div_rn(score, total);
}
// tail of Optim::computeINCC (optim.cpp:690-705) on per-view robust INCCs that are already known
// (compute_incc keeps its own copy of the loop: ending it in this function moves the code of every kernel that samples)
DEV float weighted_incc(const DParams& prm, vmask_t okm, float val_l, float weights, int n) {
    if (n < 2 || !(okm & 1u)) return 2.0f;
    const int sz = min(prm.tau, n);
    float score = 0.0f, total = 0.0f;
    for (int i = 1; i < sz; ++i) {
        if (!((okm >> i) & 1u)) continue;
        const float w = rlf(weights, i);
        total += w;
        score += rlf(val_l, i) * w;
    }
    if (total == 0.0f) return 2.0f;
    return div_rn(score, total);
}
// PatchManager::computeNcc, patch_manager.cpp:401-404
template <class WC>
DEV float compute_ncc(const DParams& prm, WC& wc, F4 coord, F4 normal, int img, int n) {
    const float w = compute_weights(prm, wc, coord, normal, img, n);
    return 1.0f - unrobustincc(compute_incc(prm, wc, coord, normal, img, n, w, 1));
}

// Optim::setINCCs (vector), optim.cpp:708-746: returns the view-lane INCC array (reference vs every view)
template <class WC>
DEV float set_inccs(const DParams& prm, WC& wc, F4 coord, F4 normal, int img, int n, int robust, vmask_t* okm_out = nullptr,
                    float* texs = nullptr, int tstride = 0, float* ssd_out = nullptr) {
    const int ref = rli(img, 0);
    F4 px, py;
    get_paxes(prm, prm.views + ref, coord, normal, px, py);
    wc.evals++;
    const Frame f = make_frame<WC::narrow>(prm, coord, px, py, normal, img, wc.lane < n);
    vmask_t okm[1];
    float incc_l;
    eval_views(prm, wc, f, n, okm, incc_l, nullptr, texs, tstride, ssd_out);
    if (okm_out) *okm_out = okm[0];
    if (!(okm[0] & 1u)) return 2.0f;
    float incc = robust ? robustincc(incc_l) : incc_l;
    if (wc.lane >= MVS_LISTCAP || !((okm[0] >> (wc.lane & (MVS_VBITS - 1))) & 1u)) incc = 2.0f;
    if (wc.lane == 0) incc = 0.0f;
    return incc;
}

// compaction of view-lane arrays through LDS scratch: keeps lanes with `keep`, order preserved
DEV int compact1(int* scratch, const WaveCtx& wc, bool keep, int& a) {
    const unsigned long long m = ballot(keep);
    const int pos = __popcll(m & ((1ull << wc.lane) - 1ull));
    __syncthreads();
    if (keep) scratch[pos] = a;
    __syncthreads();
    a = scratch[wc.lane];
    return __popcll(m);
}

// Optim::addImages, optim.cpp:165-205
DEV void add_images(const DParams& prm, const WaveCtx& wc, int* scratch, Cand& c) {
    const int ref = rli(c.img, 0);
    bool visib = false;
    for (int j = 0; j < c.nimg; ++j) visib |= (rli(c.img, j) == wc.lane);
    bool q = false;
    if (wc.lane < prm.nviews && wc.lane != ref && !visib) {
        const DView* vw = prm.views + wc.lane;
        float P[12];
        load_P(vw, prm.level, P);
        const int W = vw->W[prm.level], H = vw->H[prm.level];
        const F4 ctr = ld4(vw->center);
        const F3 ic = project_regs(P, c.coord);
        const F4 ray = nrm4(sub4(ctr, c.coord));
        q = !(ic.x < 0.0f || W - 1 <= ic.x || ic.y < 0.0f || H - 1 <= ic.y) && prm.cosAngle0 <= dot4(ray, c.normal);
    }
    const unsigned long long m = ballot(q);
    const int pos = c.nimg + __popcll(m & ((1ull << wc.lane) - 1ull));
    __syncthreads();
    if (wc.lane < c.nimg) scratch[wc.lane] = c.img;
    if (q && pos < MVS_LISTCAP) scratch[pos] = wc.lane;
    __syncthreads();
    c.nimg = min(MVS_LISTCAP, c.nimg + (int)__popcll(m));
    c.img = scratch[wc.lane];
}

// Optim::constraintImages, optim.cpp:207-219
// keep_n > 0 (first constraintImages of postProcess inside the sweep): refinePatch left the final m_ncc to this
// evaluation -- computeINCC at the refined patch samples the first min(tau, keep_n) of these very textures -- so it is
// taken here, as the tail of computeINCC over the robust INCCs of those views with the weights refinePatch computed.
// Kept textures of an evaluation (postProcess: constraintImages hands them to setRefImage): where they lie in LDS, the sum
// of squares of each (view lanes, indexed like the list at the time of the evaluation), which views sampled, and for every
// entry of the list as it is NOW the index it had then (the list is compacted in between).
struct KeptTex {
    float* texs; int tstride;
    float ssd;       // view lanes (old index)
    vmask_t okm;     // bit k: old view k sampled
    int orig;        // view lanes (current index) -> old index
    int n_eval;      // length of the list at the time of the evaluation
};
template <class WC>
DEV void constraint_images(const DParams& prm, WC& wc, int* scratch, Cand& c, float nccThreshold, float keep_w = 0.0f, int keep_n = 0,
                           KeptTex* kt = nullptr) {
    vmask_t okm = 0u;
    float ssd = 1.0f;
    const float inccs = set_inccs(prm, wc, c.coord, c.normal, c.img, c.nimg, 0, &okm, kt ? kt->texs : nullptr, kt ? kt->tstride : 0, kt ? &ssd : nullptr);
    if (keep_n > 0) c.ncc = 1.0f - unrobustincc(weighted_incc(prm, okm, robustincc(inccs), keep_w, keep_n));
    const bool keep = wc.lane == 0 || (wc.lane < c.nimg && inccs < 1.0f - nccThreshold);
    if (kt) {
        kt->ssd = ssd; kt->okm = okm; kt->orig = wc.lane; kt->n_eval = c.nimg;
        (void)compact1(scratch, wc, keep, kt->orig);
    }
    c.nimg = compact1(scratch, wc, keep, c.img);
}

// Optim::sortImages (isFixed = 1), optim.cpp:221-258
DEV void sort_images(const DParams& prm, const WaveCtx& wc, Cand& c) {
    F4 ray{0, 0, 0, 0};
    float unit = 0.0f;
    bool valid = false;
    {  // computeUnits(patch, indexes, units, rays), optim.cpp:86-107
        const bool in = wc.lane < c.nimg;
        const DView* vw = prm.views + (in ? c.img : 0);
        const F4 ctr = ld4(vw->center);
        const float ips = vw->ipscale;
        const F4 r = nrm4(sub4(ctr, c.coord));
        const float d = dot4(r, c.normal);
        const float u = unit_at(prm, ctr, ips, c.coord);
        valid = in && !(d <= 0.0f);
        if (in) ray = r;
        if (valid) unit = div_rn(u, d);
    }
    const unsigned long long vm = ballot(valid);
    const int n0 = __popcll(vm);
    if (n0 < 2) { c.nimg = 0; return; }
    const int first = __ffsll((long long)vm) - 1;
    if (wc.lane == first) unit = 0.0f;
    unsigned long long active = vm;
    int out = 0, k = 0;
    const float thr = prm.sortThreshold;
    while (active) {
        const bool act = (active >> wc.lane) & 1ull;
        const float m = wave_min(act ? unit : __int_as_float(0x7f800000));
        const unsigned long long eq = ballot(act && unit == m);
        const int sel = eq ? __ffsll((long long)eq) - 1 : __ffsll((long long)active) - 1;  // NaN guard: first remaining
        const int vsel = rli(c.img, sel);
        if (wc.lane == k) out = vsel;
        const F4 rsel{rlf(ray.x, sel), rlf(ray.y, sel), rlf(ray.z, sel), rlf(ray.w, sel)};
        active &= ~(1ull << sel);
        if (act && wc.lane != sel) {
            const float ftmp = fminf(thr, fmaxf(thr / 2.0f, 1.0f - dot4(rsel, ray)));
            unit = div_rn(unit * thr, ftmp);
        }
        ++k;
    }
    c.img = out;
    c.nimg = k;
}

// PatchManager::setScales, patch_manager.cpp:378-399
DEV void set_scales(const DParams& prm, const WaveCtx& wc, Cand& c) {
    const int ref = rli(c.img, 0);
    const DView* rv = prm.views + ref;
    const float unit = get_unit(prm, rv, c.coord);
    const float unit2 = 2.0f * unit;
    const F4 ray = nrm4(sub4(c.coord, ld4(rv->center)));
    const int num = min(prm.tau, c.nimg);
    float dn = 0.0f;
    {
        const bool in = wc.lane >= 1 && wc.lane < num;
        float P[12];
        load_P(prm.views + (in ? c.img : 0), prm.level, P);
        const float d = norm3(sub3(project_regs(P, c.coord), project_regs(P, sub4(c.coord, scl4(ray, unit2)))));
        if (in) dn = d;
    }
    float ds = c.dscale;
    for (int i = 1; i < num; ++i) ds += rlf(dn, i);
    ds = div_rn(ds, (float)(num - 1));
    ds = unit2 / ds;
    c.dscale = ds;
    c.ascale = pm_atanf(ds / (unit * (float)prm.wsize / 2.0f));
}

// PhotoSet::checkAngles, photoSet.cpp:77-103 (window test on cosines)
DEV int check_angles(const DParams& prm, const WaveCtx& wc, const Cand& c) {
    F4 ray{0, 0, 0, 0};
    if (wc.lane < c.nimg) ray = nrm4(sub4(ld4((prm.views + c.img)->center), c.coord));
    int count = 0;
    for (int j = 1; j < c.nimg; ++j) {
        const F4 rj{rlf(ray.x, j), rlf(ray.y, j), rlf(ray.z, j), rlf(ray.w, j)};
        const float d = fmaxf(-1.0f, fminf(1.0f, dot4(ray, rj)));
        count += __popcll(ballot(wc.lane < j && d < prm.cosMinAngle && prm.cosMaxAngle < d));
    }
    return count < 1 ? -1 : 0;
}

// Optim::preProcess, optim.cpp:137-163
template <class WC>
DEV int pre_process(const DParams& prm, WC& wc, int* scratch, Cand& c) {
    add_images(prm, wc, scratch, c);
    constraint_images(prm, wc, scratch, c, prm.nccThresholdBefore);
    sort_images(prm, wc, c);
    if (c.nimg > 0) set_scales(prm, wc, c);
    if (c.nimg < prm.minImageNum) return -1;
    if (check_angles(prm, wc, c) == -1) { c.nimg = 0; return -1; }
    return 0;
}

// ------------------------------------------------------------------ post-processing
// Optim::filterImagesByAngle, optim.cpp:325-346
DEV void filter_images_by_angle(const DParams& prm, const WaveCtx& wc, int* scratch, Cand& c, KeptTex* kt = nullptr) {
    bool bad = false;
    if (wc.lane < c.nimg) {
        const F4 ray = nrm4(sub4(ld4((prm.views + c.img)->center), c.coord));
        bad = dot4(ray, c.normal) < prm.cosAngle1;
    }
    const unsigned long long bm = ballot(bad);
    if (bm & 1ull) { c.nimg = 0; return; }
    if (kt) (void)compact1(scratch, wc, wc.lane < c.nimg && !bad, kt->orig);
    c.nimg = compact1(scratch, wc, wc.lane < c.nimg && !bad, c.img);
}
DEV void set_grids(const DParams& prm, const WaveCtx& wc, Cand& c) {
    c.gx = 0; c.gy = 0;
    if (wc.lane < c.nimg) cell_of(prm, prm.views + c.img, c.coord, c.gx, c.gy);
}
// Optim::setRefImage, optim.cpp:348-383 with Optim::setINCCs (matrix), optim.cpp:748-783.
// texs: LDS [LISTCAP][3][tstride] centred textures.  The V(V-1)/2 pair products get one lane each and are summed
// over the samples in the reference's sequential order (optim.cpp:605-607).
DEV int pair_index(int a, int b, int n) { return a * (2 * n - a - 1) / 2 + (b - a - 1); }  // a < b < n
// kt != nullptr (postProcess): the centred textures of these views are in LDS already -- the constraintImages just before
// sampled them at this very patch with this very reference view (engine schedule: they are not sampled a second time, the
// work counters do not count a second evaluation); entry i of the list is entry kt->orig of that evaluation.
// `pre` (Filter::filterExact, which has the frames of four patches made side by side): lane i < nimg holds the finished frame of view c.img
// -- made by make_frame from getPAxes of the FIRST view of the list, as below.
template <class WC>
DEV void set_ref_image(const DParams& prm, WC& wc, float* texs, int tstride, Cand& c, const KeptTex* kt = nullptr, const Frame* pre = nullptr) {
    if (c.nimg == 0) return;
    const int n = c.nimg;
    const int ref = rli(c.img, 0);
    WC_T0(wc)
    vmask_t okmask = 0;
    float ssd_l = 1.0f;
    int orig = wc.lane;  // where view i's texture lies
    if (kt) {
        texs = kt->texs;
        orig = wc.lane < n ? kt->orig : 0;
        ssd_l = __shfl(kt->ssd, orig);
        okmask = vballot(wc.lane < n && ((kt->okm >> orig) & 1u));
        __syncthreads();
    } else {
    Frame f;
    if (pre) f = *pre;
    else {
        F4 px, py;
        get_paxes(prm, prm.views + ref, c.coord, c.normal, px, py);
        f = make_frame<WC::narrow>(prm, c.coord, px, py, c.normal, c.img, wc.lane < n);
    }
    wc.evals++;
    WC_ADD(wc, 1)
    // centred textures to LDS behind the frames this evaluation publishes, their ssd to view lanes
    texs += MVS_FRAME1_LDS_BYTES / 4;
    vmask_t okm1[1];
    float incc_unused;
    eval_views(prm, wc, f, n, okm1, incc_unused, nullptr, texs, tstride, &ssd_l);
    okmask = okm1[0];
    if (!(okmask & 1u)) wc.view_evals += (unsigned)vpop(okmask);  // Optim::setINCCs (matrix) samples every view, whatever the first one did
    }
    const float inv_l = inv_msd(prm, ssd_l);
    WC_ADD(wc, 2)
    __syncthreads();
    // The pair products sum(k) t_a[k] t_b[k] over the 3 wsz elements of two centred textures, k = 3 sample + channel, as ONE
    // k-ordered chain acc = fma(t_a[k], t_b[k], acc) (the reference sums sample by sample, optim.cpp:601-609) -- the order of a
    // f32 MFMA, which is bit for bit such a chain (one rounding per product, no wider accumulator).  The robust INCC of pair
    // q = pair_index(a, b) goes to LDS behind the textures.
#if !MVS_PAIR_MFMA
    const int npairs = n * (n - 1) / 2;
    float* pairv = texs + prm.list_n * 3 * tstride;  // behind the textures (list_n = min(MVS_LISTCAP, nviews): no list is longer)
#endif
#if MVS_PAIR_MFMA
    // The evaluation left the Gram matrix of its textures at texs[a * MVS_GRAM_LD + b] (eval_views).  Row by row, lane b > a turns
    // G[a][b] into the robust INCC of the pair (both triangles); `ne` = the list length of that evaluation, its views' 1 / msd and
    // sampled bits by evaluation-time index.
    {
        const int MVS_GRAM_LD = prm.gram_ld;  // the data set's list length rounded up to a chunk
        const int ne = kt ? kt->n_eval : n;
        const float inv_e = kt ? inv_msd(prm, kt->ssd) : inv_l;
        const vmask_t ok_e = kt ? kt->okm : okmask;
        const bool okb = wc.lane < ne && ((ok_e >> (wc.lane & (MVS_VBITS - 1))) & 1u);
        for (int a = 0; a + 1 < ne; ++a) {
            const float inva = rlf(inv_e, a);
            const bool oka = (ok_e >> a) & 1u;
            if (wc.lane > a && wc.lane < ne) {
                float val = robustincc(1.0f - (texs[a * MVS_GRAM_LD + wc.lane] * (inva * inv_e)) * prm.inv_3sz);
                if (!(oka && okb)) val = 2.0f;
                texs[a * MVS_GRAM_LD + wc.lane] = val;
                texs[wc.lane * MVS_GRAM_LD + a] = val;
            }
        }
    }
#else
    // one lane per pair (a, b), a < b < n: 120 pairs = 2 rounds of 64 lanes for 16 views
    for (int r = 0; r * 64 < npairs; ++r) {
        const int q0 = wc.lane + 64 * r;
        int q = q0;
        const bool act = q < npairs;
        int a = 0;
        if (act) { while (q >= n - 1 - a) { q -= n - 1 - a; ++a; } }
        const int b = act ? a + 1 + q : 1;
        const float* ta = texs + (__shfl(orig, a) * 3) * tstride;
        const float* tb = texs + (__shfl(orig, b) * 3) * tstride;
        float acc = 0.0f;
        for (int i = 0; i < 3 * prm.wsz; i += 3) {
            acc = fma_(ta[i], tb[i], acc); acc = fma_(ta[i + 1], tb[i + 1], acc); acc = fma_(ta[i + 2], tb[i + 2], acc);
        }
        const float inva = __shfl(inv_l, a), invb = __shfl(inv_l, b);
        float val = robustincc(1.0f - (acc * (inva * invb)) * prm.inv_3sz);
        if (!(act && ((okmask >> a) & 1u) && ((okmask >> b) & 1u))) val = 2.0f;
        if (act) pairv[q0] = val;
    }
#endif
    __syncthreads();
    WC_ADD(wc, 3)
    // view lane i: sum over j of inccs[i][j], j ascending (std::accumulate, optim.cpp:368)
    float acc = 0.0f;
#if MVS_PAIR_MFMA
    {
        const int MVS_GRAM_LD = prm.gram_ld;
        const int oi = wc.lane < n ? orig : 0;  // where view i sat in the evaluation whose matrix this is
        for (int j = 0; j < n; ++j) {
            const float v = texs[oi * MVS_GRAM_LD + rli(orig, j)];
            if (wc.lane < n && wc.lane != j) acc += v;
        }
    }
#else
    for (int j = 0; j < n; ++j) {
        const int i = min(wc.lane, n - 1);
        const int a = min(i, j), b = max(i, j);
        const int q = a < b ? pair_index(a, b, n) : 0;
        const float v = pairv[q];
        if (wc.lane < n && wc.lane != j) acc += v;
    }
#endif
    const float big = (float)(INT_MAX / 2);
    const bool cand = wc.lane < n && acc < big;
    const float m = wave_min(cand ? acc : __int_as_float(0x7f800000));
    const unsigned long long eq = ballot(cand && acc == m);
    WC_ADD(wc, 4)
    if (!eq) return;
    const int refindex = __ffsll((long long)eq) - 1;
    const int vref = rli(c.img, refindex), v0 = rli(c.img, 0);
    if (wc.lane == 0) c.img = vref;
    else if (wc.lane == refindex) c.img = v0;
}

// PatchManager::isVisible, patch_manager.cpp:335-376 (per view lane)
DEV int is_visible(const DParams& prm, const Cand& c, int image, int ix, int iy, float strict) {
    const DView* vw = prm.views + image;
    if (ix < 0 || vw->gw <= ix || iy < 0 || vw->gh <= iy) return 0;
    if (prm.depth == 0) return 1;
    const unsigned long long dp = prm.dpgrid[vw->cell_base + iy * vw->gw + ix];
    if (dp == ~0ull) return 1;
    const DPatch* q = prm.pool + (uint32_t)(dp & 0xffffffffull);
    const F4 qc = ld4(q->coord);
    const F4 ray = nrm4(sub4(c.coord, ld4(vw->center)));
    const float diff = dot4(ray, sub4(c.coord, qc));
    // patch_manager.cpp:366-369: the factor is a float there (the double minimum narrowed; 2 + dot is exact in double, so this float sum is
    // the same value), and the product and the comparison run in float
    const float factor = fminf(2.0f, 2.0f + dot4(ray, c.normal));
    const float lhs = get_unit(prm, vw, c.coord) * (float)prm.csize * strict;
    return diff < lhs * factor ? 1 : 0;
}
// PatchManager::setVImagesVGrids, patch_manager.cpp:267-301
DEV void set_vimages_vgrids(const DParams& prm, const WaveCtx& wc, int* scratch, Cand& c) {
    bool visib = false;
    for (int j = 0; j < c.nimg; ++j) visib |= (rli(c.img, j) == wc.lane);
    for (int j = 0; j < c.nvimg; ++j) visib |= (rli(c.vimg, j) == wc.lane);
    bool q = false;
    int ix = 0, iy = 0;
    if (wc.lane < prm.nviews && !visib) {
        cell_of(prm, prm.views + wc.lane, c.coord, ix, iy);
        q = is_visible(prm, c, wc.lane, ix, iy, prm.neighborThreshold) != 0;
    }
    const unsigned long long m = ballot(q);
    const int pos = c.nvimg + __popcll(m & ((1ull << wc.lane) - 1ull));
    __syncthreads();
    if (wc.lane < c.nvimg) { scratch[wc.lane] = c.vimg; scratch[64 + wc.lane] = c.vgx; scratch[128 + wc.lane] = c.vgy; }
    if (q && pos < MVS_LISTCAP) { scratch[pos] = wc.lane; scratch[64 + pos] = ix; scratch[128 + pos] = iy; }
    __syncthreads();
    c.nvimg = min(MVS_LISTCAP, c.nvimg + (int)__popcll(m));
    c.vimg = scratch[wc.lane]; c.vgx = scratch[64 + wc.lane]; c.vgy = scratch[128 + wc.lane];
}
// PhotoSet::getMask(coord, level), photoSet.cpp:223-233
DEV int get_mask_all(const DParams& prm, const WaveCtx& wc, const Cand& c) {
    bool zero = false;
    if (wc.lane < prm.nviews) {
        const DView* vw = prm.views + wc.lane;
        if (vw->mask) {
            const F3 ic = project(vw, c.coord, prm.level);
            const int ix = (int)floorf(ic.x + 0.5f), iy = (int)floorf(ic.y + 0.5f);
            if (!(ix < 0 || vw->W[prm.level] <= ix || iy < 0 || vw->H[prm.level] <= iy))
                zero = vw->mask[(size_t)iy * vw->W[prm.level] + ix] == 0;
        }
    }
    return ballot(zero) ? 0 : -1;
}
DEV float score2(const Cand& c, float thr) { return fmaxf(0.0f, c.ncc - thr) * (float)c.nimg; }

// Optim::postProcess, optim.cpp:260-298 (Optim::check is applied by the caller, which owns the cell lists)
template <class WC>
DEV int post_process(const DParams& prm, WC& wc, int* scratch, float* texs, int tstride, Cand& c, float keep_w = 0.0f, bool keep = false) {
    if (c.nimg < prm.minImageNum) return -1;
    if (get_mask_all(prm, wc, c) == 0) return -1;
    const int keep_n = keep ? c.nimg : 0;
    add_images(prm, wc, scratch, c);
    // the textures of this evaluation stay in LDS (behind the frame region, which the evaluation itself uses) for setRefImage
    KeptTex kt;
    kt.texs = texs + MVS_FRAME1_LDS_BYTES / 4; kt.tstride = tstride; kt.ssd = 1.0f; kt.okm = 0u; kt.orig = wc.lane; kt.n_eval = 0;
    constraint_images(prm, wc, scratch, c, prm.nccThreshold, keep_w, keep_n, &kt);
    filter_images_by_angle(prm, wc, scratch, c, &kt);
    if (c.nimg < prm.minImageNum) return -1;
    set_grids(prm, wc, c);
    const int ref_before = rli(c.img, 0);
    set_ref_image(prm, wc, texs, tstride, c, &kt);
    // Same reference view as before: the second constraintImages would sample the very textures of the first one for
    // the views that passed it, under the same threshold, and remove nothing.  It runs when the reference changed.
    if (rli(c.img, 0) != ref_before) constraint_images(prm, wc, scratch, c, prm.nccThreshold);
    if (c.nimg < prm.minImageNum) return -1;
    set_grids(prm, wc, c);
    c.tmp = score2(c, prm.nccThreshold);
    if (prm.depth) set_vimages_vgrids(prm, wc, scratch, c);
    return 0;
}

// ------------------------------------------------------------------ record <-> registers
DEV void load_cand(const DPatch* p, const WaveCtx& wc, Cand& c) {
    c.coord = ld4(p->coord);
    c.normal = ld4(p->normal);
    c.ncc = p->ncc; c.dscale = p->dscale; c.ascale = p->ascale; c.tmp = p->tmp;
    c.nimg = min(p->nimages, MVS_LISTCAP);
    c.nvimg = min(p->nvimages, MVS_LISTCAP);
    c.img = (wc.lane < MVS_MAXI) ? (int)p->images[wc.lane] : 0;
    c.vimg = (wc.lane < MVS_MAXI) ? (int)p->vimages[wc.lane] : 0;
    c.gx = c.gy = c.vgx = c.vgy = 0;
}
DEV void store_cand(DPatch* p, const WaveCtx& wc, const Cand& c, int flags, int id) {
    if (wc.lane == 0) {
        p->coord[0] = c.coord.x; p->coord[1] = c.coord.y; p->coord[2] = c.coord.z; p->coord[3] = c.coord.w;
        p->normal[0] = c.normal.x; p->normal[1] = c.normal.y; p->normal[2] = c.normal.z; p->normal[3] = c.normal.w;
        p->ncc = c.ncc; p->dscale = c.dscale; p->ascale = c.ascale; p->tmp = c.tmp;
        p->nimages = c.nimg; p->nvimages = c.nvimg; p->flags = flags; p->id = id;
    }
    if (wc.lane < MVS_MAXI) {
        p->images[wc.lane] = (uint8_t)(wc.lane < c.nimg ? c.img : 0);
        p->vimages[wc.lane] = (uint8_t)(wc.lane < c.nvimg ? c.vimg : 0);
    }
}
DEV WaveCtx make_wave_ctx(const DParams& prm) {
    WaveCtx wc;
    wc.lane = lane_id();
    wc.cc = make_cls(prm, wc.lane);
    wc.evals = 0; wc.view_evals = 0;
#ifdef MVS_STAGE_TIMING
    for (int k = 0; k < 8; ++k) wc.st_acc[k] = 0;
    wc.st_t = 0;
#endif
    return wc;
}

// Propagate::generatePatch, propagate.cpp:220-237.  `src` is in registers (view lanes hold m_images).
// as_view >= 0 (view propagation): the patch is re-anchored on the ray of view `as_view` and Optim::swapImage
// (optim.cpp:385-395) makes that view the reference.
// need_ncc = false (engine schedule, destination cell not full): the initial score is only ever read by the
// replace-worst pre-filter (propagate.cpp:170); refinePatch overwrites it, so it is not computed when nothing reads it.
template <class WC>
DEV bool generate_patch(const DParams& prm, WC& wc, int* scratch, const Cand& src, F3 icoord, Cand& out, int as_view = -1, bool need_ncc = true) {
    int simg = src.img;
    if (as_view >= 0 && rli(src.img, 0) != as_view) {
        const unsigned long long hit = ballot(0 < wc.lane && wc.lane < src.nimg && src.img == as_view);
        if (hit == 0ull) return false;
        const int k = __ffsll((long long)hit) - 1, first = rli(src.img, 0);
        simg = wc.lane == 0 ? as_view : (wc.lane == k ? first : src.img);
    }
    const int image = rli(simg, 0);
    const DView* vw = prm.views + image;
    const float depth = dot4(ld4(vw->oaxis), src.coord);
    const F3 nic{depth * icoord.x, depth * icoord.y, depth * icoord.z};
    out.coord = unproject(vw, nic, prm.level);
    out.normal = src.normal;
    out.ncc = -1.0f; out.dscale = 0.0f; out.ascale = 0.0f; out.tmp = 0.0f;
    out.nvimg = 0; out.vimg = 0; out.vgx = 0; out.vgy = 0;
    // PatchManager::setGridsImages, patch_manager.cpp:223-239
    int ix = 0, iy = 0;
    bool keep = false;
    if (wc.lane < src.nimg) {
        const DView* v2 = prm.views + simg;
        cell_of(prm, v2, out.coord, ix, iy);
        keep = 0 <= ix && ix < v2->gw && 0 <= iy && iy < v2->gh;
    }
    out.img = simg; out.gx = ix; out.gy = iy;
    const unsigned long long m = ballot(keep);
    const int pos = __popcll(m & ((1ull << wc.lane) - 1ull));
    __syncthreads();
    if (keep) { scratch[pos] = out.img; scratch[64 + pos] = ix; scratch[128 + pos] = iy; }
    __syncthreads();
    out.nimg = __popcll(m);
    out.img = scratch[wc.lane]; out.gx = scratch[64 + wc.lane]; out.gy = scratch[128 + wc.lane];
    if (out.nimg == 0) return false;
    if (need_ncc) out.ncc = compute_ncc(prm, wc, out.coord, out.normal, out.img, out.nimg);
    return true;
}

}  // namespace mvsdev
