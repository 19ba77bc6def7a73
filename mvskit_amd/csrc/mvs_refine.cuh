// mvs_refine.cuh -- Optim::refinePatch: the three coordinates of a patch and their cost, the halving random search for one candidate and
// for two of a cell side by side, and the bounded Nelder-Mead that runs to convergence.
#pragma once
#include "mvs_cand.cuh"

namespace mvsdev {

// ------------------------------------------------------------------ refinement
struct RefineCtx {
    F4 center, ray;
    float dscale, ascale;
    int ref;
};
// the bounds of the two angle coordinates (optim.cpp:496-506): every refiner clamps to them after every step
static constexpr float REFINE_AMIN = -23.99999f, REFINE_AMAX = 23.99999f;
// Optim::encode, optim.cpp:549-580
DEV void encode(const DParams& prm, const RefineCtx& rc, F4 coord, F4 normal, float* x) {
    x[0] = dot4(sub4(coord, rc.center), rc.ray) / rc.dscale;
    const DView* vw = prm.views + rc.ref;
    const F3 n3{normal.x, normal.y, normal.z};
    const float fx = dot3(ld3(vw->xaxis), n3), fy = dot3(ld3(vw->yaxis), n3), fz = dot3(ld3(vw->zaxis), n3);
    const float a2 = pm_asinf(fmaxf(-1.0f, fminf(1.0f, fy)));
    const float cosb = pm_cosf(a2);
    float a1;
    if (cosb == 0.0f) a1 = 0.0f;
    else {
        const float sina = fx / cosb, cosa = -fz / cosb;
        a1 = pm_acosf(fmaxf(-1.0f, fminf(1.0f, cosa)));
        if (sina < 0.0f) a1 = -a1;
    }
    x[1] = a1 / rc.ascale;
    x[2] = a2 / rc.ascale;
}
// Optim::decode, optim.cpp:582-599 (x0..x2 may differ per lane: frame lanes decode their own proposal)
DEV void decode(const DParams& prm, const RefineCtx& rc, float x0, float x1, float x2, F4& coord, F4& normal) {
    const float t = rc.dscale * x0;
    coord = {fma_(t, rc.ray.x, rc.center.x), fma_(t, rc.ray.y, rc.center.y), fma_(t, rc.ray.z, rc.center.z), fma_(t, rc.ray.w, rc.center.w)};
    const float angle1 = x1 * rc.ascale, angle2 = x2 * rc.ascale;
    float s1, c1, s2, c2;
    pm_sincosf(angle1, s1, c1);
    pm_sincosf(angle2, s2, c2);
    const float fx = s1 * c2, fy = s2, fz = -c1 * c2;
    const DView* vw = prm.views + rc.ref;
    normal = {fma_(vw->zaxis[0], fz, fma_(vw->yaxis[0], fy, vw->xaxis[0] * fx)),
              fma_(vw->zaxis[1], fz, fma_(vw->yaxis[1], fy, vw->xaxis[1] * fx)),
              fma_(vw->zaxis[2], fz, fma_(vw->yaxis[2], fy, vw->xaxis[2] * fx)), 0.0f};
}
// the mean of cost_func (optim.cpp:451-465) over the views of group g that sampled, in double, i ascending
DEV void sum_of_group(unsigned okm, float val_l, int g, int sz, double& ans, int& denom) {
    ans = 0.0;
    denom = 0;
    for (int i = 1; i < sz; ++i) {
        if (!((okm >> i) & 1u)) continue;
        ans += (double)rlf(val_l, 16 * g + i);
        denom++;
    }
}
DEV double cost_of_group(unsigned okm, float val_l, int g, int sz, int minimum) {
    if (!(okm & 1u)) return 2.0;
    double ans;
    int denom;
    sum_of_group(okm, val_l, g, sz, ans, denom);
    if (denom < minimum - 1) return 2.0;
    return ans / (double)denom;
}
// Optim::cost_func (optim.cpp:401-468) for up to four proposals at once: lane 16*g + i decodes proposal g
// (x0..x2 hold that lane's proposal), builds the patch axes and the frame of view i; then each proposal is
// evaluated in turn.  imgx = m_images replicated into every group of 16 lanes.
// rows (four proposals): bit g = proposal g is evaluated; a proposal left out samples nothing, costs 2 and is not counted.
template <class WC>
DEV void cost_func4(const DParams& prm, WC& wc, const RefineCtx& rc, int imgx, int n, bool four, float x0, float x1, float x2,
                    double (&fv)[4], float* piv = nullptr, const ClsConst* cc = nullptr, unsigned rows = 0xFu) {
    F4 coord, normal, px, py;
    decode(prm, rc, x0, x1, x2, coord, normal);
    get_paxes(prm, prm.views + rc.ref, coord, normal, px, py);
    const int sz = min(prm.tau, n);
    const int minimum = min(prm.minImageNum, sz);
    const int g = wc.lane >> 4, i = wc.lane & 15;
    const Frame f = make_frame<WC::narrow>(prm, coord, px, py, normal, imgx, (four ? ((rows >> g) & 1u) != 0u : g < 1) && i < sz);
    float incc_l;
    fv[1] = fv[2] = fv[3] = 2.0;
    if (four) {
        wc.evals += (unsigned)__popc(rows);
        unsigned okm[4];
        eval_steps4(prm, wc, *cc, f, sz, okm, incc_l);
        const float val_l = robustincc(incc_l);
        // the four means, lane j < 4 = proposal j: its views' robust INCCs come over from the frame lanes 16 j + i one by one
        // (ds_bpermute) and are added in the order of cost_func's loop (optim.cpp:451-465, i ascending, in double); one fp64
        // division for all four
        const int gl = wc.lane & 3;
        const unsigned okl = gl == 1 ? okm[1] : (gl == 2 ? okm[2] : (gl == 3 ? okm[3] : okm[0]));
        double num = 0.0;
        int den = 0;
        for (int i = 1; i < sz; ++i) {
            const float v = bperm_f(4 * (16 * gl + i), val_l);
            const bool ok = (okl >> i) & 1u;
            num = ok ? num + (double)v : num;
            den += ok ? 1 : 0;
        }
        const double q = num / (double)den;
#pragma unroll
        for (int j = 0; j < 4; ++j) fv[j] = ((okm[j] & 1u) && rli(den, j) >= minimum - 1) ? rld(q, j) : 2.0;
    } else {
        wc.evals += 1;
        vmask_t okm[1];
        if (piv) eval_views<true>(prm, wc, f, sz, okm, incc_l, piv);  // refinePatch's first evaluation: the view means become the pivots
        else eval_views(prm, wc, f, sz, okm, incc_l);
        const float val_l = robustincc(incc_l);
        fv[0] = cost_of_group((unsigned)okm[0], val_l, 0, sz, minimum);  // sz <= tau <= 16 views
    }
}
// Optim::refinePatch, optim.cpp:480-547, BOBYQA replaced by the halving random search
// w_out != nullptr (inside the sweep): the weights go out and the final m_ncc is left to postProcess
// (The head down to the publication of the pivots is written out in all three refiners, and the step's proposals here and in
// refine_patch_pair: through a shared helper either moves the code of the sweep and probe kernels.)
template <class WC>
DEV void refine_patch(const DParams& prm, WC& wc, Cand& c, uint32_t k0, uint32_t k1, uint32_t k2, uint32_t k3, float* w_out = nullptr) {
    RefineCtx rc;
    rc.center = c.coord;
    rc.ref = rli(c.img, 0);
    rc.ray = nrm4(sub4(c.coord, ld4((prm.views + rc.ref)->center)));
    rc.dscale = c.dscale;
    rc.ascale = prm.ascaleConst;
    const float w = compute_weights(prm, wc, c.coord, c.normal, c.img, c.nimg);
    const int imgx = __shfl(c.img, wc.lane & 15);
    float x[3];
    encode(prm, rc, c.coord, c.normal, x);
    x[1] = fmaxf(fminf(x[1], REFINE_AMAX), REFINE_AMIN);
    x[2] = fmaxf(fminf(x[2], REFINE_AMAX), REFINE_AMIN);
    float bx0 = x[0], bx1 = x[1], bx2 = x[2];
    double fv[4];
    float piv[3] = {128.0f, 128.0f, 128.0f};  // view lanes: the mean colour of view k at the starting point
    cost_func4(prm, wc, rc, imgx, c.nimg, false, bx0, bx1, bx2, fv, piv);
    __syncthreads();
    if (wc.lane < 16) mvs_dyn_lds4[MVS_PIVOT_LDS4 + wc.lane] = make_float4(piv[0], piv[1], piv[2], 0.0f);
    __syncthreads();
    double fbest = fv[0];
    const ClsConst cc = wc.cc;
    float rd = prm.rd0, ra = prm.ra0;
    const int g = wc.lane >> 4;  // this lane's proposal: 0 depth only, 1 angles only, 2 both, 3 both mirrored about the step's start
    const uint32_t gj = (uint32_t)min(g, 2);
    for (int k = 0; k < prm.refine_steps; ++k) {
        const uint32_t draw = 16u + ((uint32_t)(k * 3) + gj) * 3u;
        const float u0 = 2.0f * rng_uniform(prm.seed, k0, k1, k2, k3, draw + 0);
        const float u1 = 2.0f * rng_uniform(prm.seed, k0, k1, k2, k3, draw + 1);
        const float u2 = 2.0f * rng_uniform(prm.seed, k0, k1, k2, k3, draw + 2);
        float cx0 = (gj == 1u) ? bx0 : fma_(u0, rd, bx0);
        float cx1 = (gj == 0u) ? bx1 : fmaxf(fminf(fma_(u1, ra, bx1), REFINE_AMAX), REFINE_AMIN);
        float cx2 = (gj == 0u) ? bx2 : fmaxf(fminf(fma_(u2, ra, bx2), REFINE_AMAX), REFINE_AMIN);
        if (g == 3) {
            cx0 = bx0 - (cx0 - bx0);
            cx1 = fmaxf(fminf(bx1 - (cx1 - bx1), REFINE_AMAX), REFINE_AMIN);
            cx2 = fmaxf(fminf(bx2 - (cx2 - bx2), REFINE_AMAX), REFINE_AMIN);
        }
        cost_func4(prm, wc, rc, imgx, c.nimg, true, cx0, cx1, cx2, fv, nullptr, &cc);
        int jb = 0;
        double fstep = fv[0];
#pragma unroll
        for (int j = 1; j < 4; ++j) if (fv[j] < fstep) { fstep = fv[j]; jb = j; }
        if (fstep < fbest) { fbest = fstep; bx0 = rlf(cx0, 16 * jb); bx1 = rlf(cx1, 16 * jb); bx2 = rlf(cx2, 16 * jb); }
        rd *= 0.5f; ra *= 0.5f;
    }
    x[0] = bx0; x[1] = bx1; x[2] = bx2;
    decode(prm, rc, x[0], x[1], x[2], c.coord, c.normal);
    c.normal.w = 0.0f;
    if (w_out) *w_out = w;
    else c.ncc = 1.0f - unrobustincc(compute_incc(prm, wc, c.coord, c.normal, c.img, c.nimg, w, 1));
}

// ------------------------------------------------------------------ two candidates in one refinement
// A candidate that waits for a partner (sweep_cell) lies in a static LDS block of MVS_PEND_INTS ints: the scalars of its Cand, the three
// view-lane arrays a candidate has before postProcess (m_images and their cells; the m_vimages side is empty until then), and the weights
// of its refinement once it ran.  Behind them, the working block of a pair's refinement: per candidate s the 16 values a frame lane takes
// each step (RefineCtx, the step's starting point, the prefix of the draws' key, min(tau, nimg)) and m_images at 8 s + k.
#define MVS_PEND_IMG 16
#define MVS_PEND_GX 80
#define MVS_PEND_GY 144
#define MVS_PEND_W 208
#define MVS_PEND_CTX 272   // 2 x 16 floats, 16-byte aligned
#define MVS_PEND_XIMG 304  // 16 ints
#define MVS_PEND_INTS 320
DEV void pend_store(int* st, const WaveCtx& wc, const Cand& c, float w) {
    __syncthreads();
    if (wc.lane == 0) {
        float* f = reinterpret_cast<float*>(st);
        f[0] = c.coord.x; f[1] = c.coord.y; f[2] = c.coord.z; f[3] = c.coord.w;
        f[4] = c.normal.x; f[5] = c.normal.y; f[6] = c.normal.z; f[7] = c.normal.w;
        f[8] = c.ncc; f[9] = c.dscale; f[10] = c.ascale; f[11] = c.tmp;
        st[12] = c.nimg; st[13] = c.nvimg;
    }
    st[MVS_PEND_IMG + wc.lane] = c.img; st[MVS_PEND_GX + wc.lane] = c.gx; st[MVS_PEND_GY + wc.lane] = c.gy;
    st[MVS_PEND_W + wc.lane] = __float_as_int(w);
    __syncthreads();
}
DEV void pend_load(const int* st, const WaveCtx& wc, Cand& c, float& w) {
    const float* f = reinterpret_cast<const float*>(st);
    c.coord = {rff(f[0]), rff(f[1]), rff(f[2]), rff(f[3])};
    c.normal = {rff(f[4]), rff(f[5]), rff(f[6]), rff(f[7])};
    c.ncc = rff(f[8]); c.dscale = rff(f[9]); c.ascale = rff(f[10]); c.tmp = rff(f[11]);
    c.nimg = rfl(st[12]); c.nvimg = rfl(st[13]);
    c.img = st[MVS_PEND_IMG + wc.lane]; c.gx = st[MVS_PEND_GX + wc.lane]; c.gy = st[MVS_PEND_GY + wc.lane];
    c.vimg = 0; c.vgx = 0; c.vgy = 0;
    w = __int_as_float(st[MVS_PEND_W + wc.lane]);
}
// cost_func4 for the four proposals of TWO candidates: lane 16 g + 8 s + k decodes proposal g of candidate s (rc, imgx, szl and x0..x2 are
// that lane's), builds its patch axes and the frame of view k < szl = min(tau, nimg) of candidate s (<= 8).  fv[s][g]: the cost of proposal g
// of candidate s -- the eight means in lanes j < 8 (candidate j >> 2, proposal j & 3), added in cost_func's order, one fp64 division.
template <class WC>
DEV void cost_func4_pair(const DParams& prm, WC& wc, const RefineCtx& rc, int imgx, int sz0, int sz1, int szl, float x0, float x1, float x2,
                         double (&fv)[2][4], const ClsConst& cc) {
    F4 coord, normal, px, py;
    decode(prm, rc, x0, x1, x2, coord, normal);
    get_paxes<true>(prm, prm.views + rc.ref, coord, normal, px, py);
    const Frame f = make_frame<WC::narrow>(prm, coord, px, py, normal, imgx, (wc.lane & 7) < szl);
    wc.evals += 8u;
    unsigned okm[2][4];
    float incc_l;
    const unsigned long long okb = eval_steps4_pair(prm, wc, cc, f, sz0, sz1, okm, incc_l);
    const float val_l = robustincc(incc_l);
    // lane j < 8 takes the mean of candidate j >> 2, proposal j & 3, whose frame lanes start at src.  (Taken from an opaque copy of the
    // lane number: as a loop invariant of the whole kernel the address only turns into a spilled register.)
    const int src = (int)(((cls_opaque((unsigned)wc.lane) & 3u) << 4) | ((cls_opaque((unsigned)wc.lane) & 4u) << 1));
    const unsigned okl = (unsigned)(okb >> src) & 0xffu;
    double num = 0.0;
    int den = 0;
    const int szm = max(sz0, sz1);  // a view beyond a candidate's own list never samples: its bit is clear
    for (int i = 1; i < szm; ++i) {
        const float v = bperm_f(4 * (src + i), val_l);
        const bool ok = (okl >> i) & 1u;
        num = ok ? num + (double)v : num;
        den += ok ? 1 : 0;
    }
    const double q = num / (double)den;
    const int min0 = min(prm.minImageNum, sz0), min1 = min(prm.minImageNum, sz1);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        fv[0][j] = ((okm[0][j] & 1u) && rli(den, j) >= min0 - 1) ? rld(q, j) : 2.0;
        fv[1][j] = ((okm[1][j] & 1u) && rli(den, 4 + j) >= min1 - 1) ? rld(q, 4 + j) : 2.0;
    }
}
// refine_patch for two candidates of one cell at once (sweep_cell): candidate 0 is the one stashed at st (pend_store), candidate 1 is c1; both
// have min(tau, nimg) <= 8.  Per candidate every value and every operation is refine_patch's, with that candidate's draws (k3a / k3b); what
// changes is where the work of the frame lanes runs -- decode, getPAxes, the frames, the extra sample, the per-view scalars, the robust
// INCCs and the cost means are issued once for both, candidate s in lanes 16 g + 8 s + k (refine_patch leaves the lanes 16 g + 8 .. 15 idle).
// Leaves the refined coord / normal of candidate 0 and its weights in the stash, those of candidate 1 in c1 and w1.
template <class WC>
DEV void refine_patch_pair(const DParams& prm, WC& wc, int* st, Cand& c1, uint32_t k0, uint32_t k1, uint32_t k2, uint32_t k3a, uint32_t k3b, float& w1) {
    float* const ctx = reinterpret_cast<float*>(st + MVS_PEND_CTX);
    int* const ximg = st + MVS_PEND_XIMG;
    double fbest0 = 2.0, fbest1 = 2.0;
    int sz0 = 0, sz1 = 0;
    w1 = 0.0f;
#pragma nounroll
    for (int s = 0; s < 2; ++s) {  // the first evaluation, which also gives the pivots, candidate after candidate
        F4 coord = c1.coord, normal = c1.normal;
        float dscale = c1.dscale;
        int img = c1.img, nimg = c1.nimg;
        if (s == 0) {
            const float* f = reinterpret_cast<const float*>(st);
            coord = {rff(f[0]), rff(f[1]), rff(f[2]), rff(f[3])};
            normal = {rff(f[4]), rff(f[5]), rff(f[6]), rff(f[7])};
            dscale = rff(f[9]); nimg = rfl(st[12]);
            img = st[MVS_PEND_IMG + wc.lane];
        }
        RefineCtx rc;
        rc.center = coord;
        rc.ref = rli(img, 0);
        rc.ray = nrm4(sub4(coord, ld4((prm.views + rc.ref)->center)));
        rc.dscale = dscale;
        rc.ascale = prm.ascaleConst;
        const float w = compute_weights(prm, wc, coord, normal, img, nimg);
        if (s == 0) st[MVS_PEND_W + wc.lane] = __float_as_int(w);
        else w1 = w;
        float x[3];
        encode(prm, rc, coord, normal, x);
        x[1] = fmaxf(fminf(x[1], REFINE_AMAX), REFINE_AMIN);
        x[2] = fmaxf(fminf(x[2], REFINE_AMAX), REFINE_AMIN);
        double fv[4];
        float piv[3] = {128.0f, 128.0f, 128.0f};
        cost_func4(prm, wc, rc, __shfl(img, wc.lane & 15), nimg, false, x[0], x[1], x[2], fv, piv);
        __syncthreads();
        if (wc.lane < 8) {
            mvs_dyn_lds4[MVS_PIVOT_LDS4 + 8 * s + wc.lane] = make_float4(piv[0], piv[1], piv[2], 0.0f);
            ximg[8 * s + wc.lane] = img;
        }
        const int sz = min(prm.tau, nimg);
        if (wc.lane == 0) {
            float* d = ctx + 16 * s;
            d[0] = rc.center.x; d[1] = rc.center.y; d[2] = rc.center.z; d[3] = rc.center.w;
            d[4] = rc.ray.x; d[5] = rc.ray.y; d[6] = rc.ray.z; d[7] = rc.ray.w;
            d[8] = rc.dscale; d[9] = __int_as_float(rc.ref); d[10] = x[0]; d[11] = x[1]; d[12] = x[2];
            d[13] = __int_as_float((int)rng_prefix(prm.seed, k0, k1, k2, s ? k3b : k3a)); d[14] = __int_as_float(sz); d[15] = 0.0f;
        }
        if (s == 0) { fbest0 = fv[0]; sz0 = sz; } else { fbest1 = fv[0]; sz1 = sz; }
    }
    __syncthreads();
    const ClsConst cc = wc.cc;
    float rd = prm.rd0, ra = prm.ra0;
    const int g = wc.lane >> 4;
    const uint32_t gj = (uint32_t)min(g, 2);
    const float4* const my = reinterpret_cast<const float4*>(ctx + 16 * ((wc.lane >> 3) & 1));
    for (int k = 0; k < prm.refine_steps; ++k) {
        const float4 A = my[0], B = my[1], Cq = my[2], D = my[3];  // this lane's candidate, from LDS every step: nothing of it stays in registers
        RefineCtx rc;
        rc.center = {A.x, A.y, A.z, A.w};
        rc.ray = {B.x, B.y, B.z, B.w};
        rc.dscale = Cq.x; rc.ref = __float_as_int(Cq.y); rc.ascale = prm.ascaleConst;
        const float bx0 = Cq.z, bx1 = Cq.w, bx2 = D.x;
        const uint32_t hp = (uint32_t)__float_as_int(D.y);
        const int szl = __float_as_int(D.z);
        const int imgx = ximg[wc.lane & 15];
        const uint32_t draw = 16u + ((uint32_t)(k * 3) + gj) * 3u;
        const float u0 = 2.0f * rng_tail(hp, draw + 0);
        const float u1 = 2.0f * rng_tail(hp, draw + 1);
        const float u2 = 2.0f * rng_tail(hp, draw + 2);
        float cx0 = (gj == 1u) ? bx0 : fma_(u0, rd, bx0);
        float cx1 = (gj == 0u) ? bx1 : fmaxf(fminf(fma_(u1, ra, bx1), REFINE_AMAX), REFINE_AMIN);
        float cx2 = (gj == 0u) ? bx2 : fmaxf(fminf(fma_(u2, ra, bx2), REFINE_AMAX), REFINE_AMIN);
        if (g == 3) {
            cx0 = bx0 - (cx0 - bx0);
            cx1 = fmaxf(fminf(bx1 - (cx1 - bx1), REFINE_AMAX), REFINE_AMIN);
            cx2 = fmaxf(fminf(bx2 - (cx2 - bx2), REFINE_AMAX), REFINE_AMIN);
        }
        double fv[2][4];
        cost_func4_pair(prm, wc, rc, imgx, sz0, sz1, szl, cx0, cx1, cx2, fv, cc);
        __syncthreads();  // every lane has read its candidate's block
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            int jb = 0;
            double fstep = fv[s][0];
#pragma unroll
            for (int j = 1; j < 4; ++j) if (fv[s][j] < fstep) { fstep = fv[s][j]; jb = j; }
            const double fb = s ? fbest1 : fbest0;
            if (fstep < fb) {
                if (s) fbest1 = fstep; else fbest0 = fstep;
                const float n0 = rlf(cx0, 16 * jb + 8 * s), n1 = rlf(cx1, 16 * jb + 8 * s), n2 = rlf(cx2, 16 * jb + 8 * s);
                if (wc.lane == 0) { ctx[16 * s + 10] = n0; ctx[16 * s + 11] = n1; ctx[16 * s + 12] = n2; }
            }
        }
        __syncthreads();
        rd *= 0.5f; ra *= 0.5f;
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const float* d = ctx + 16 * s;
        RefineCtx rc;
        rc.center = {rff(d[0]), rff(d[1]), rff(d[2]), rff(d[3])};
        rc.ray = {rff(d[4]), rff(d[5]), rff(d[6]), rff(d[7])};
        rc.dscale = rff(d[8]); rc.ref = rfl(__float_as_int(d[9])); rc.ascale = prm.ascaleConst;
        F4 coord, normal;
        decode(prm, rc, rff(d[10]), rff(d[11]), rff(d[12]), coord, normal);
        normal.w = 0.0f;
        if (s) { c1.coord = coord; c1.normal = normal; }
        else if (wc.lane == 0) {
            float* f = reinterpret_cast<float*>(st);
            f[0] = coord.x; f[1] = coord.y; f[2] = coord.z; f[3] = coord.w;
            f[4] = normal.x; f[5] = normal.y; f[6] = normal.z; f[7] = normal.w;
        }
    }
    __syncthreads();
}

// Optim::refinePatch run to convergence (mvs_refiner CONVERGED): a bounded Nelder-Mead over the same three
// variables.  A simplex in three variables has four vertices, one per proposal row: row g holds vertex g (vx0..vx2, its cost vf)
// and every decision is taken on values read back from lanes 0, 16, 32, 48 -- wave-uniform.  One pass per iteration evaluates
// the four trials for the worst vertex w: reflection, expansion, outside and inside contraction, c + k d with k = 1, 2, 1/2, -1/2,
// c = ((v_a + v_b) + v_c) / 3 over the other three vertices in ascending slot order, d = c - v_w (float32, no fused operations;
// tests/refiner_restatement.py restates it in this order).  If no trial is accepted the other three vertices shrink towards the
// best one, v_j = v_b + 0.5 (v_j - v_b): one more pass, three rows.  Angle coordinates are clamped to the bounds of
// optim.cpp:496-506 after every step.  Stop: every coordinate's spread over the simplex <= xtol * max(1, |x_best,i|) (converged),
// or the next pass would take the evaluations beyond max_evals (NLopt's MAXEVAL_REACHED: the reference counts that a failure and
// leaves the patch as it was, optim.cpp:530-545).  Returns the evaluations made, negated when the budget ran out; x_out / f_out:
// the best vertex and its cost.  w_out as refine_patch.
template <class WC>
DEV int refine_patch_simplex(const DParams& prm, WC& wc, Cand& c, int max_evals, float xtol, float* w_out = nullptr,
                               float* x_out = nullptr, double* f_out = nullptr) {
    RefineCtx rc;
    rc.center = c.coord;
    rc.ref = rli(c.img, 0);
    rc.ray = nrm4(sub4(c.coord, ld4((prm.views + rc.ref)->center)));
    rc.dscale = c.dscale;
    rc.ascale = prm.ascaleConst;
    const float w = compute_weights(prm, wc, c.coord, c.normal, c.img, c.nimg);
    const int imgx = __shfl(c.img, wc.lane & 15);
    float x[3];
    encode(prm, rc, c.coord, c.normal, x);
    x[1] = fmaxf(fminf(x[1], REFINE_AMAX), REFINE_AMIN);
    x[2] = fmaxf(fminf(x[2], REFINE_AMAX), REFINE_AMIN);
    double fv[4];
    float piv[3] = {128.0f, 128.0f, 128.0f};  // as refine_patch: the first evaluation publishes the class-lane pivots
    cost_func4(prm, wc, rc, imgx, c.nimg, false, x[0], x[1], x[2], fv, piv);
    __syncthreads();
    if (wc.lane < 16) mvs_dyn_lds4[MVS_PIVOT_LDS4 + wc.lane] = make_float4(piv[0], piv[1], piv[2], 0.0f);
    __syncthreads();
    const double f0 = fv[0];
    const ClsConst cc = wc.cc;
    const int g = wc.lane >> 4;
    // the start simplex: x, x + rd0 e0, x + ra0 e1, x + ra0 e2 (rows 1..3 in one pass, row 0 idle)
    float vx0 = g == 1 ? x[0] + prm.rd0 : x[0];
    float vx1 = g == 2 ? fmaxf(fminf(x[1] + prm.ra0, REFINE_AMAX), REFINE_AMIN) : x[1];
    float vx2 = g == 3 ? fmaxf(fminf(x[2] + prm.ra0, REFINE_AMAX), REFINE_AMIN) : x[2];
    cost_func4(prm, wc, rc, imgx, c.nimg, true, vx0, vx1, vx2, fv, nullptr, &cc, 0xEu);
    double vf = g == 0 ? f0 : (g == 1 ? fv[1] : (g == 2 ? fv[2] : fv[3]));
    int evals = 4;
    bool ok = false;
    int b = 0;
    for (;;) {
        double f[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) f[j] = rld(vf, 16 * j);
        b = 0;
        int wv = 0;  // best: lowest cost, lowest slot on a tie; worst: highest cost, highest slot on a tie
#pragma unroll
        for (int j = 1; j < 4; ++j) {
            if (f[j] < (b == 1 ? f[1] : (b == 2 ? f[2] : f[0]))) b = j;
            if (f[j] >= (wv == 1 ? f[1] : (wv == 2 ? f[2] : f[0]))) wv = j;
        }
        const float b0 = rlf(vx0, 16 * b), b1 = rlf(vx1, 16 * b), b2 = rlf(vx2, 16 * b);
        {
            float lo0 = rlf(vx0, 0), hi0 = lo0, lo1 = rlf(vx1, 0), hi1 = lo1, lo2 = rlf(vx2, 0), hi2 = lo2;
#pragma unroll
            for (int j = 1; j < 4; ++j) {
                const float a0 = rlf(vx0, 16 * j), a1 = rlf(vx1, 16 * j), a2 = rlf(vx2, 16 * j);
                lo0 = fminf(lo0, a0); hi0 = fmaxf(hi0, a0);
                lo1 = fminf(lo1, a1); hi1 = fmaxf(hi1, a1);
                lo2 = fminf(lo2, a2); hi2 = fmaxf(hi2, a2);
            }
            if (hi0 - lo0 <= xtol * fmaxf(1.0f, fabsf(b0)) && hi1 - lo1 <= xtol * fmaxf(1.0f, fabsf(b1)) &&
                hi2 - lo2 <= xtol * fmaxf(1.0f, fabsf(b2))) { ok = true; break; }
        }
        if (evals + 4 > max_evals) break;
        const double fb = rld(vf, 16 * b), fw = rld(vf, 16 * wv);
        double fsw = wv == 0 ? f[1] : f[0];  // the highest cost of the other three
#pragma unroll
        for (int j = 0; j < 4; ++j) if (j != wv) fsw = fmax(fsw, f[j]);
        const int r0 = wv == 0 ? 1 : 0, r1 = wv <= 1 ? 2 : 1, r2 = wv <= 2 ? 3 : 2;
        const float c0 = ((rlf(vx0, 16 * r0) + rlf(vx0, 16 * r1)) + rlf(vx0, 16 * r2)) / 3.0f;
        const float c1 = ((rlf(vx1, 16 * r0) + rlf(vx1, 16 * r1)) + rlf(vx1, 16 * r2)) / 3.0f;
        const float c2 = ((rlf(vx2, 16 * r0) + rlf(vx2, 16 * r1)) + rlf(vx2, 16 * r2)) / 3.0f;
        const float d0 = c0 - rlf(vx0, 16 * wv), d1 = c1 - rlf(vx1, 16 * wv), d2 = c2 - rlf(vx2, 16 * wv);
        const float k = g == 0 ? 1.0f : (g == 1 ? 2.0f : (g == 2 ? 0.5f : -0.5f));  // this row's trial
        const float t0 = c0 + k * d0;
        const float t1 = fmaxf(fminf(c1 + k * d1, REFINE_AMAX), REFINE_AMIN);
        const float t2 = fmaxf(fminf(c2 + k * d2, REFINE_AMAX), REFINE_AMIN);
        cost_func4(prm, wc, rc, imgx, c.nimg, true, t0, t1, t2, fv, nullptr, &cc);
        evals += 4;
        int acc = -1;  // Nelder-Mead's sequential rules on the four costs
        if (fv[0] < fb) acc = fv[1] < fv[0] ? 1 : 0;
        else if (fv[0] < fsw) acc = 0;
        else if (fv[0] < fw) acc = fv[2] <= fv[0] ? 2 : -1;
        else acc = fv[3] < fw ? 3 : -1;
        if (acc >= 0) {
            const float a0 = rlf(t0, 16 * acc), a1 = rlf(t1, 16 * acc), a2 = rlf(t2, 16 * acc);
            const double fa = acc == 0 ? fv[0] : (acc == 1 ? fv[1] : (acc == 2 ? fv[2] : fv[3]));
            if (g == wv) { vx0 = a0; vx1 = a1; vx2 = a2; vf = fa; }
            continue;
        }
        if (evals + 3 > max_evals) break;
        if (g != b) {  // shrink towards the best vertex
            vx0 = b0 + 0.5f * (vx0 - b0);
            vx1 = fmaxf(fminf(b1 + 0.5f * (vx1 - b1), REFINE_AMAX), REFINE_AMIN);
            vx2 = fmaxf(fminf(b2 + 0.5f * (vx2 - b2), REFINE_AMAX), REFINE_AMIN);
        }
        cost_func4(prm, wc, rc, imgx, c.nimg, true, vx0, vx1, vx2, fv, nullptr, &cc, 0xFu & ~(1u << b));
        evals += 3;
        if (g != b) vf = g == 0 ? fv[0] : (g == 1 ? fv[1] : (g == 2 ? fv[2] : fv[3]));
    }
    const float xb0 = rlf(vx0, 16 * b), xb1 = rlf(vx1, 16 * b), xb2 = rlf(vx2, 16 * b);
    if (x_out) { x_out[0] = xb0; x_out[1] = xb1; x_out[2] = xb2; }
    if (f_out) *f_out = rld(vf, 16 * b);
    if (ok) {
        decode(prm, rc, xb0, xb1, xb2, c.coord, c.normal);
        c.normal.w = 0.0f;
        if (!w_out) c.ncc = 1.0f - unrobustincc(compute_incc(prm, wc, c.coord, c.normal, c.img, c.nimg, w, 1));
    }
    if (w_out) *w_out = w;
    return ok ? evals : -evals;
}

}  // namespace mvsdev
