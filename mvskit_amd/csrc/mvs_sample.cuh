// mvs_sample.cuh -- how a wave samples texture windows: the sampling frame of a (patch, view) and its place in LDS, the per-wave context,
// the class-lane sample layout with its loads and blends, and the evaluation of the four proposals of a refinement step (one candidate's,
// or two candidates' side by side).
#pragma once
#include "mvs_types.h"
#include "mvs_math.cuh"
#include "mvs_wave.cuh"
#include "mvs_camera.cuh"

namespace mvsdev {

// ------------------------------------------------------------------ texture frames (frame lanes)
// Head of Optim::getTex, optim.cpp:790-818: per (proposal, view) the sampling frame (top-left, dx, dy), the
// pyramid level, and the base pointer / width of that level so that the sampling loop needs no further loads.
// A rejected view keeps ok = 0 and a harmless frame (the 2x2 texels at the origin of the view's own image), so
// that sampling can stay branch-free; its results are masked out by the caller.
struct Frame {
    float tlx, tly, dxx, dxy, dyx, dyy;
    int w;               // width of the chosen level
    int ok;              // 1 = the view passed the angle gate and getTexSafe
    // where the RGBA8 texels of the chosen level lie, in the form of the sampler that reads the frame (WaveCtx::narrow):
    //   narrow  a_lo = the level's byte offset in the pyramid block (DView::img_off), a_hi = its row pitch in bytes (4 w)
    //   wide    a_lo, a_hi = the halves of the level's address (DView::img)
    unsigned a_lo, a_hi;
};
// levelDiff = clamp(floor(log2(ratio) + .5)) (optim.cpp:808) as comparisons against 2^(k - .5), k = -3 .. 2 ("level
// pick").  Those six thresholds are ONE float mantissa (that of sqrt 2, 0x3504F3) under six exponents, so for ratio = 2^e * 1.m the
// largest k with ratio >= 2^(k - .5) is e + (m >= 0x3504F3): adding 0x800000 - 0x3504F3 to the bits carries into the exponent exactly
// then -- three integer instructions for six compares and selects; the clamp to [-4, 2] takes care of zero, tiny and huge ratios as
// the chain of comparisons does (a NaN ratio, which only a degenerate frame that is rejected anyway can produce, reads -4 there and
// 2 here).
DEV int level_diff(const DParams& prm, float ratio) {
    static_assert(0x3504F3 == (0x3FB504F3 & 0x7FFFFF), "mantissa of 1.414213562373095f");
    const int k = ((__float_as_int(ratio) + (0x800000 - 0x3504F3)) >> 23) - 127;
    const int ld = max(-4, min(2, k));
    return max(-prm.level, min(2, ld));
}
DEV float pow2_level(int ld) { return __int_as_float((127 + ld) << 23); }  // Optim::myPow2, exact powers of two
// Straight-line: every load of the view's constants is issued at the top (one wait instead of one per early exit --
// a lane that leaves early saves nothing while its neighbours go on), the gates only select the result.
// NARROW: the frame is for a sampler that addresses the pyramid block by 32-bit byte offsets (Frame::a_lo / a_hi)
template <bool NARROW = false>
DEV Frame make_frame(const DParams& prm, F4 coord, F4 px, F4 py, F4 pz, int v, bool active) {
    const DView* vw = prm.views + (active ? v : 0);
    const F4 ctr = ld4(vw->center);
    float P[12];
    load_P(vw, prm.level, P);
    const int W0 = vw->W[0], H0 = vw->H[0];
    const unsigned long long base_level = NARROW ? (unsigned long long)vw->img_off[prm.level] : (unsigned long long)vw->img[prm.level];
    const F4 ray = nrm4(sub4(ctr, coord));
    const float weight = fmaxf(0.0f, dot4(ray, pz));
    F3 center = project_regs(P, coord);
    F3 dx = sub3(project_regs(P, add4(coord, px)), center);
    F3 dy = sub3(project_regs(P, add4(coord, py)), center);
    const float ratio = (norm3(dx) + norm3(dy)) / 2.0f;
    const int ld = level_diff(prm, ratio);
    const float iscale = pow2_level(-ld);  // exact reciprocal of a power of two
    const int newLevel = prm.level + ld;
    // the one load that depends on the arithmetic
    const unsigned long long base_new = NARROW ? (unsigned long long)vw->img_off[newLevel] : (unsigned long long)vw->img[newLevel];
    center = scl3(center, iscale);
    dx = scl3(dx, iscale);
    dy = scl3(dy, iscale);
    // Optim::getTexSafe, optim.cpp:895-915
    // The four corners are (c -+ a) -+ b with a = dx * m, b = dy * m (each product rounded once, each sum rounded): all four sign
    // combinations.  Rounding is monotone, so the smallest of the four is (c - |a|) - |b| and the largest (c + |a|) + |b| -- the very
    // values the reference's min / max over the corners pick (optim.cpp:902-912), without forming the other three corners.
    const float m = (float)(prm.wsize / 2);
    const float ax = dx.x * m, bx = dy.x * m, ay = dx.y * m, by = dy.y * m;
    const float tlx = (center.x - ax) - bx, tly = (center.y - ay) - by;
    const float minx = (center.x - fabsf(ax)) - fabsf(bx), maxx = (center.x + fabsf(ax)) + fabsf(bx);
    const float miny = (center.y - fabsf(ay)) - fabsf(by), maxy = (center.y + fabsf(ay)) + fabsf(by);
    const int margin2 = 2;
    const int W = W0 >> newLevel, H = H0 >> newLevel;  // the pyramid halves (rounding down) at every level
    const bool inside = !(minx < margin2 || W - 1 - margin2 <= maxx || miny < margin2 || H - 1 - margin2 <= maxy);
    const bool ok = active && !(weight < prm.cosAngle1) && inside;
    Frame f;
    f.tlx = ok ? tlx : 0.0f; f.tly = ok ? tly : 0.0f;
    f.dxx = ok ? dx.x : 0.0f; f.dxy = ok ? dx.y : 0.0f; f.dyx = ok ? dy.x : 0.0f; f.dyy = ok ? dy.y : 0.0f;
    f.w = ok ? W : (W0 >> prm.level);
    f.ok = ok ? 1 : 0;
    const unsigned long long a = ok ? base_new : base_level;
    f.a_lo = (unsigned)(a & 0xffffffffull);
    f.a_hi = NARROW ? 4u * (unsigned)f.w : (unsigned)(a >> 32);
    return f;
}

struct __attribute__((packed, aligned(4))) Texel2 { uint32_t a, b; };

// Per-lane constants of the class-lane sample layout: lane 16 r + c owns samples c, c + 16, c + 32 of the window its row
// works on (a proposal in a refinement step, a view in a single evaluation).  A window of 16 k + 1 samples (7x7) has one
// sample more, the "extra" xbase, which the lane that owns the sampling frame takes.
struct ClsConst {
    unsigned cs[3];  // per slot j: fx | fy << 8 | valid << 16
    int fb;          // first lane of this lane's row (16 r)
    int xbase, nx;   // the extra: sample xbase if nx == 1 (wave-uniform)
    unsigned xcs;    // the extra's fx | fy << 8 | 1 << 16 (wave-uniform; meaningless if nx == 0)
};
// How a window of wsz samples falls on the three slots of a row's 16 lanes; make_cls on the device and the sweep's launcher on the host.
struct ClsLayout { int njx, lim, xbase, nx; };  // slots j < njx hold the samples q = c + 16 j < lim; the extra as in ClsConst
__host__ __device__ inline ClsLayout cls_layout(int wsz) {
    const int nj = wsz >> 4, rem = wsz & 15;
    return {nj + (rem > 1 ? 1 : 0), rem > 1 ? wsz : 16 * nj, 16 * nj, rem == 1 ? 1 : 0};
}
// Every slot of every lane holds a sample and the window has its extra (3 x 16 + 1 samples: 7x7).  The valid bit of a slot is then 1
// on every lane, and the arithmetic that applies it as a factor 1.0f is the identity: x * 1.0f, fma(-p, 1.0f, r) = r - p and
// 1.0f - dx1 round once either way, so code that leaves the factor out computes the same bits.
__host__ __device__ inline bool cls_full_window(int wsz) {
    const ClsLayout l = cls_layout(wsz);
    return l.njx >= 3 && l.lim >= 48 && l.nx == 1;
}
// Per-wave working state.
struct WaveCtx {
    static constexpr bool full_window = false, narrow = false;  // the generic window code and the wide samplers (WaveCtxT below)
    int lane;
    ClsConst cc;
    unsigned evals, view_evals;
#ifdef MVS_STAGE_TIMING
    unsigned long long st_acc[8];  // diagnostic build: phase times, kept in registers and flushed once by the kernel
    unsigned long long st_t;
#endif
};
// The same state in a launch whose window is full (cls_full_window) has full_window = true: the functions that sample are templates on the
// context's type and leave out the slot-mask arithmetic for it; everything else takes it as a WaveCtx.
// How a launch addresses the texels it samples is a property of the context's type as well.  WIDE (narrow = false, plain WaveCtx among
// them): a 64-bit address per lane, for a pyramid block of any size.  NARROW (narrow = true): the block's base, one value for the whole launch
// (DParams::pyr32, scalar registers), plus a 32-bit byte offset per lane -- the address arithmetic of a sample slot is then 32-bit
// (v_mad_u32_u24, v_lshl_add_u32, v_add_u32 in place of v_mad_u64_u32 and three v_lshl_add_u64) and the loads take the form
// global_load v, v_off, s[base].  The texels read are the same, so the results are.  The launcher picks a narrow instantiation where
// the block is below 4 GiB (DParams::pyr32 is set).  A Frame is made (make_frame) and consumed by functions of ONE context type.
template <bool FULL, bool NARROW> struct WaveCtxT : WaveCtx { static constexpr bool full_window = FULL, narrow = NARROW; };
#ifdef MVS_STAGE_TIMING
#define WC_T0(wc) { (wc).st_t = (unsigned long long)__builtin_amdgcn_s_memtime(); }
#define WC_ADD(wc, k) { const unsigned long long t1_ = (unsigned long long)__builtin_amdgcn_s_memtime(); (wc).st_acc[k] += t1_ - (wc).st_t; (wc).st_t = t1_; }
#else
#define WC_T0(wc)
#define WC_ADD(wc, k)
#endif

// The sampling frames of an evaluation are published in LDS (frames_publish) and read back by the sampling lanes: uniform
// or per-row ds_read_b128 instead of ten v_readlane_b32 per sample on the vector ALU, the unit this kernel saturates.
#define MVS_PIVOT_LDS4 192                         // float4 index of the per-view pivot colours (refinePatch, class lanes)
#define MVS_FRAME_LDS_BYTES (64 * 48 + 16 * 16)    // frame lanes 0..63, 12 dwords each, + 16 pivots; the start of the kernel's dynamic LDS
#define MVS_FRAME1_LDS_BYTES (48 * (MVS_LISTCAP > 16 ? MVS_LISTCAP : 16))  // what a single-proposal evaluation publishes there
extern __shared__ float4 mvs_dyn_lds4[];
DEV void frames_publish(const WaveCtx& wc, const Frame& f, int nlanes) {
    __syncthreads();  // whatever used the region before (setRefImage textures, Optim::check rows) is done
    if (wc.lane < nlanes) {
        float4* d = mvs_dyn_lds4 + 3 * wc.lane;
        d[0] = make_float4(f.tlx, f.tly, f.dxx, f.dxy);
        d[1] = make_float4(f.dyx, f.dyy, __int_as_float(f.w), __int_as_float(f.ok));
        d[2] = make_float4(__int_as_float((int)f.a_lo), __int_as_float((int)f.a_hi), 0.0f, 0.0f);
    }
    __syncthreads();
}
// second half of Optim::normalize, optim.cpp:932-939, on whatever lanes hold an ssd: 1 / msd
DEV float inv_msd(const DParams& prm, float ssd) {
    float msd = sqrt_rn(ssd * prm.inv_3sz);
    if (msd == 0.0f) msd = 1.0f;
    return rcp_rn(msd);
}

// ------------------------------------------------------------------ class-lane evaluation (the four proposals of a refinement step)
// Optim::getTex sampling + normalize + dot for proposals g = 0..3 against the views k < n, with a lane per (proposal,
// sample class) instead of a lane per sample: lane 16 g + c walks its samples c, c + 16, c + 32 of EVERY view and keeps
// running sums -- colour, colour^2 and colour x reference colour (the reference view's colours of its own samples stay in
// registers) -- so no sum crosses lanes per sample.  Per view the five sums are finished by the four DPP steps of a
// 16-lane row, once for all four proposals, and dropped into view lane 16 g + k; the per-view scalars (1/msd, INCC) then
// come out of one vector sequence.  A wave instruction of the view loop covers 64 samples.
// The few samples beyond the last full 16 ("extras": sample 48 of a 7x7 window) are taken afterwards by the FRAME lanes:
// lane 16 g + k samples them in its own frame (proposal g, view k) and adds them to the sums it has just received.
// Arithmetic (mirrored by the oracle, tex_stats_class16): colours are taken relative to a per-view pivot p (the view's
// mean colour in refinePatch's first evaluation), c' = blend - p;  S1 = sum c', S2 = sum |c'|^2, S01 = sum c' . c0';
// mean m = S1 / n;  ssd = max(S2 - S1 . m, 0);  dot = S01 - S1 . m0;  INCC = 1 - dot (inv0 inv) / 3n.  The sums run
// j-ascending inside a lane, the row tree pairs lanes 1, 2, 4, 8 apart, the extras are added last, in sample order.
struct ClsPend { Texel2 q0, q1; float dx1, dy1; };
DEV ClsConst make_cls(const DParams& prm, int lane) {
    ClsConst cc;
    const ClsLayout l = cls_layout(prm.wsz);
    const int row = lane >> 4, c = lane & 15;
    cc.fb = 16 * row;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int q = c + 16 * j;
        const bool valid = j < l.njx && q < l.lim;
        cc.cs[j] = valid ? (unsigned)(q % prm.wsize) | ((unsigned)(q / prm.wsize) << 8) | (1u << 16) : 0u;
    }
    cc.xbase = l.xbase; cc.nx = l.nx;
    cc.xcs = (unsigned)(l.xbase % prm.wsize) | ((unsigned)(l.xbase / prm.wsize) << 8) | (1u << 16);
    return cc;
}
DEV float cvt_ub0(unsigned x) { return (float)(x & 255u); }
DEV float cvt_ub1(unsigned x) { return (float)((x >> 8) & 255u); }
DEV float cvt_ub2(unsigned x) { return (float)((x >> 16) & 255u); }
// The sample constants are unpacked where they are used (three v_cvt_f32_ubyte): hoisted out of the refinement loop as nine
// floats they only turn into scratch traffic.  The empty asm hides the loop invariance from the optimiser.
DEV unsigned cls_opaque(unsigned x) { asm volatile("" : "+v"(x)); return x; }
struct ClsFrame { float tlx, tly, dxx, dxy, dyx, dyy; int w; unsigned a_lo, a_hi; };  // a_lo, a_hi: as in Frame
DEV ClsFrame cls_frame(int fidx) {
    const float4* s = mvs_dyn_lds4 + 3 * fidx;
    const float4 A = s[0], B = s[1];
    const float2 Cc = *reinterpret_cast<const float2*>(s + 2);
    ClsFrame f;
    f.tlx = A.x; f.tly = A.y; f.dxx = A.z; f.dxy = A.w; f.dyx = B.x; f.dyy = B.y; f.w = __float_as_int(B.z);
    f.a_lo = (unsigned)__float_as_int(Cc.x); f.a_hi = (unsigned)__float_as_int(Cc.y);
    return f;
}
DEV ClsFrame cls_frame_of(const Frame& f) {  // a frame lane's own frame (the extra sample)
    ClsFrame fr;
    fr.tlx = f.tlx; fr.tly = f.tly; fr.dxx = f.dxx; fr.dxy = f.dxy; fr.dyx = f.dyx; fr.dyy = f.dyy; fr.w = f.w;
    fr.a_lo = f.a_lo; fr.a_hi = f.a_hi;
    return fr;
}
// NARROW (WaveCtxT::narrow): pyr = DParams::pyr32, the launch's one base; the byte offsets of the two texel rows are formed in 32-bit unsigned
// arithmetic -- row number and pitch are below 2^24 and the block below 2^32 (mvs_engine_set_views), so the 24-bit multiply and the
// sums are exact -- and the address is the base plus the zero-extended offset, which the compiler turns into scalar-base loads.
template <bool NARROW> DEV const uint8_t* sampler_base(const DParams& prm) { return NARROW ? prm.pyr32 : nullptr; }
template <bool NARROW>
DEV ClsPend cls_issue(const uint8_t* pyr, const ClsFrame& f, unsigned cs) {
    typedef const __attribute__((address_space(1))) uint32_t* GlobalTexels;
    typedef const __attribute__((address_space(1))) uint8_t* GlobalBytes;
    // a slot without a sample has cs = 0: it reads the window's first texels (a valid address) and is weighted out in
    // cls_colour, so no select is needed here
    const float fx = cvt_ub0(cs), fy = cvt_ub1(cs);
    const float sx = fma_(f.dyx, fy, fma_(f.dxx, fx, f.tlx));
    const float sy = fma_(f.dyy, fy, fma_(f.dxy, fx, f.tly));
    const int lx = (int)sx, ly = (int)sy;
    GlobalTexels t0, t1;
    if (NARROW) {
        // (the empty asm keeps the row's offset one v_mad_u32_u24: reassociated, the sum costs a shift and a three-operand add more)
        unsigned row = __umul24((unsigned)ly, f.a_hi) + f.a_lo;
        asm("" : "+v"(row));
        const unsigned o0 = row + ((unsigned)lx << 2), o1 = o0 + f.a_hi;
        t0 = (GlobalTexels)((GlobalBytes)pyr + (unsigned long long)o0); t1 = (GlobalTexels)((GlobalBytes)pyr + (unsigned long long)o1);
    } else {
        const unsigned long long base = ((unsigned long long)f.a_hi << 32) | (unsigned long long)f.a_lo;
        const unsigned long long a0 = base + 4ull * (unsigned long long)(unsigned)(ly * f.w + lx);
        t0 = (GlobalTexels)a0; t1 = (GlobalTexels)(a0 + 4ull * (unsigned long long)(unsigned)f.w);
    }
    ClsPend p;
    p.q0.a = t0[0]; p.q0.b = t0[1];
    p.q1.a = t1[0]; p.q1.b = t1[1];
    // sx - (float)(int)sx for the non-negative positions getTexSafe lets through: one v_fract_f32 (exact)
    p.dx1 = __builtin_amdgcn_fractf(sx); p.dy1 = __builtin_amdgcn_fractf(sy);
    return p;
}
// bilinear blend (Image::getColor, image.cpp:447-472); 0 on lanes whose sample does not exist
// FULL (a full window, cls_full_window): the slot holds a sample, the factor below is 1.0f and is left out
template <bool FULL = false>
DEV void cls_raw(const ClsPend& p, unsigned cs, float& r, float& g, float& b) {
    const Texel2 q0 = p.q0, q1 = p.q1;
    const float fm = FULL ? 1.0f : cvt_ub2(cs);  // 1, or 0 for a slot without a sample: both column weights vanish, and with them all four
    const float dx1 = FULL ? p.dx1 : p.dx1 * fm, dx0 = fm - dx1, dy1 = p.dy1, dy0 = 1.0f - dy1;
    const float f00 = dx0 * dy0, f01 = dx0 * dy1, f10 = dx1 * dy0, f11 = dx1 * dy1;
    r = fma_((float)(q1.b & 255u), f11, fma_((float)(q0.b & 255u), f10, fma_((float)(q1.a & 255u), f01, (float)(q0.a & 255u) * f00)));
    g = fma_((float)((q1.b >> 8) & 255u), f11, fma_((float)((q0.b >> 8) & 255u), f10, fma_((float)((q1.a >> 8) & 255u), f01, (float)((q0.a >> 8) & 255u) * f00)));
    b = fma_((float)((q1.b >> 16) & 255u), f11, fma_((float)((q0.b >> 16) & 255u), f10, fma_((float)((q1.a >> 16) & 255u), f01, (float)((q0.a >> 16) & 255u) * f00)));
}
// the blend minus the pivot (which a slot without a sample does not have either)
template <bool FULL = false>
DEV void cls_colour(const ClsPend& p, unsigned cs, float pr, float pg, float pb, float& r, float& g, float& b) {
    cls_raw<FULL>(p, cs, r, g, b);
    if (FULL) { r = r - pr; g = g - pg; b = b - pb; }
    else { const float fm = cvt_ub2(cs); r = fma_(-pr, fm, r); g = fma_(-pg, fm, g); b = fma_(-pb, fm, b); }
}
// (bound_ctrl form: every lane has a source within its row, so no "old" value has to be provided)
#define MVS_ROW_STEP5(C) { const float t0 = dpp0_f<C>(s1r), t1 = dpp0_f<C>(s1g), t2 = dpp0_f<C>(s1b), t3 = dpp0_f<C>(s2), t4 = dpp0_f<C>(s01); \
                           s1r = s1r + t0; s1g = s1g + t1; s1b = s1b + t2; s2 = s2 + t3; s01 = s01 + t4; }
#define MVS_ROW_STEP4(C) { const float t0 = dpp0_f<C>(s1r), t1 = dpp0_f<C>(s1g), t2 = dpp0_f<C>(s1b), t3 = dpp0_f<C>(s2); \
                           s1r = s1r + t0; s1g = s1g + t1; s1b = s1b + t2; s2 = s2 + t3; }
// The INCC of a view against its reference view from the five sums a frame lane holds: mean, ssd and centred product of the lane's view;
// the reference view's mean and 1 / msd come from its frame lane, whose ds_bpermute address is a0.
DEV float cls_incc(const DParams& prm, int a0, float P1r, float P1g, float P1b, float P2, float P01) {
    const float m_r = P1r * prm.inv_sz, m_g = P1g * prm.inv_sz, m_b = P1b * prm.inv_sz;
    const float ssd = fmaxf(P2 - fma_(P1b, m_b, fma_(P1g, m_g, P1r * m_r)), 0.0f);
    const float inv_l = inv_msd(prm, ssd);
    const float m0r = bperm_f(a0, m_r), m0g = bperm_f(a0, m_g), m0b = bperm_f(a0, m_b), inv0 = bperm_f(a0, inv_l);
    const float dot = P01 - fma_(P1b, m0b, fma_(P1g, m0g, P1r * m0r));
    return 1.0f - (dot * (inv0 * inv_l)) * prm.inv_3sz;
}
// frames: published in LDS for frame lanes 16 g + k (frames_publish); okm[g] = views of proposal g that sample.
// Leaves in frame lane 16 g + k (k >= 1) the INCC of view k against the reference view of proposal g.
// Straight-line per view (always three sample slots per lane; a slot without a sample contributes exact zeros), the
// reference view peeled off, and the loads of view k + 1 issued as the slots of view k are consumed.
template <class WC>
DEV void eval_steps4(const DParams& prm, WC& wc, const ClsConst& cc, const Frame& f, int n, unsigned (&okm)[4], float& incc_l) {
    constexpr bool FULL = WC::full_window, NARROW = WC::narrow;
    const uint8_t* const pyr = sampler_base<NARROW>(prm);
    // (the extra's test stays a run-time one here even for a full window: known true, this loop's scalar reloads go from 17 to 20 -- DESIGN.md section 5)
    const bool has_x = cc.nx > 0;
    frames_publish(wc, f, 64);
    const unsigned long long okb = ballot(f.ok != 0);
#pragma unroll
    for (int g = 0; g < 4; ++g) okm[g] = (unsigned)((okb >> (16 * g)) & 0xffffull);
#pragma unroll
    for (int g = 0; g < 4; ++g) wc.view_evals += (okm[g] & 1u) ? (unsigned)__popc(okm[g]) : 0u;
    const int fb = cc.fb;
    const int lc = wc.lane & 15;
    float c0[3][3];
    ClsPend pend[3];
    float P1r, P1g, P1b, P2, P01 = 0.0f;
    const int vlast = max(n - 1, 0);
    {
        const ClsFrame fr = cls_frame(fb);
#pragma unroll
        for (int j = 0; j < 3; ++j) pend[j] = cls_issue<NARROW>(pyr, fr, cls_opaque(cc.cs[j]));
    }
    {   // the reference view
        const float4 pv = mvs_dyn_lds4[MVS_PIVOT_LDS4];
        const ClsFrame fn = cls_frame(fb + min(1, vlast));
        float s1r = 0.0f, s1g = 0.0f, s1b = 0.0f, s2 = 0.0f;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const unsigned cs = cls_opaque(cc.cs[j]);
            float r, g, b;
            cls_colour<FULL>(pend[j], cs, pv.x, pv.y, pv.z, r, g, b);
            pend[j] = cls_issue<NARROW>(pyr, fn, cs);
            c0[j][0] = r; c0[j][1] = g; c0[j][2] = b;
            s1r += r; s1g += g; s1b += b;
            s2 = fma_(r, r, s2); s2 = fma_(g, g, s2); s2 = fma_(b, b, s2);
        }
        MVS_ROW_STEP4(0xB1) MVS_ROW_STEP4(0x4E) MVS_ROW_STEP4(0x141) MVS_ROW_STEP4(0x140)
        P1r = s1r; P1g = s1g; P1b = s1b; P2 = s2;  // lanes lc != 0 are overwritten below or unused
    }
    for (int k = 1; k < n; ++k) {
        const float4 pv = mvs_dyn_lds4[MVS_PIVOT_LDS4 + k];
        const ClsFrame fn = cls_frame(fb + min(k + 1, vlast));
        float s1r = 0.0f, s1g = 0.0f, s1b = 0.0f, s2 = 0.0f, s01 = 0.0f;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const unsigned cs = cls_opaque(cc.cs[j]);
            float r, g, b;
            cls_colour<FULL>(pend[j], cs, pv.x, pv.y, pv.z, r, g, b);
            pend[j] = cls_issue<NARROW>(pyr, fn, cs);
            s1r += r; s1g += g; s1b += b;
            s2 = fma_(r, r, s2); s2 = fma_(g, g, s2); s2 = fma_(b, b, s2);
            s01 = fma_(r, c0[j][0], s01); s01 = fma_(g, c0[j][1], s01); s01 = fma_(b, c0[j][2], s01);
        }
        MVS_ROW_STEP5(0xB1) MVS_ROW_STEP5(0x4E) MVS_ROW_STEP5(0x141) MVS_ROW_STEP5(0x140)  // the row tree (lanes 1, 2, 4, 8 apart)
        if (lc == k) { P1r = s1r; P1g = s1g; P1b = s1b; P2 = s2; P01 = s01; }
    }
    const int a0 = (wc.lane & 48) << 2;  // ds_bpermute address of lane 16 g: the reference view of this lane's proposal
    // the extras: frame lane 16 g + k samples them in its own frame (a frame that does not sample holds a harmless address
    // and its sums are never looked at) and adds them to the sums of (proposal g, view k) it holds
    if (has_x) {
        const float4 pv = mvs_dyn_lds4[MVS_PIVOT_LDS4 + lc];
        const ClsFrame fr = cls_frame_of(f);
        {
            const unsigned cs = cc.xcs;
            const ClsPend pe = cls_issue<NARROW>(pyr, fr, cs);
            float r, g, b;
            cls_colour<FULL>(pe, cs, pv.x, pv.y, pv.z, r, g, b);
            const float r0 = bperm_f(a0, r), g0 = bperm_f(a0, g), b0 = bperm_f(a0, b);
            P1r += r; P1g += g; P1b += b;
            P2 = fma_(r, r, P2); P2 = fma_(g, g, P2); P2 = fma_(b, b, P2);
            P01 = fma_(r, r0, P01); P01 = fma_(g, g0, P01); P01 = fma_(b, b0, P01);
        }
    }
    incc_l = cls_incc(prm, a0, P1r, P1g, P1b, P2, P01);
}

// eval_steps4 for TWO candidates (refine_patch_pair): frame lane 16 g + 8 s + k holds the frame of (candidate s, proposal g, view k), k < n_s <= 8.
// One publication; the sampling -- the peeled reference view and the view loop, the very code above -- once per candidate, from the frames
// fb + 8 s + k and the pivots 8 s + k into the lanes lc == 8 s + k; then ONE pass of the extras, the per-view scalars (reference lane 16 g + 8 s)
// and, in the caller, the robust INCCs.  okm[s][g]: the views of (candidate s, proposal g) that sample; returns the same bits by frame lane.
// (The sampling and the extras are written out a second time: through a helper shared with eval_steps4 the code of the sweep and probe
// kernels moves; only the per-view scalars, cls_incc, are shared.)
template <class WC>
DEV unsigned long long eval_steps4_pair(const DParams& prm, WC& wc, const ClsConst& cc, const Frame& f, int n0, int n1, unsigned (&okm)[2][4], float& incc_l) {
    constexpr bool FULL = WC::full_window, NARROW = WC::narrow;
    const uint8_t* const pyr = sampler_base<NARROW>(prm);
    const bool has_x = FULL || cc.nx > 0;
    frames_publish(wc, f, 64);
    const unsigned long long okb = ballot(f.ok != 0);
#pragma unroll
    for (int g = 0; g < 4; ++g) { okm[0][g] = (unsigned)((okb >> (16 * g)) & 0xffull); okm[1][g] = (unsigned)((okb >> (16 * g + 8)) & 0xffull); }
#pragma unroll
    for (int g = 0; g < 4; ++g)
        wc.view_evals += ((okm[0][g] & 1u) ? (unsigned)__popc(okm[0][g]) : 0u) + ((okm[1][g] & 1u) ? (unsigned)__popc(okm[1][g]) : 0u);
    const int lc = wc.lane & 15;
    float P1r = 0.0f, P1g = 0.0f, P1b = 0.0f, P2 = 0.0f, P01 = 0.0f;
#pragma nounroll
    for (int s = 0; s < 2; ++s) {
        const int n = s ? n1 : n0;
        const int fb = cc.fb + 8 * s, pb = MVS_PIVOT_LDS4 + 8 * s, lb = 8 * s;
        float c0[3][3];
        ClsPend pend[3];
        const int vlast = max(n - 1, 0);
        {
            const ClsFrame fr = cls_frame(fb);
#pragma unroll
            for (int j = 0; j < 3; ++j) pend[j] = cls_issue<NARROW>(pyr, fr, cls_opaque(cc.cs[j]));
        }
        {   // the reference view
            const float4 pv = mvs_dyn_lds4[pb];
            const ClsFrame fn = cls_frame(fb + min(1, vlast));
            float s1r = 0.0f, s1g = 0.0f, s1b = 0.0f, s2 = 0.0f;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const unsigned cs = cls_opaque(cc.cs[j]);
                float r, g, b;
                cls_colour<FULL>(pend[j], cs, pv.x, pv.y, pv.z, r, g, b);
                pend[j] = cls_issue<NARROW>(pyr, fn, cs);
                c0[j][0] = r; c0[j][1] = g; c0[j][2] = b;
                s1r += r; s1g += g; s1b += b;
                s2 = fma_(r, r, s2); s2 = fma_(g, g, s2); s2 = fma_(b, b, s2);
            }
            MVS_ROW_STEP4(0xB1) MVS_ROW_STEP4(0x4E) MVS_ROW_STEP4(0x141) MVS_ROW_STEP4(0x140)
            if (lc >= lb) { P1r = s1r; P1g = s1g; P1b = s1b; P2 = s2; }  // this candidate's half; lanes lc != 8 s are overwritten below or unused
        }
        for (int k = 1; k < n; ++k) {
            const float4 pv = mvs_dyn_lds4[pb + k];
            const ClsFrame fn = cls_frame(fb + min(k + 1, vlast));
            float s1r = 0.0f, s1g = 0.0f, s1b = 0.0f, s2 = 0.0f, s01 = 0.0f;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const unsigned cs = cls_opaque(cc.cs[j]);
                float r, g, b;
                cls_colour<FULL>(pend[j], cs, pv.x, pv.y, pv.z, r, g, b);
                pend[j] = cls_issue<NARROW>(pyr, fn, cs);
                s1r += r; s1g += g; s1b += b;
                s2 = fma_(r, r, s2); s2 = fma_(g, g, s2); s2 = fma_(b, b, s2);
                s01 = fma_(r, c0[j][0], s01); s01 = fma_(g, c0[j][1], s01); s01 = fma_(b, c0[j][2], s01);
            }
            MVS_ROW_STEP5(0xB1) MVS_ROW_STEP5(0x4E) MVS_ROW_STEP5(0x141) MVS_ROW_STEP5(0x140)
            if (lc == lb + k) { P1r = s1r; P1g = s1g; P1b = s1b; P2 = s2; P01 = s01; }
        }
    }
    const int a0 = (wc.lane & 56) << 2;  // ds_bpermute address of lane 16 g + 8 s: the reference view of this lane's candidate and proposal
    if (has_x) {
        const float4 pv = mvs_dyn_lds4[MVS_PIVOT_LDS4 + lc];
        const ClsFrame fr = cls_frame_of(f);
        {
            const unsigned cs = cc.xcs;
            const ClsPend pe = cls_issue<NARROW>(pyr, fr, cs);
            float r, g, b;
            cls_colour<FULL>(pe, cs, pv.x, pv.y, pv.z, r, g, b);
            const float r0 = bperm_f(a0, r), g0 = bperm_f(a0, g), b0 = bperm_f(a0, b);
            P1r += r; P1g += g; P1b += b;
            P2 = fma_(r, r, P2); P2 = fma_(g, g, P2); P2 = fma_(b, b, P2);
            P01 = fma_(r, r0, P01); P01 = fma_(g, g0, P01); P01 = fma_(b, b0, P01);
        }
    }
    incc_l = cls_incc(prm, a0, P1r, P1g, P1b, P2, P01);
    return okb;
}
#undef MVS_ROW_STEP4
#undef MVS_ROW_STEP5

}  // namespace mvsdev
