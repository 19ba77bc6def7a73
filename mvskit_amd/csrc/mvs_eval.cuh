// mvs_eval.cuh -- the single evaluation: one patch against the n views of its list, four views a round, with the Gram matrix of the
// centred textures taken on the matrix cores in the 32- and 64-view builds.
#pragma once
#include "mvs_sample.cuh"

namespace mvsdev {

// ------------------------------------------------------------------ class-lane evaluation of ONE patch against n views
// Every single evaluation (computeINCC, setINCCs, constraintImages, the first cost_func of refinePatch, setRefImage's
// textures): frame lane k < n holds the sampling frame of view k.  The four 16-lane rows take four views at a time --
// row r of round t samples view 4 t + r, lane 16 r + c its samples c, c + 16, c + 32 -- and the frame lanes take the
// extra sample of their own view beforehand.  Optim::normalize and Optim::dot in two passes as the reference has them:
// channel means (lane sums, row tree, extra), centring, then sum of squares and product with the centred reference
// texture (same order).  The reference view is view 0 = row 0 of round 0; its centred colours reach the other rows
// through ds_bpermute once, after which every row holds them for the samples it owns.
// The per-view scalars of view v are formed in lane 16 (v & 3) + (v >> 2) and moved to view lane v at the end.
// Leaves in view lane k >= 1 the INCC of view k against the reference view, okm[0] = views that sampled.
// PIV: piv[0..2] receive, in view lane k, the channel means of view k (128 for a view that was not sampled) -- the
// pivots of the class-lane steps that follow in refinePatch.
// texs != nullptr: the centred texture of view k goes to LDS, texs[3 k tstride + 3 sample + channel], and *ssd_out
// receives, in view lane k, its sum of squares -- what Optim::setRefImage needs.
#define MVS_ROW_STEP3(C) { const float t0 = dpp0_f<C>(s1r), t1 = dpp0_f<C>(s1g), t2 = dpp0_f<C>(s1b); s1r = s1r + t0; s1g = s1g + t1; s1b = s1b + t2; }
#define MVS_ROW_STEP2(C) { const float t0 = dpp0_f<C>(sq), t1 = dpp0_f<C>(dt); sq = sq + t0; dt = dt + t1; }

#define MVS_PAIR_MFMA (MVS_LISTCAP > 16)  // setRefImage's pair sums on the matrix cores (the 32- and 64-view builds)
#if MVS_PAIR_MFMA
// The Gram matrix G[a][b] = sum(k) t_a[k] t_b[k] of the kept textures is taken WHILE the views are sampled, in chunks of 16 views, so
// that only one chunk of textures lies in LDS at a time (the textures of a whole 32- or 64-view list were what held these builds at one
// or two waves per SIMD).  Every 16 x 16 tile runs down the k-ordered chain acc = fma(t_a[k], t_b[k], acc), which is what
// v_mfma_f32_16x16x4_f32 computes (37 of them for a 7 x 7 window).  G then replaces the textures in LDS (prm.gram_ld floats per row).
// The MFMA operands of a finished chunk go to PRIVATE memory -- a dynamically indexed per-lane array, i.e. the compiler's scratch
// segment: L1 / L2 resident, no slot bookkeeping, each lane reads back exactly what it wrote -- and come back eight k-steps at a time:
//   MVS_GRAM_SCRATCH 1 (the 32-view build): the tiles of a chunk with the earlier chunks are taken as soon as the chunk is sampled,
//     the accumulators of all tiles (3 x 4 registers) stay in registers until the list is through;
//   MVS_GRAM_SCRATCH 2 (the 64-view build): nothing of the matrix lives in registers while the views are sampled -- all chunks'
//     operands go out, and when the list is through the (up to 10) tiles are taken one after the other from there (4 accumulator
//     registers): 44 spilled registers at three waves per SIMD where the first form spills 146.
// Rounds 3-4 kept chunk A (half the list) in 37 / 74 registers while chunk B was sampled: the 64-view build then needed the 256 VGPRs
// and the 22 KB of LDS of two waves per SIMD and ran at 11.5 M patches/s on 48 x 540p; 13.6 M with form 1, 14.5 M with form 2
// (gpurun_out/r04l, r04m); the 32-view build 17.4 M either way, 16.6 M with form 2.
#define MVS_GRAM_SCRATCH (MVS_LISTCAP > 32 ? 2 : 1)
#define MVS_GRAM_CH 16
#define MVS_GRAM_NCH (MVS_LISTCAP / 16)                          // chunks at most: 2 or 4
#define MVS_GRAM_NT (MVS_GRAM_NCH * (MVS_GRAM_NCH + 1) / 2)     // tiles (p <= c): 3 or 10
#define MVS_GRAM_KSP 40                                         // MVS_GRAM_KS rounded up to groups of 8 k-steps
#define MVS_GRAM_T(p, c) ((c) * ((c) + 1) / 2 + (p))
#define MVS_GRAM_KK 4                                           // k values per MFMA (16x16x4)
#define MVS_GRAM_KS ((147 + MVS_GRAM_KK - 1) / MVS_GRAM_KK)      // MFMAs per tile for a 7x7 window (3 * 49 elements): 37
#define MVS_GRAM_NACC 4                                         // accumulator registers of a tile
typedef float gram_acc_t __attribute__((ext_vector_type(MVS_GRAM_NACC)));
DEV gram_acc_t gram_mfma(float a, float b, gram_acc_t c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
// accumulator register r of lane l holds tile element (row, col)
DEV int gram_col(int lane) { return lane & 15; }
DEV int gram_row(int lane, int r) { return (lane >> 4) * 4 + r; }
template <int N> struct GramIC { static constexpr int value = N; };
#endif
template <bool PIV = false, class WC>
DEV void eval_views(const DParams& prm, WC& wc, const Frame& f, int n, vmask_t (&okm)[1], float& incc_l, float* piv = nullptr,
                    float* texs = nullptr, int tstride = 0, float* ssd_out = nullptr) {
#if MVS_PAIR_MFMA
    // texs != nullptr: the Gram matrix of the centred textures is left at texs[a * LD + b] (see MVS_GRAM_CH above)
#if MVS_GRAM_SCRATCH == 2
    float gops[MVS_GRAM_NCH * MVS_GRAM_KSP];           // private memory: the MFMA operands of ALL chunks (lane l: t_{l % 16}[4 s + l / 16])
#elif MVS_GRAM_SCRATCH
    gram_acc_t gacc[MVS_GRAM_NT];                      // tile (p, c), p <= c, at MVS_GRAM_T(p, c)
    float gops[(MVS_GRAM_NCH - 1) * MVS_GRAM_KSP];     // private memory: the MFMA operands of the finished chunks (lane l: t_{l % 16}[4 s + l / 16])
#pragma unroll
    for (int q = 0; q < MVS_GRAM_NT; ++q)
#pragma unroll
        for (int r = 0; r < MVS_GRAM_NACC; ++r) gacc[q][r] = 0.0f;
#endif
    const int gK = 3 * prm.wsz, gtp = 3 * tstride;
    const int gk0 = wc.lane / MVS_GRAM_CH;                       // this lane's k within an MFMA
    const float* const grow = texs + (wc.lane & (MVS_GRAM_CH - 1)) * gtp;  // this lane's view of the chunk in LDS
#endif
    constexpr bool FULL = WC::full_window, NARROW = WC::narrow;
    const uint8_t* const pyr = sampler_base<NARROW>(prm);
    const ClsConst& cc = wc.cc;
    const bool has_x = FULL || cc.nx > 0;
    frames_publish(wc, f, MVS_LISTCAP > 16 ? MVS_LISTCAP : 16);
    okm[0] = vballot(f.ok != 0);  // a frame is only ever valid on a lane < n <= MVS_LISTCAP
    wc.view_evals += (okm[0] & 1u) ? (unsigned)vpop(okm[0]) : 0u;
    const int row = wc.lane >> 4, lc = wc.lane & 15;
    // the extra sample of view k in frame lane k (raw colours): its loads go out first, the first round's behind them
    float fxr = 0.0f, fxg = 0.0f, fxb = 0.0f;
    unsigned xcs = 0u;
    ClsPend pe;
    if (has_x) {
        const ClsFrame fr = cls_frame_of(f);
        xcs = cc.xcs;
        pe = cls_issue<NARROW>(pyr, fr, xcs);
    }
    float d0[3][3], d0x[3] = {0.0f, 0.0f, 0.0f};
    float ssd_l = 1.0f, dot_l = 0.0f, mr_l = 128.0f, mg_l = 128.0f, mb_l = 128.0f;
    ClsPend pend[3];
    {
        const int last = max(n - 1, 0);  // an empty list never reaches this point; the clamps below stay inside the frames all the same
        const ClsFrame fr = cls_frame(min(row, last));
#pragma unroll
        for (int j = 0; j < 3; ++j) pend[j] = cls_issue<NARROW>(pyr, fr, cls_opaque(cc.cs[j]));
    }
    if (has_x) cls_raw<FULL>(pe, xcs, fxr, fxg, fxb);
    const int rounds = (n + 3) >> 2;
    auto round_body = [&](const int t) {
        const int v = 4 * t + row, vq = min(v, max(n - 1, 0));
        const ClsFrame fn = cls_frame(min(v + 4, max(n - 1, 0)));
        float cr[3], cg[3], cb[3];
        float s1r = 0.0f, s1g = 0.0f, s1b = 0.0f;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const unsigned cs = cls_opaque(cc.cs[j]);
            cls_raw<FULL>(pend[j], cs, cr[j], cg[j], cb[j]);
            pend[j] = cls_issue<NARROW>(pyr, fn, cs);
            s1r += cr[j]; s1g += cg[j]; s1b += cb[j];
        }
        MVS_ROW_STEP3(0xB1) MVS_ROW_STEP3(0x4E) MVS_ROW_STEP3(0x141) MVS_ROW_STEP3(0x140)
        float xr = 0.0f, xg = 0.0f, xb = 0.0f;
        if (has_x) {
            xr = bperm_f(4 * vq, fxr); xg = bperm_f(4 * vq, fxg); xb = bperm_f(4 * vq, fxb);
            s1r += xr; s1g += xg; s1b += xb;
        }
        const float mr = s1r * prm.inv_sz, mg = s1g * prm.inv_sz, mb = s1b * prm.inv_sz;
        float er[3], eg[3], eb[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            if (FULL) { er[j] = cr[j] - mr; eg[j] = cg[j] - mg; eb[j] = cb[j] - mb; }
            else {
                const float fm = cvt_ub2(cls_opaque(cc.cs[j]));
                er[j] = fma_(-mr, fm, cr[j]); eg[j] = fma_(-mg, fm, cg[j]); eb[j] = fma_(-mb, fm, cb[j]);
            }
        }
        const float exr = xr - mr, exg = xg - mg, exb = xb - mb;
        if (t == 0) {  // the centred reference texture: from row 0 to every row
            const int a0 = 4 * lc;
#pragma unroll
            for (int j = 0; j < 3; ++j) { d0[j][0] = bperm_f(a0, er[j]); d0[j][1] = bperm_f(a0, eg[j]); d0[j][2] = bperm_f(a0, eb[j]); }
            if (has_x) { d0x[0] = bperm_f(0, exr); d0x[1] = bperm_f(0, exg); d0x[2] = bperm_f(0, exb); }
        }
        float sq = 0.0f, dt = 0.0f;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            sq += fma_(eb[j], eb[j], fma_(eg[j], eg[j], er[j] * er[j]));
            dt += fma_(d0[j][2], eb[j], fma_(d0[j][1], eg[j], d0[j][0] * er[j]));
        }
        MVS_ROW_STEP2(0xB1) MVS_ROW_STEP2(0x4E) MVS_ROW_STEP2(0x141) MVS_ROW_STEP2(0x140)
        if (has_x) {
            sq += fma_(exb, exb, fma_(exg, exg, exr * exr));
            dt += fma_(d0x[2], exb, fma_(d0x[1], exg, d0x[0] * exr));
        }
        if (lc == t) { ssd_l = sq; dot_l = dt; if (PIV) { mr_l = mr; mg_l = mg; mb_l = mb; } }
#if MVS_PAIR_MFMA
        if (texs) {  // sample-major: element 3 q + channel of the view's row of 3 * tstride floats (the k order of the pair sums); slot = view % CH
            float* tv = texs + (3 * (v & (MVS_GRAM_CH - 1))) * tstride;
            const bool have = v < n;  // rows without a view hold zeros: their products vanish and are never looked at
#pragma unroll
            for (int j = 0; j < 3; ++j)
                if (cc.cs[j] >> 16) { const int q = 3 * (lc + 16 * j); tv[q] = have ? er[j] : 0.0f; tv[q + 1] = have ? eg[j] : 0.0f; tv[q + 2] = have ? eb[j] : 0.0f; }
            if (has_x && lc == 0) { tv[3 * cc.xbase] = have ? exr : 0.0f; tv[3 * cc.xbase + 1] = have ? exg : 0.0f; tv[3 * cc.xbase + 2] = have ? exb : 0.0f; }
        }
#else
        if (texs && v < n) {  // sample-major: element 3 q + channel of view v's row of 3 * tstride floats (the k order of the pair sums)
            float* tv = texs + (3 * v) * tstride;
#pragma unroll
            for (int j = 0; j < 3; ++j)
                if (cc.cs[j] >> 16) { const int q = 3 * (lc + 16 * j); tv[q] = er[j]; tv[q + 1] = eg[j]; tv[q + 2] = eb[j]; }
            if (has_x && lc == 0) { tv[3 * cc.xbase] = exr; tv[3 * cc.xbase + 1] = exg; tv[3 * cc.xbase + 2] = exb; }
        }
#endif
    };
#if MVS_PAIR_MFMA && MVS_GRAM_SCRATCH == 2
    // Variant: NOTHING of the Gram matrix lives in registers while the views are sampled.  A finished chunk's operands go to private
    // memory; when the list is through, the tiles are taken one after the other from there (four accumulator registers) and written
    // to LDS over the textures.
    if (texs) {
        int ch = 0;
        for (int t = 0; t < rounds; ++t) {
            round_body(t);
            if ((t & 3) == 3 || t + 1 == rounds) {
                const int rc = (t & 3) + 1;
                __syncthreads();
                for (int vz = 4 * rc + (wc.lane >> 4); vz < MVS_GRAM_CH; vz += 4)
                    for (int q = lc; q < gtp; q += 16) texs[vz * gtp + q] = 0.0f;
                __syncthreads();
#pragma unroll 1
                for (int s0 = 0; s0 < MVS_GRAM_KSP; s0 += 8) {
                    float tb[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int k = MVS_GRAM_KK * (s0 + j) + gk0;
                        tb[j] = (s0 + j < MVS_GRAM_KS && k < gK) ? grow[k] : 0.0f;
                    }
#pragma unroll
                    for (int j = 0; j < 8; ++j) gops[ch * MVS_GRAM_KSP + s0 + j] = tb[j];
                }
                __syncthreads();
                ++ch;
            }
        }
        const int LD = prm.gram_ld, col = gram_col(wc.lane);
#pragma unroll 1
        for (int c2 = 0; c2 < ch; ++c2) {
#pragma unroll 1
            for (int pq = 0; pq <= c2; ++pq) {
                gram_acc_t acc;
#pragma unroll
                for (int r = 0; r < MVS_GRAM_NACC; ++r) acc[r] = 0.0f;
#pragma unroll 1
                for (int s0 = 0; s0 < MVS_GRAM_KSP; s0 += 8) {
                    float a8[8], b8[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) { a8[j] = gops[pq * MVS_GRAM_KSP + s0 + j]; b8[j] = gops[c2 * MVS_GRAM_KSP + s0 + j]; }
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        if (s0 + j < MVS_GRAM_KS) acc = gram_mfma(a8[j], b8[j], acc);
                }
#pragma unroll
                for (int r = 0; r < MVS_GRAM_NACC; ++r) {
                    const int rw = gram_row(wc.lane, r);
                    texs[(MVS_GRAM_CH * pq + rw) * LD + MVS_GRAM_CH * c2 + col] = acc[r];
                    if (pq != c2) texs[(MVS_GRAM_CH * c2 + col) * LD + MVS_GRAM_CH * pq + rw] = acc[r];
                }
            }
        }
        // rows / columns of chunks the list never reached are never read (set_ref_image reads indices < n_eval)
        __syncthreads();
    } else
        for (int t = 0; t < rounds; ++t) round_body(t);
#elif MVS_PAIR_MFMA && MVS_GRAM_SCRATCH
    // chunk C is complete after `rc` rounds of its own (or the list ends inside it): its diagonal tile from LDS, its tiles with the
    // earlier chunks p < C (their operands back from private memory, eight k-steps in flight), and its own operands out
    auto chunk_done = [&](auto Cc, const int rc) {
        constexpr int C = decltype(Cc)::value;
        __syncthreads();
        // rows of the chunk that no round wrote (the list ends inside it) must read as zeros
        for (int vz = 4 * rc + (wc.lane >> 4); vz < MVS_GRAM_CH; vz += 4)
            for (int q = lc; q < gtp; q += 16) texs[vz * gtp + q] = 0.0f;
        __syncthreads();
#pragma unroll 1
        for (int s0 = 0; s0 < MVS_GRAM_KSP; s0 += 8) {
            float tb[8], ap[C > 0 ? C : 1][8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = MVS_GRAM_KK * (s0 + j) + gk0;
                tb[j] = (s0 + j < MVS_GRAM_KS && k < gK) ? grow[k] : 0.0f;
#pragma unroll
                for (int pq = 0; pq < C; ++pq) ap[pq][j] = gops[pq * MVS_GRAM_KSP + s0 + j];
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (s0 + j < MVS_GRAM_KS) {  // wave-uniform
                    gacc[MVS_GRAM_T(C, C)] = gram_mfma(tb[j], tb[j], gacc[MVS_GRAM_T(C, C)]);
#pragma unroll
                    for (int pq = 0; pq < C; ++pq) gacc[MVS_GRAM_T(pq, C)] = gram_mfma(ap[pq][j], tb[j], gacc[MVS_GRAM_T(pq, C)]);
                }
            }
            if (C < MVS_GRAM_NCH - 1) {
#pragma unroll
                for (int j = 0; j < 8; ++j) gops[C * MVS_GRAM_KSP + s0 + j] = tb[j];
            }
        }
        __syncthreads();
    };
    if (texs) {
        int ch = 0;
        for (int t = 0; t < rounds; ++t) {
            round_body(t);
            if ((t & 3) == 3 || t + 1 == rounds) {
                const int rc = (t & 3) + 1;
                switch (ch) {
                    case 0: chunk_done(GramIC<0>{}, rc); break;
                    case 1: chunk_done(GramIC<1>{}, rc); break;
#if MVS_GRAM_NCH > 2
                    case 2: chunk_done(GramIC<2>{}, rc); break;
                    default: chunk_done(GramIC<3>{}, rc); break;
#else
                    default: break;
#endif
                }
                ++ch;
            }
        }
        // the tiles to LDS over the textures: G[a][b], a and b in the order of this evaluation's list (LD = prm.gram_ld columns)
        __syncthreads();
        const int LD = prm.gram_ld, col = gram_col(wc.lane);
#pragma unroll
        for (int c2 = 0; c2 < MVS_GRAM_NCH; ++c2) {
            if (MVS_GRAM_CH * c2 >= LD) continue;  // chunks the data set's list length never reaches (wave-uniform)
#pragma unroll
            for (int pq = 0; pq <= c2; ++pq) {
#pragma unroll
                for (int r = 0; r < MVS_GRAM_NACC; ++r) {
                    const int rw = gram_row(wc.lane, r);
                    const float gv = gacc[MVS_GRAM_T(pq, c2)][r];
                    texs[(MVS_GRAM_CH * pq + rw) * LD + MVS_GRAM_CH * c2 + col] = gv;
                    if (pq != c2) texs[(MVS_GRAM_CH * c2 + col) * LD + MVS_GRAM_CH * pq + rw] = gv;
                }
            }
        }
        __syncthreads();
    } else
        for (int t = 0; t < rounds; ++t) round_body(t);
#else
    for (int t = 0; t < rounds; ++t) round_body(t);
#endif
    // lane 16 (v & 3) + (v >> 2): 1 / msd and the INCC of view v; then to view lane v
    const float inv_l = inv_msd(prm, ssd_l);
    const float inv0 = rlf(inv_l, 0);
    const float incc_v = 1.0f - (dot_l * (inv0 * inv_l)) * prm.inv_3sz;
    const int src = 4 * (16 * (wc.lane & 3) + ((wc.lane >> 2) & 15));
    incc_l = bperm_f(src, incc_v);
    if (ssd_out) *ssd_out = bperm_f(src, ssd_l);
    if (PIV) {
        const bool okk = (okm[0] >> (wc.lane & (MVS_VBITS - 1))) & 1u;
        const float a0 = bperm_f(src, mr_l), a1 = bperm_f(src, mg_l), a2 = bperm_f(src, mb_l);
        piv[0] = (wc.lane < MVS_VBITS && okk) ? a0 : 128.0f; piv[1] = (wc.lane < MVS_VBITS && okk) ? a1 : 128.0f; piv[2] = (wc.lane < MVS_VBITS && okk) ? a2 : 128.0f;
    }
}
#undef MVS_ROW_STEP2
#undef MVS_ROW_STEP3

}  // namespace mvsdev
