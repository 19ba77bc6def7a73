// mvs_maps.hip -- dense per-view depth / normal / confidence maps and their cross-view fusion (mvs_engine_render_maps and
// mvs_engine_fused_points in mvs_engine.cpp drive it; the definitions are in include/mvskit_engine.h).  PatchMatch keeps a plane per
// cell: the dense map of a view is that plane cut by the ray of every pixel of the cell.
//   k_maps_select   source 0, all views in one pass over the pool: per cell of a patch's reference view the key of k_best_ncc_map
//                   (highest m_ncc, the lowest id among equals), written with atomicMax -- the only atomic of this file
//   k_maps_render   a wave per 8 x 8 pixel tile of one view: the selected patch's plane cut by the pixel's ray -> the id and the point
//   k_maps_agree    a lane per pixel of one view, looping over the other views: the agree word; and the view's depth / normal / conf maps
//   k_maps_flag     the pixels of one view that count: valid ones (n_valid), or the ones mvs_engine_fused_points emits
//   k_maps_expand   a byte per pixel back to the int32 the scan takes
//   k_maps_gather   the 32-byte records of the flagged pixels behind the exclusive scan of the flags: (view, y, x) order
// Arithmetic as everywhere in the engine: fp32, no contraction, dot products as left-to-right fmaf chains.  Every comparison that decides
// validity or agreement is written so that a NaN fails it.  Stores are plain vector stores.
#include <hip/hip_runtime.h>

#include "mvs_camera.cuh"
#include "mvs_common.cuh"
#include "mvs_kernels.h"

using namespace mvsdev;

DEV bool maps_finite_nonzero(float a) { return fabsf(a) > 0.0f && fabsf(a) < __int_as_float(0x7f800000); }
DEV float maps_qnan() { return __int_as_float(0x7fc00000); }

// k_best_ncc_map's rule for every view at once: sel[cell_base(v) + cell] over the alive patches whose reference view is v
__global__ __launch_bounds__(256) void k_maps_select(DParams prm, unsigned long long* __restrict__ sel) {
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= prm.pool_n) return;
    const DPatch* p = prm.pool + id;
    if (!(p->flags & 1) || p->nimages == 0) return;
    const int view = p->images[0];
    if (view >= prm.nviews) return;
    const DView* vw = prm.views + view;
    int ix, iy;
    cell_of(prm, vw, ld4(p->coord), ix, iy);
    if (ix < 0 || vw->gw <= ix || iy < 0 || vw->gh <= iy) return;
    const unsigned long long key = ((unsigned long long)sortable_f32(p->ncc) << 32) | (unsigned long long)(0xffffffffu - (uint32_t)id);
    atomicMax(&sel[vw->cell_base + iy * vw->gw + ix], key);
}

// Four waves a block, side by side; wave w of block (bx, by) takes the tile (4 bx + w, by), lane l its pixel (l & 7, l >> 3): the
// csize^2 pixels of a cell read the same 32 bytes of coord and normal.  Minv, the centre and oaxis come through uniform loads (`view` is a
// kernel argument).  ids / pts: the view's own slices.
__global__ __launch_bounds__(256) void k_maps_render(DParams prm, int view, int source, const unsigned long long* __restrict__ sel,
                                                     int32_t* __restrict__ ids, float* __restrict__ pts) {
    const DView* vw = prm.views + view;
    const int W = vw->W[prm.level], H = vw->H[prm.level];
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    const int x = ((int)blockIdx.x * 4 + wave) * 8 + (lane & 7), y = (int)blockIdx.y * 8 + (lane >> 3);
    if (x >= W || y >= H) return;
    const size_t pix = (size_t)y * W + x;
    int32_t id = -1;
    F3 X{maps_qnan(), maps_qnan(), maps_qnan()};
    const int cx = x / prm.csize, cy = y / prm.csize;
    bool have = cx < vw->gw && cy < vw->gh;
    if (have && vw->mask && vw->mask[pix] == 0) have = false;
    if (have) {
        const unsigned long long k = sel[vw->cell_base + cy * vw->gw + cx];
        have = source == 0 ? (k != 0ull) : (k != ~0ull);
        const uint32_t sid = source == 0 ? 0xffffffffu - (uint32_t)(k & 0xffffffffull) : (uint32_t)(k & 0xffffffffull);
        if (have && (int64_t)sid < prm.pool_n) {
            const DPatch* p = prm.pool + sid;
            const F4 X0 = ld4(p->coord), n4 = ld4(p->normal);
            const F3 n{n4.x, n4.y, n4.z};
            const float* M = vw->Minv;
            const F4 C = ld4(vw->center);
            const float fx = (float)x, fy = (float)y;
            const F3 dir{fma_(M[2], 1.0f, fma_(M[1], fy, M[0] * fx)), fma_(M[5], 1.0f, fma_(M[4], fy, M[3] * fx)),
                         fma_(M[8], 1.0f, fma_(M[7], fy, M[6] * fx))};
            const float nd = dot3(n, dir);
            const float num = dot3(n, F3{X0.x - C.x, X0.y - C.y, X0.z - C.z});
            const float t = num / nd;
            const F3 Xp{fma_(t, dir.x, C.x), fma_(t, dir.y, C.y), fma_(t, dir.z, C.z)};
            const float depth = dot4(ld4(vw->oaxis), F4{Xp.x, Xp.y, Xp.z, 1.0f});
            if (maps_finite_nonzero(nd) && t > 0.0f && depth > 0.0f && depth < __int_as_float(0x7f800000)) {
                id = (int32_t)sid;
                X = Xp;
            }
        }
    }
    ids[pix] = id;
    pts[3 * pix] = X.x; pts[3 * pix + 1] = X.y; pts[3 * pix + 2] = X.z;
}

// One lane per pixel of `view`; the loop over the other views is wave-uniform, so their projection and centre are uniform loads; the id map
// and the 32 bytes of geometry of the patch met are gathers.  ids / pts: all views, view u's slice at a.pix_base[u].  agree, depth,
// normal, conf: the view's own maps, any of them null.
__global__ __launch_bounds__(256) void k_maps_agree(DParams prm, MapsArgs a, int view, const int32_t* __restrict__ ids, const float* __restrict__ pts,
                                                    unsigned long long* __restrict__ agree, float* __restrict__ depth, float* __restrict__ normal,
                                                    float* __restrict__ conf) {
    const DView* vw = prm.views + view;
    const int64_t npix = (int64_t)vw->W[prm.level] * vw->H[prm.level];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npix) return;
    const int64_t pix = a.pix_base[view] + i;
    const int32_t id = ids[pix];
    if (id < 0) {
        if (agree) agree[i] = 0ull;
        if (depth) depth[i] = maps_qnan();
        if (normal) normal[3 * i] = normal[3 * i + 1] = normal[3 * i + 2] = maps_qnan();
        if (conf) conf[i] = maps_qnan();
        return;
    }
    const DPatch* p = prm.pool + id;
    const F3 X{pts[3 * pix], pts[3 * pix + 1], pts[3 * pix + 2]};
    const F3 n{p->normal[0], p->normal[1], p->normal[2]};
    if (depth) depth[i] = dot4(ld4(vw->oaxis), F4{X.x, X.y, X.z, 1.0f});
    if (normal) { normal[3 * i] = n.x; normal[3 * i + 1] = n.y; normal[3 * i + 2] = n.z; }
    if (conf) conf[i] = p->ncc;
    if (!agree) return;
    unsigned long long bits = 0ull;
    for (int u = 0; u < prm.nviews; ++u) {
        if (u == view) continue;
        const DView* uw = prm.views + u;
        const int Wu = uw->W[prm.level], Hu = uw->H[prm.level];
        const F3 ic = project(uw, F4{X.x, X.y, X.z, 1.0f}, prm.level);
        const float fx = floorf(ic.x + 0.5f), fy = floorf(ic.y + 0.5f);
        if (!(ic.z > 0.0f && fx >= 0.0f && fx < (float)Wu && fy >= 0.0f && fy < (float)Hu)) continue;
        const int32_t idq = ids[a.pix_base[u] + (int64_t)(int)fy * Wu + (int)fx];
        if (idq < 0) continue;
        const DPatch* q = prm.pool + idq;
        const F4 X0q = ld4(q->coord), nq4 = ld4(q->normal);
        const F3 nq{nq4.x, nq4.y, nq4.z};
        const F4 Cu = ld4(uw->center);
        const float den = dot3(nq, F3{X.x - Cu.x, X.y - Cu.y, X.z - Cu.z});
        const float num = dot3(nq, F3{X0q.x - Cu.x, X0q.y - Cu.y, X0q.z - Cu.z});
        if (!maps_finite_nonzero(den)) continue;
        const float s = num / den;
        if (!(fabsf(s - 1.0f) <= a.depth_tol)) continue;
        if (a.normal_cos > -1.0f && !(dot3(n, nq) >= a.normal_cos)) continue;
        bits |= 1ull << u;
    }
    agree[i] = bits;
}

// flag[i] (and flag8[i], if given) = 1 for the pixels of `view` that count: valid, and -- with an agree map -- popcount(agree) >=
// min_consistent and, with dedupe, no agreeing view below `view`
__global__ __launch_bounds__(256) void k_maps_flag(int64_t npix, int view, const int32_t* __restrict__ ids, const unsigned long long* __restrict__ agree,
                                                   int min_consistent, int dedupe, int32_t* __restrict__ flag, uint8_t* __restrict__ flag8) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npix) return;
    bool f = ids[i] >= 0;
    if (f && agree) {
        const unsigned long long b = agree[i];
        f = __popcll(b) >= min_consistent && !(dedupe && (b & ((1ull << view) - 1ull)) != 0ull);
    }
    flag[i] = f ? 1 : 0;
    if (flag8) flag8[i] = f ? 1 : 0;
}
__global__ __launch_bounds__(256) void k_maps_expand(int64_t npix, const uint8_t* __restrict__ flag8, int32_t* __restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < npix) flag[i] = flag8[i];
}
// the record of pixel i of `view` at out[base[i]] where flag[i] is set: two 16-byte stores.  ids / pts: the view's own slices.
__global__ __launch_bounds__(256) void k_maps_gather(DParams prm, int view, const int32_t* __restrict__ ids, const float* __restrict__ pts,
                                                     const int32_t* __restrict__ flag, const int32_t* __restrict__ base, uint4* __restrict__ out,
                                                     int64_t cap) {
    const DView* vw = prm.views + view;
    const int64_t npix = (int64_t)vw->W[prm.level] * vw->H[prm.level];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npix || !flag[i]) return;
    const int64_t k = base[i];
    const int32_t id = ids[i];
    if (k < 0 || k >= cap || id < 0) return;
    const DPatch* p = prm.pool + id;
    const uint32_t texel = vw->img[prm.level][i] & 0x00ffffffu;
    uint4 lo, hi;
    lo.x = __float_as_uint(pts[3 * i]); lo.y = __float_as_uint(pts[3 * i + 1]); lo.z = __float_as_uint(pts[3 * i + 2]);
    lo.w = __float_as_uint(p->normal[0]);
    hi.x = __float_as_uint(p->normal[1]); hi.y = __float_as_uint(p->normal[2]);
    hi.z = __float_as_uint(p->ncc);
    hi.w = texel | ((uint32_t)view << 24);
    out[2 * k] = lo;
    out[2 * k + 1] = hi;
}


// sel[0, total_cells) must be zero
void mvsk_maps_select(const DParams& prm, unsigned long long* sel, hipStream_t st) {
    if (prm.pool_n > 0) hipLaunchKernelGGL(k_maps_select, dim3(nblk(prm.pool_n, 256)), dim3(256), 0, st, prm, sel);
}
void mvsk_maps_render(const DParams& prm, int view, int W, int H, int source, const unsigned long long* sel, int32_t* ids, float* pts, hipStream_t st) {
    hipLaunchKernelGGL(k_maps_render, dim3((unsigned)((W + 31) / 32), (unsigned)((H + 7) / 8)), dim3(256), 0, st, prm, view, source, sel, ids, pts);
}
void mvsk_maps_agree(const DParams& prm, const MapsArgs& a, int view, int64_t npix, const int32_t* ids, const float* pts, unsigned long long* agree,
                     float* depth, float* normal, float* conf, hipStream_t st) {
    hipLaunchKernelGGL(k_maps_agree, dim3(nblk(npix, 256)), dim3(256), 0, st, prm, a, view, ids, pts, agree, depth, normal, conf);
}
void mvsk_maps_flag(int64_t npix, int view, const int32_t* ids, const unsigned long long* agree, int min_consistent, int dedupe, int32_t* flag,
                    uint8_t* flag8, hipStream_t st) {
    hipLaunchKernelGGL(k_maps_flag, dim3(nblk(npix, 256)), dim3(256), 0, st, npix, view, ids, agree, min_consistent, dedupe, flag, flag8);
}
void mvsk_maps_expand(int64_t npix, const uint8_t* flag8, int32_t* flag, hipStream_t st) {
    hipLaunchKernelGGL(k_maps_expand, dim3(nblk(npix, 256)), dim3(256), 0, st, npix, flag8, flag);
}
void mvsk_maps_gather(const DParams& prm, int view, int64_t npix, const int32_t* ids, const float* pts, const int32_t* flag, const int32_t* base,
                      void* out, int64_t cap, hipStream_t st) {
    hipLaunchKernelGGL(k_maps_gather, dim3(nblk(npix, 256)), dim3(256), 0, st, prm, view, ids, pts, flag, base, reinterpret_cast<uint4*>(out), cap);
}
