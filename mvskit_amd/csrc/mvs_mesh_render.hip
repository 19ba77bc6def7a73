// mvs_mesh_render.hip -- a triangle mesh seen from the views: an order-free z-buffer of depth and triangle row per view, and the per-vertex
// visibility derived from it (mvs_engine_mesh_render and mvs_engine_mesh_visibility in mvs_engine_mesh.cpp drive it; the contract is in
// include/mvskit_engine.h).  One view at a time, through one set of per-view buffers.
//   k_mrender_project   a lane per vertex: project()'s three fma chains on P at the level, the position snapped to 1/256 pixel, the depth
//                       along the optical axis and the usable flag
//   k_mrender_small     a lane per triangle: the integer edges and the three reciprocal depths once (mrender_setup), then the pixel
//                       centres of its clipped box where that holds at most `small_max` of them; the others go to a list (one atomic a
//                       wave, the list's order cannot matter); the skipped ones are counted (one add a wave)
//   k_mrender_large     a wave per listed triangle: the clipped box in tiles of 8 x 8 pixels, a lane a pixel; a tile whose corners lie
//                       outside one edge is rejected before any pixel is tested.  A triangle across the whole image costs its wave
//                       W H / 64 steps
//   k_mrender_resolve   a lane per pixel: the key into depth and triangle row, NaN and -1 where no triangle wrote; the covered pixels
//                       counted (one add a wave)
//   k_mrender_visible   a lane per vertex: the vertex's depth against the z-buffer at its nearest pixel; bit v of its own word, no atomic
// The z-buffer holds one 64-bit key a pixel, (bits(depth) << 32) | row, all ones before a view; the rasterising kernels write it with a
// non-returning global_atomic_umin_x2 and look at the key first with a relaxed agent-scope atomic load (never a plain load of what another
// workgroup writes in the same launch), skipping the atomic that cannot win.  The minimum is associative: the maps do not depend on the
// order the hardware meets the triangles in.  Coverage is integer arithmetic (every edge function below 2^51), the depth an fp64 chain
// without contraction.  Every loop is bounded by the clipped box: no kernel waits for another's progress.  Stores are plain vector stores.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "mvs_mesh_common.cuh"
#include "mvs_kernels.h"

using namespace mvsdev;

#define MRENDER_LIMIT ((long long)1 << 24)  // |sx|, |sy| of a usable vertex, in 1/256 pixel

DEV u64 mrender_peek(const u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// scr[2 i ..] = (sx, sy) saturated to int32, vd[i] = d, ok[i] = usable
__global__ __launch_bounds__(MESH_BLOCK) void k_mrender_project(const DView* __restrict__ views, int view, int level, int64_t n_v, const float* __restrict__ verts,
                                                                 int32_t* __restrict__ scr, float* __restrict__ vd, uint32_t* __restrict__ ok) {
    const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (i >= n_v) return;
    const float* P = views[view].P[level];
    const F3 X = ld3(verts + 3 * i);
    const float r0 = fma_(P[3], 1.0f, fma_(P[2], X.z, fma_(P[1], X.y, P[0] * X.x)));
    const float r1 = fma_(P[7], 1.0f, fma_(P[6], X.z, fma_(P[5], X.y, P[4] * X.x)));
    const float r2 = fma_(P[11], 1.0f, fma_(P[10], X.z, fma_(P[9], X.y, P[8] * X.x)));
    const float lo = (float)(INT_MIN + 3.0f), hi = (float)(INT_MAX - 3.0f);
    const float inv = rcp_rn(r2);
    const float x = fmaxf(lo, fminf(hi, r0 * inv)), y = fmaxf(lo, fminf(hi, r1 * inv));  // a NaN becomes hi
    const long long sx = __double2ll_rn((double)x * 256.0), sy = __double2ll_rn((double)y * 256.0);
    const bool usable = r2 > 0.0f && r2 < __int_as_float(0x7f800000) && sx >= -MRENDER_LIMIT && sx <= MRENDER_LIMIT && sy >= -MRENDER_LIMIT && sy <= MRENDER_LIMIT;
    scr[2 * i] = (int32_t)max((long long)INT_MIN, min((long long)INT_MAX, sx));
    scr[2 * i + 1] = (int32_t)max((long long)INT_MIN, min((long long)INT_MAX, sy));
    vd[i] = r2;
    ok[i] = usable ? 1u : 0u;
}

// One triangle ready for its pixels.  Edge k lies opposite vertex k (after the swap that makes the area positive): E_k at the pixel
// (px, py) = a[k] px + b[k] py + c[k], covered when E_k + tl[k] > 0 for every k (tl = 1 on a top-left edge: E == 0 counts there).
struct MrTri {
    long long a[3], b[3], c[3], area;
    int tl[3];
    double w[3];
    int x0, y0, x1, y1;  // the pixels of the bounding box clipped to the image; empty when x1 < x0 or y1 < y0
};
enum { MR_SKIPPED = 0, MR_EMPTY = 1, MR_READY = 2 };

DEV int mrender_setup(int64_t t, const int32_t* __restrict__ tris, const int32_t* __restrict__ scr, const float* __restrict__ vd, const uint32_t* __restrict__ ok,
                      int W, int H, MrTri& s) {
    const int64_t i0 = tris[3 * t];
    int64_t i1 = tris[3 * t + 1], i2 = tris[3 * t + 2];
    if (!(ok[i0] && ok[i1] && ok[i2])) return MR_SKIPPED;
    const long long X0 = scr[2 * i0], Y0 = scr[2 * i0 + 1];
    long long X1 = scr[2 * i1], Y1 = scr[2 * i1 + 1], X2 = scr[2 * i2], Y2 = scr[2 * i2 + 1];
    long long area = (X1 - X0) * (Y2 - Y0) - (Y1 - Y0) * (X2 - X0);
    if (area == 0) return MR_EMPTY;
    if (area < 0) {
        const long long tx = X1, ty = Y1; X1 = X2; Y1 = Y2; X2 = tx; Y2 = ty;
        const int64_t ti = i1; i1 = i2; i2 = ti;
        area = -area;
    }
    s.area = area;
    s.w[0] = 1.0 / (double)vd[i0]; s.w[1] = 1.0 / (double)vd[i1]; s.w[2] = 1.0 / (double)vd[i2];
    // the directed edges 1 -> 2, 2 -> 0, 0 -> 1: E = dx (qy - ay) - dy (qx - ax) at q = 256 (px, py)
    const long long ax[3] = {X1, X2, X0}, ay[3] = {Y1, Y2, Y0}, bx[3] = {X2, X0, X1}, by[3] = {Y2, Y0, Y1};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const long long dx = bx[k] - ax[k], dy = by[k] - ay[k];
        s.a[k] = -dy * 256; s.b[k] = dx * 256; s.c[k] = dy * ax[k] - dx * ay[k];
        s.tl[k] = (dy < 0 || (dy == 0 && dx > 0)) ? 1 : 0;
    }
    const long long xmin = min(X0, min(X1, X2)), xmax = max(X0, max(X1, X2)), ymin = min(Y0, min(Y1, Y2)), ymax = max(Y0, max(Y1, Y2));
    // the pixels whose centre 256 p lies in [min, max]: ceil(min / 256) .. floor(max / 256) (an arithmetic shift floors)
    s.x0 = (int)max((long long)0, (xmin + 255) >> 8); s.x1 = (int)min((long long)(W - 1), xmax >> 8);
    s.y0 = (int)max((long long)0, (ymin + 255) >> 8); s.y1 = (int)min((long long)(H - 1), ymax >> 8);
    return MR_READY;
}

// the pixel (px, py) of triangle t: the cover test, the depth, the key
DEV void mrender_pixel(const MrTri& s, int64_t t, int px, int py, int W, u64* __restrict__ keys) {
    const long long E0 = s.a[0] * px + s.b[0] * py + s.c[0], E1 = s.a[1] * px + s.b[1] * py + s.c[1], E2 = s.a[2] * px + s.b[2] * py + s.c[2];
    if (!(E0 + s.tl[0] > 0 && E1 + s.tl[1] > 0 && E2 + s.tl[2] > 0)) return;
    const double inv = ((double)E0 * s.w[0] + (double)E1 * s.w[1] + (double)E2 * s.w[2]) / (double)s.area;
    const float depth = (float)(1.0 / inv);
    if (!(fabsf(depth) < __int_as_float(0x7f800000))) return;
    const u64 key = (u64)__float_as_uint(depth) << 32 | (u64)(uint32_t)t;
    u64* slot = keys + ((int64_t)py * W + px);
    if (key < mrender_peek(slot)) (void)atomicMin(slot, key);
}

// counts: [0] the listed triangles, [1] the skipped ones (both zero before the launch); list holds up to n_t rows
__global__ __launch_bounds__(MESH_BLOCK) void k_mrender_small(int64_t n_t, const int32_t* __restrict__ tris, const int32_t* __restrict__ scr,
                                                               const float* __restrict__ vd, const uint32_t* __restrict__ ok, int W, int H, int small_max,
                                                               u64* __restrict__ keys, int32_t* __restrict__ list, u64* __restrict__ counts) {
    const int64_t t = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    const int lane = lane_id();
    MrTri s;
    int state = MR_EMPTY;
    if (t < n_t) state = mrender_setup(t, tris, scr, vd, ok, W, H, s);
    const bool boxed = state == MR_READY && s.x1 >= s.x0 && s.y1 >= s.y0;
    const bool big = boxed && (int64_t)(s.x1 - s.x0 + 1) * (s.y1 - s.y0 + 1) > small_max;
    const u64 skipped = ballot(state == MR_SKIPPED), listed = ballot(big);
    if (skipped != 0ull && lane == 0) atomicAdd(counts + 1, (u64)__popcll(skipped));
    if (listed != 0ull) {
        u64 base = 0;
        if (lane == 0) base = atomicAdd(counts, (u64)__popcll(listed));
        base = (u64)(uint32_t)__shfl((int)(uint32_t)base, 0);  // at most 2^30 rows
        if (big) list[base + __popcll(listed & ((1ull << lane) - 1ull))] = (int32_t)t;
    }
    if (!boxed || big) return;
    for (int py = s.y0; py <= s.y1; ++py)
        for (int px = s.x0; px <= s.x1; ++px) mrender_pixel(s, t, px, py, W, keys);
}

// nlist: the number of rows in list, written by the launch before
__global__ __launch_bounds__(MESH_BLOCK) void k_mrender_large(const int32_t* __restrict__ tris, const int32_t* __restrict__ scr, const float* __restrict__ vd,
                                                               const uint32_t* __restrict__ ok, int W, int H, u64* __restrict__ keys,
                                                               const int32_t* __restrict__ list, const u64* __restrict__ nlist) {
    const int64_t n = (int64_t)*nlist, nwaves = (int64_t)gridDim.x * (MESH_BLOCK / 64);
    const int lane = lane_id(), lx = lane & 7, ly = lane >> 3;
    for (int64_t i = (int64_t)blockIdx.x * (MESH_BLOCK / 64) + (threadIdx.x >> 6); i < n; i += nwaves) {
        const int64_t t = list[i];
        MrTri s;
        if (mrender_setup(t, tris, scr, vd, ok, W, H, s) != MR_READY) continue;  // a listed triangle is ready
        for (int oy = s.y0; oy <= s.y1; oy += 8)
            for (int ox = s.x0; ox <= s.x1; ox += 8) {
                // E_k is affine: its largest value over the tile lies in a corner.  Below zero on one edge, no pixel of the tile is covered
                bool out = false;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const long long top = s.a[k] * ox + s.b[k] * oy + s.c[k] + max(0ll, 7 * s.a[k]) + max(0ll, 7 * s.b[k]);
                    out = out || top < 0;
                }
                if (out) continue;
                const int px = ox + lx, py = oy + ly;
                if (px <= s.x1 && py <= s.y1) mrender_pixel(s, t, px, py, W, keys);
            }
    }
}

// *covered += the pixels with a key (zero before the launch); depth or tri may be null
__global__ __launch_bounds__(MESH_BLOCK) void k_mrender_resolve(int64_t npix, const u64* __restrict__ keys, float* __restrict__ depth, int32_t* __restrict__ tri,
                                                                 u64* __restrict__ covered) {
    const int64_t p = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    bool have = false;
    if (p < npix) {
        const u64 key = keys[p];
        have = key != MESH_EMPTY;
        if (depth) depth[p] = have ? __uint_as_float((uint32_t)(key >> 32)) : __int_as_float(0x7fc00000);
        if (tri) tri[p] = have ? (int32_t)(uint32_t)key : -1;
    }
    const u64 m = ballot(have);
    if (m != 0ull && lane_id() == 0) atomicAdd(covered, (u64)__popcll(m));
}

// visible[i] |= 1 << view where vertex i is usable, its nearest pixel lies inside the image and holds no nearer surface
__global__ __launch_bounds__(MESH_BLOCK) void k_mrender_visible(int view, float tol, int64_t n_v, const int32_t* __restrict__ scr, const float* __restrict__ vd,
                                                                 const uint32_t* __restrict__ ok, int W, int H, const u64* __restrict__ keys,
                                                                 u64* __restrict__ visible) {
    const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (i >= n_v || !ok[i]) return;
    const int px = (scr[2 * i] + 128) >> 8, py = (scr[2 * i + 1] + 128) >> 8;
    if (px < 0 || px >= W || py < 0 || py >= H) return;
    const u64 key = keys[(int64_t)py * W + px];
    bool seen = key == MESH_EMPTY;
    if (!seen) {
        const float z = __uint_as_float((uint32_t)(key >> 32));
        seen = (double)vd[i] <= (double)z * (1.0 + (double)tol);
    }
    if (seen) visible[i] |= 1ull << view;
}


void mvsk_mrender_project(const DParams& prm, int view, int64_t n_v, const float* verts, int32_t* scr, float* vd, uint32_t* ok, hipStream_t st) {
    MESH_LAUNCH(k_mrender_project, n_v, prm.views, view, prm.level, n_v, verts, scr, vd, ok);
}
void mvsk_mrender_raster(int64_t n_t, const int32_t* tris, const int32_t* scr, const float* vd, const uint32_t* ok, int W, int H, int small_max,
                         unsigned long long* keys, int32_t* list, unsigned long long* counts, hipStream_t st) {
    if (n_t <= 0) return;
    MESH_LAUNCH(k_mrender_small, n_t, n_t, tris, scr, vd, ok, W, H, small_max, keys, list, counts);
    // the list's length stays on the device: a fixed grid walks it, a wave a triangle
    const unsigned blocks = (unsigned)std::min<int64_t>(nblk(n_t, MESH_BLOCK / 64), 2048);
    hipLaunchKernelGGL(k_mrender_large, dim3(blocks), dim3(MESH_BLOCK), 0, st, tris, scr, vd, ok, W, H, keys, list, counts);
}
void mvsk_mrender_resolve(int64_t npix, const unsigned long long* keys, float* depth, int32_t* tri, unsigned long long* covered, hipStream_t st) {
    MESH_LAUNCH(k_mrender_resolve, npix, npix, keys, depth, tri, covered);
}
void mvsk_mrender_visible(int view, float tol, int64_t n_v, const int32_t* scr, const float* vd, const uint32_t* ok, int W, int H, const unsigned long long* keys,
                          unsigned long long* visible, hipStream_t st) {
    MESH_LAUNCH(k_mrender_visible, n_v, view, tol, n_v, scr, vd, ok, W, H, keys, visible);
}
