// mvs_mesh_attr.hip -- what a triangle mesh needs to be looked at: vertex normals and view-blended vertex colours (mvs_engine_mesh_normals
// and mvs_engine_mesh_colours in mvs_engine_mesh.cpp drive it; the definitions are in include/mvskit_engine.h).
//   k_mattr_scan      a lane per triangle: its three indices checked against n_v, and the largest |component| of the face vectors --
//                     block_max's two halves (mvs_mesh_common.cuh), the wave's report of a bad index between them
//   k_mattr_accum     a lane per triangle: the face vector scaled to 31-bit integers (quantise3), nine 64-bit integer atomic adds into the sums of
//                     its three corners.  Integer addition is associative: the sums do not depend on the order the hardware meets
//                     the triangles in, whatever the valence of a vertex
//   k_mattr_finish    a lane per vertex: the sum normalised in fp64, cast to fp32
//   k_mattr_colours   a lane per vertex, the views in ascending order, wave-uniform (the camera comes through uniform loads): window,
//                     mask, facing weight, the surface test against the dense maps at the nearest pixel, the bilinear sample;
//                     the weighted mean of the confirmed views, else of the unconfirmed ones.  Vertices of mvs_engine_extract_mesh
//                     come in lattice order, so neighbouring lanes meet neighbouring pixels.  Four lanes share three 32-bit stores
//                     for their twelve colour bytes where the output is 4-byte aligned.
// The atomics are vector memory atomics (global_atomic_umax, global_atomic_add_x2).  Arithmetic as everywhere in the engine: fp32, no
// contraction, dot products as left-to-right fmaf chains where the helpers do so; every deciding comparison is written so that a NaN
// fails it.  Stores are plain vector stores.
#include <hip/hip_runtime.h>

#include "mvs_mesh_common.cuh"
#include "mvs_kernels.h"

using namespace mvsdev;

DEV bool mattr_finite_nonzero(float a) { return fabsf(a) > 0.0f && fabsf(a) < __int_as_float(0x7f800000); }

// f = (v1 - v0) x (v2 - v0), every component two products and one subtraction; false when a component is not finite
DEV bool mattr_face(const float* __restrict__ verts, int64_t i0, int64_t i1, int64_t i2, F3& f) {
    const F3 a = ld3(verts + 3 * i0), b = ld3(verts + 3 * i1), c = ld3(verts + 3 * i2);
    f = cross3(sub3(b, a), sub3(c, a));
    return finite3(f);
}

// mbits: max over the contributing triangles of the bits of max |f_c| (non-negative floats order as their bits do); bad: != 0 when an
// index lies outside 0 .. n_v - 1.  A triangle with such an index reads no vertex.
__global__ __launch_bounds__(MESH_BLOCK) void k_mattr_scan(int64_t n_v, const float* __restrict__ verts, int64_t n_t, const int32_t* __restrict__ tris,
                                                            uint32_t* __restrict__ mbits, uint32_t* __restrict__ bad) {
    __shared__ uint32_t wave_max[MESH_BLOCK / 64];
    const int64_t t = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    uint32_t m = 0;
    bool wrong = false;
    if (t < n_t) {
        const int64_t i0 = tris[3 * t], i1 = tris[3 * t + 1], i2 = tris[3 * t + 2];
        wrong = !(i0 >= 0 && i0 < n_v && i1 >= 0 && i1 < n_v && i2 >= 0 && i2 < n_v);
        F3 f;
        if (!wrong && mattr_face(verts, i0, i1, i2, f)) m = __float_as_uint(fmaxf(fmaxf(fabsf(f.x), fabsf(f.y)), fabsf(f.z)));
    }
    const int lane = lane_id();
    m = block_max_waves(m, wave_max);
    if (ballot(wrong) != 0ull && lane == 0) atomicOr(bad, 1u);
    block_max_atomic(m, wave_max, mbits);
}

// acc[3 i + c] += llrint((double)f_c * S) for the three corners i of every contributing triangle; the product is exact and below 2^31
__global__ __launch_bounds__(MESH_BLOCK) void k_mattr_accum(const float* __restrict__ verts, int64_t n_t, const int32_t* __restrict__ tris,
                                                             const uint32_t* __restrict__ mbits, unsigned long long* __restrict__ acc) {
    const int64_t t = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (t >= n_t) return;
    const uint32_t mb = *mbits;
    if (mb == 0u) return;
    const double S = pow2(30 - exponent(mb));
    const int64_t i[3] = {tris[3 * t], tris[3 * t + 1], tris[3 * t + 2]};
    F3 f;
    if (!mattr_face(verts, i[0], i[1], i[2], f)) return;
    const Q3 q = quantise3(f, S);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        atomicAdd(acc + 3 * i[k], (u64)q.x);
        atomicAdd(acc + 3 * i[k] + 1, (u64)q.y);
        atomicAdd(acc + 3 * i[k] + 2, (u64)q.z);
    }
}

// n = (float)(a / sqrt(ax ax + ay ay + az az)) in fp64, left to right; a zero length gives (0, 0, 0)
__global__ __launch_bounds__(MESH_BLOCK) void k_mattr_finish(int64_t n_v, const long long* __restrict__ acc, float* __restrict__ normals) {
    const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (i >= n_v) return;
    const double ax = (double)acc[3 * i], ay = (double)acc[3 * i + 1], az = (double)acc[3 * i + 2];
    const double len = sqrt(ax * ax + ay * ay + az * az);
    const bool have = len > 0.0;
    normals[3 * i] = have ? (float)(ax / len) : 0.0f;
    normals[3 * i + 1] = have ? (float)(ay / len) : 0.0f;
    normals[3 * i + 2] = have ? (float)(az / len) : 0.0f;
}

// min(255, (int)floorf(sc / sw + 0.5f)); nothing below 0, and 0 for a NaN (a weight sum that is not positive: min_cos <= 0)
DEV uint32_t mattr_channel(float sc, float sw) {
    const float t = floorf(sc / sw + 0.5f);
    return t >= 255.0f ? 255u : (t >= 0.0f ? (uint32_t)(int)t : 0u);
}

// ids / usable: all views, view v's slice at a.pix_base[v] (k_mesh_tsdf's); normals may be null; used may be null
__global__ __launch_bounds__(MESH_BLOCK) void k_mattr_colours(DParams prm, MapsArgs a, MeshColourArgs m, int64_t n_v, const float* __restrict__ verts,
                                                               const float* __restrict__ normals, const int32_t* __restrict__ ids,
                                                               const uint8_t* __restrict__ usable, uint8_t* __restrict__ rgb, uint8_t* __restrict__ used) {
    const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    const bool live = i < n_v;  // a lane beyond the end stays for the shuffles of the packed store
    uint32_t colour = 128u | 128u << 8 | 128u << 16, use = 0u;
    if (live) {
        const F3 X = ld3(verts + 3 * i);
        const F4 X1{X.x, X.y, X.z, 1.0f};
        const F3 n = normals ? ld3(normals + 3 * i) : F3{0.0f, 0.0f, 0.0f};
        const bool facing = !(n.x == 0.0f && n.y == 0.0f && n.z == 0.0f);  // a NaN normal is tested, and fails
        // tier 0: the CONFIRMED views, tier 1: the UNCONFIRMED ones
        float sw[2] = {0.0f, 0.0f}, sr[2] = {0.0f, 0.0f}, sg[2] = {0.0f, 0.0f}, sb[2] = {0.0f, 0.0f};
        int cnt[2] = {0, 0};
        for (int v = 0; v < prm.nviews; ++v) {
            const DView* vw = prm.views + v;
            const int W = vw->W[prm.level], H = vw->H[prm.level];
            const F3 ic = project(vw, X1, prm.level);
            if (!(ic.z > 0.0f && ic.x >= 0.0f && ic.y >= 0.0f && ic.x < (float)(W - 1) && ic.y < (float)(H - 1))) continue;
            const int64_t near = (int64_t)(int)floorf(ic.y + 0.5f) * W + (int)floorf(ic.x + 0.5f);  // inside the image: the window is
            if (vw->mask && vw->mask[near] == 0) continue;
            const F4 C = ld4(vw->center);
            float w = 1.0f;
            if (facing) {
                const F3 d{C.x - X.x, C.y - X.y, C.z - X.z};
                w = dot3(n, d) / sqrtf(dot3(d, d));
                if (!(w >= m.min_cos)) continue;
            }
            int tier = 1;
            const int64_t pix = a.pix_base[v] + near;
            const int32_t idq = usable[pix] ? ids[pix] : -1;
            if (idq >= 0 && (int64_t)idq < prm.pool_n) {
                const DPatch* q = prm.pool + idq;
                const F4 X0q = ld4(q->coord), nq4 = ld4(q->normal);
                const F3 nq{nq4.x, nq4.y, nq4.z};
                const float den = dot3(nq, F3{X.x - C.x, X.y - C.y, X.z - C.z});
                const float num = dot3(nq, F3{X0q.x - C.x, X0q.y - C.y, X0q.z - C.z});
                if (!mattr_finite_nonzero(den)) continue;
                const float s = num / den;
                if (!(fabsf(s - 1.0f) <= m.occl_tol)) continue;  // occluded behind that view's surface, or floating in front of it
                tier = 0;
            }
            // ply_colour's bilinear sample of the RGBA8 pyramid, its expressions in its order
            const float x = ic.x, y = ic.y;
            const int lx = (int)x, ly = (int)y;
            const float dx1 = x - lx, dx0 = 1.0f - dx1, dy1 = y - ly, dy0 = 1.0f - dy1;
            const float f00 = dx0 * dy0, f01 = dx0 * dy1, f10 = dx1 * dy0, f11 = dx1 * dy1;
            const uint32_t* r0 = vw->img[prm.level] + ((size_t)ly * W + lx);
            const uint32_t* r1 = r0 + W;
            const uint32_t ta = r0[0], tb = r0[1], tc = r1[0], td = r1[1];
#define MATTR_CH(t, s) ((int)(((t) >> (s)) & 0xffu))
            const float cr = (MATTR_CH(ta, 0) * f00 + MATTR_CH(tc, 0) * f01) + (MATTR_CH(tb, 0) * f10 + MATTR_CH(td, 0) * f11);
            const float cg = (MATTR_CH(ta, 8) * f00 + MATTR_CH(tc, 8) * f01) + (MATTR_CH(tb, 8) * f10 + MATTR_CH(td, 8) * f11);
            const float cb = (MATTR_CH(ta, 16) * f00 + MATTR_CH(tc, 16) * f01) + (MATTR_CH(tb, 16) * f10 + MATTR_CH(td, 16) * f11);
#undef MATTR_CH
            // the tier is a select, not an index: the sums stay in registers
            const bool t0 = tier == 0;
            sw[0] = t0 ? sw[0] + w : sw[0]; sr[0] = t0 ? sr[0] + w * cr : sr[0]; sg[0] = t0 ? sg[0] + w * cg : sg[0]; sb[0] = t0 ? sb[0] + w * cb : sb[0];
            sw[1] = t0 ? sw[1] : sw[1] + w; sr[1] = t0 ? sr[1] : sr[1] + w * cr; sg[1] = t0 ? sg[1] : sg[1] + w * cg; sb[1] = t0 ? sb[1] : sb[1] + w * cb;
            cnt[0] += t0 ? 1 : 0; cnt[1] += t0 ? 0 : 1;
        }
        if (cnt[0] > 0) {
            colour = mattr_channel(sr[0], sw[0]) | mattr_channel(sg[0], sw[0]) << 8 | mattr_channel(sb[0], sw[0]) << 16;
            use = (uint32_t)cnt[0] | 0x80u;
        } else if (cnt[1] > 0) {
            colour = mattr_channel(sr[1], sw[1]) | mattr_channel(sg[1], sw[1]) << 8 | mattr_channel(sb[1], sw[1]) << 16;
            use = (uint32_t)cnt[1];
        }
    }
    if (live && used) used[i] = (uint8_t)use;
    // the twelve bytes of lanes 4 g .. 4 g + 3 as three words, written by the first three of them: the block starts at a multiple of four
    // vertices, so a 4-byte aligned rgb has every quad on a word boundary
    const int lane = lane_id(), quad = lane & ~3, j = lane & 3;
    const uint32_t c0 = (uint32_t)__shfl((int)colour, quad), c1 = (uint32_t)__shfl((int)colour, quad + 1), c2 = (uint32_t)__shfl((int)colour, quad + 2),
                   c3 = (uint32_t)__shfl((int)colour, quad + 3);
    const bool packed = (reinterpret_cast<uintptr_t>(rgb) & 3u) == 0u && (i - j) + 3 < n_v;
    if (packed) {
        const uint32_t word = j == 0 ? (c0 | c1 << 24) : (j == 1 ? (c1 >> 8 | c2 << 16) : (c2 >> 16 | c3 << 8));
        if (j < 3) reinterpret_cast<uint32_t*>(rgb + 3 * (i - j))[j] = word;
    } else if (live) {
        rgb[3 * i] = (uint8_t)(colour & 0xffu);
        rgb[3 * i + 1] = (uint8_t)((colour >> 8) & 0xffu);
        rgb[3 * i + 2] = (uint8_t)((colour >> 16) & 0xffu);
    }
}


void mvsk_mesh_normals_scan(int64_t n_v, const float* verts, int64_t n_t, const int32_t* tris, uint32_t* mbits, uint32_t* bad, hipStream_t st) {
    if (n_t > 0) hipLaunchKernelGGL(k_mattr_scan, dim3(nblk(n_t, MESH_BLOCK)), dim3(MESH_BLOCK), 0, st, n_v, verts, n_t, tris, mbits, bad);
}
void mvsk_mesh_normals_accum(const float* verts, int64_t n_t, const int32_t* tris, const uint32_t* mbits, long long* acc, hipStream_t st) {
    if (n_t > 0)
        hipLaunchKernelGGL(k_mattr_accum, dim3(nblk(n_t, MESH_BLOCK)), dim3(MESH_BLOCK), 0, st, verts, n_t, tris, mbits, reinterpret_cast<unsigned long long*>(acc));
}
void mvsk_mesh_normals_finish(int64_t n_v, const long long* acc, float* normals, hipStream_t st) {
    if (n_v > 0) hipLaunchKernelGGL(k_mattr_finish, dim3(nblk(n_v, MESH_BLOCK)), dim3(MESH_BLOCK), 0, st, n_v, acc, normals);
}
void mvsk_mesh_colours(const DParams& prm, const MapsArgs& a, const MeshColourArgs& m, int64_t n_v, const float* verts, const float* normals,
                       const int32_t* ids, const uint8_t* usable, uint8_t* rgb, uint8_t* used, hipStream_t st) {
    if (n_v > 0) hipLaunchKernelGGL(k_mattr_colours, dim3(nblk(n_v, MESH_BLOCK)), dim3(MESH_BLOCK), 0, st, prm, a, m, n_v, verts, normals, ids, usable, rgb, used);
}
