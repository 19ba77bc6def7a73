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
//   k_mattr_colours_visible   the same body with one more gate in front of a view: bit v of the vertex's visibility word
//                     (mvs_engine_mesh_colours_visible; the words come from mvs_mesh_render.hip or from the caller)
// The atomics are vector memory atomics (global_atomic_umax, global_atomic_add_x2).  Arithmetic as everywhere in the engine: fp32, no
// contraction, dot products as left-to-right fmaf chains where the helpers do so; every deciding comparison is written so that a NaN
// fails it.  Stores are plain vector stores.
#include <hip/hip_runtime.h>

#include "mvs_camera.cuh"
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

// ids / usable: all views, view v's slice at a.pix_base[v] (k_mesh_tsdf's); normals may be null; used may be null.  The body of both
// kernels is mvs_mesh_attr_colours.cuh
__global__ __launch_bounds__(MESH_BLOCK) void k_mattr_colours(DParams prm, MapsArgs a, MeshColourArgs m, int64_t n_v, const float* __restrict__ verts,
                                                               const float* __restrict__ normals, const int32_t* __restrict__ ids,
                                                               const uint8_t* __restrict__ usable, uint8_t* __restrict__ rgb, uint8_t* __restrict__ used) {
#define MATTR_GATED 0
#include "mvs_mesh_attr_colours.cuh"
#undef MATTR_GATED
}
// visible: a word a vertex, bit v = view v may take part
__global__ __launch_bounds__(MESH_BLOCK) void k_mattr_colours_visible(DParams prm, MapsArgs a, MeshColourArgs m, int64_t n_v, const float* __restrict__ verts,
                                                                       const float* __restrict__ normals, const int32_t* __restrict__ ids,
                                                                       const uint8_t* __restrict__ usable, const u64* __restrict__ visible,
                                                                       uint8_t* __restrict__ rgb, uint8_t* __restrict__ used) {
#define MATTR_GATED 1
#include "mvs_mesh_attr_colours.cuh"
#undef MATTR_GATED
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
void mvsk_mesh_colours_visible(const DParams& prm, const MapsArgs& a, const MeshColourArgs& m, int64_t n_v, const float* verts, const float* normals,
                               const int32_t* ids, const uint8_t* usable, const unsigned long long* visible, uint8_t* rgb, uint8_t* used, hipStream_t st) {
    if (n_v > 0)
        hipLaunchKernelGGL(k_mattr_colours_visible, dim3(nblk(n_v, MESH_BLOCK)), dim3(MESH_BLOCK), 0, st, prm, a, m, n_v, verts, normals, ids, usable, visible, rgb,
                           used);
}
