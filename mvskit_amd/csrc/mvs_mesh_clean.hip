// mvs_mesh_clean.hip -- what a triangle mesh needs before it is shown: its connected components, the removal of small ones, and Taubin
// smoothing (mvs_engine_mesh_components, mvs_engine_mesh_prune and mvs_engine_mesh_smooth in mvs_engine_mesh.cpp drive it; the
// definitions are in include/mvskit_engine.h).  A lane per triangle or per vertex, 256-thread blocks.
//   k_mclean_check     a lane per triangle: its three ids checked against n_v, one atomic OR per wave that met a bad one
//   k_mclean_init      a lane per vertex: parent[i] = i, size[i] = 0
//   k_mclean_union     a lane per triangle: the lock-free union-find of filterSmallGroups (the smaller id becomes the root, so a root is
//                      the smallest id of its set whatever order the hardware met the triangles in)
//   k_mclean_flatten   a lane per vertex: parent[i] = its root, found WITHOUT path compression -- lane i alone writes parent[i], and what
//                      it replaces pointed at an ancestor of the same root, so every reader ends at that root before and after.  The
//                      boundary components of mvs_mesh_fill.hip are flattened by it too (mvsk_mesh_flatten)
//   k_mclean_count     a lane per triangle: size[root] += 1.  A mesh that is one component would put every add on one word: the lanes that
//                      share the first active lane's root add once, with the popcount of their ballot; the others add for themselves
//   k_mclean_spread    a lane per vertex: size[i] = size[parent[i]] in place (only roots are read, and a root writes what it read), and
//                      the number of roots with a triangle, one add per wave
//   k_mclean_largest   a lane per vertex: a 64-bit atomic max over (ntris << 32) | (0xffffffff - label) of the roots, a wave maximum first
//   k_mclean_keep      a lane per triangle: its keep flag, and a 1 on each of its vertices when it is kept (plain stores of one value)
//   k_mclean_vgather / k_mclean_tgather   the kept rows behind the exclusive scans of the flags; the vertex map
//   k_msmooth_scan     a lane per triangle: the largest |component| of its finite edge differences, through block_max
//   k_msmooth_accum    a lane per triangle: per corner the two terms scaled to 31-bit integers and summed in the lane, three 64-bit integer
//                      atomic adds and one count.  Integer addition is associative: the two terms of a corner may be added before they
//                      reach memory, and the sums do not depend on the order the hardware meets the triangles in
//   k_msmooth_update   a lane per vertex: the mean term in fp64, the step, the cast; the sums cleared for the next step
// The atomics are vector memory atomics; stores are plain vector stores.  fp32 / fp64 without contraction.
#include <hip/hip_runtime.h>

#include "mvs_mesh_common.cuh"
#include "mvs_kernels.h"

using namespace mvsdev;

__global__ __launch_bounds__(MESH_BLOCK) void k_mclean_check(int64_t n_v, int64_t n_t, const int32_t* __restrict__ tris, uint32_t* __restrict__ bad) {
    const int64_t t = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    bool wrong = false;
    if (t < n_t) {
        const int64_t i0 = tris[3 * t], i1 = tris[3 * t + 1], i2 = tris[3 * t + 2];
        wrong = !(i0 >= 0 && i0 < n_v && i1 >= 0 && i1 < n_v && i2 >= 0 && i2 < n_v);
    }
    if (ballot(wrong) != 0ull && lane_id() == 0) atomicOr(bad, 1u);
}

__global__ __launch_bounds__(MESH_BLOCK) void k_mclean_init(int64_t n_v, int* __restrict__ parent, int* __restrict__ size) {
    const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (i < n_v) { parent[i] = (int)i; size[i] = 0; }
}

__global__ __launch_bounds__(MESH_BLOCK) void k_mclean_union(int64_t n_t, const int32_t* __restrict__ tris, int* parent) {
    const int64_t t = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (t >= n_t) return;
    const int i0 = tris[3 * t], i1 = tris[3 * t + 1], i2 = tris[3 * t + 2];
    uf_union(parent, i0, i1);
    uf_union(parent, i0, i2);
}

__global__ __launch_bounds__(MESH_BLOCK) void k_mclean_flatten(int64_t n_v, int* parent) {
    const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (i >= n_v) return;
    int a = (int)i;
    while (true) {
        const int pa = __atomic_load_n(&parent[a], __ATOMIC_RELAXED);
        if (pa == a) break;
        a = pa;
    }
    __atomic_store_n(&parent[i], a, __ATOMIC_RELAXED);
}

__global__ __launch_bounds__(MESH_BLOCK) void k_mclean_count(int64_t n_t, const int32_t* __restrict__ tris, const int* __restrict__ parent, int* __restrict__ size) {
    const int64_t t = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (t >= n_t) return;
    const int r = parent[tris[3 * t]];
    const int r0 = __builtin_amdgcn_readfirstlane(r);
    const unsigned long long same = ballot(r == r0);
    if (r == r0) { if (lane_id() == __ffsll((long long)same) - 1) atomicAdd(&size[r0], (int)__popcll(same)); }
    else atomicAdd(&size[r], 1);
}

__global__ __launch_bounds__(MESH_BLOCK) void k_mclean_spread(int64_t n_v, const int* __restrict__ parent, int* size, unsigned long long* __restrict__ ncomp) {
    const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    bool counts = false;
    if (i < n_v) {
        const int r = parent[i];
        const int s = size[r];
        size[i] = s;
        counts = r == (int)i && s > 0;
    }
    const unsigned long long roots = ballot(counts);
    if (roots != 0ull && lane_id() == __ffsll((long long)roots) - 1) atomicAdd(ncomp, (unsigned long long)__popcll(roots));
}

__global__ __launch_bounds__(MESH_BLOCK) void k_mclean_largest(int64_t n_v, const int* __restrict__ parent, const int* __restrict__ size,
                                                                 unsigned long long* __restrict__ best) {
    const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    unsigned long long key = 0ull;
    if (i < n_v && parent[i] == (int)i && size[i] > 0) key = (unsigned long long)(uint32_t)size[i] << 32 | (unsigned long long)(0xffffffffu - (uint32_t)i);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = shfl_xor64(key, off);
        key = o > key ? o : key;
    }
    if (key != 0ull && lane_id() == 0) atomicMax(best, key);
}

// size: per vertex, after k_mclean_spread.  best: k_mclean_largest's word (read only with largest_only)
__global__ __launch_bounds__(MESH_BLOCK) void k_mclean_keep(int64_t n_t, const int32_t* __restrict__ tris, const int* __restrict__ parent, const int* __restrict__ size,
                                                              int64_t min_triangles, int largest_only, const unsigned long long* __restrict__ best,
                                                              int32_t* __restrict__ tflag, int32_t* __restrict__ vflag) {
    const int64_t t = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (t >= n_t) return;
    const int i0 = tris[3 * t], i1 = tris[3 * t + 1], i2 = tris[3 * t + 2];
    bool keep = (int64_t)size[i0] >= min_triangles;
    if (largest_only) keep = keep && (uint32_t)parent[i0] == 0xffffffffu - (uint32_t)(*best & 0xffffffffull);
    tflag[t] = keep ? 1 : 0;
    if (keep) { vflag[i0] = 1; vflag[i1] = 1; vflag[i2] = 1; }
}

// the kept vertices' position bytes at out[3 vbase[i] ..]; vflag[i] becomes the vertex map: the new id, or -1
__global__ __launch_bounds__(MESH_BLOCK) void k_mclean_vgather(int64_t n_v, const uint32_t* __restrict__ verts, int32_t* __restrict__ vflag,
                                                                 const int32_t* __restrict__ vbase, uint32_t* __restrict__ out, int64_t cap_v) {
    const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (i >= n_v) return;
    const bool keep = vflag[i] != 0;
    const int64_t k = vbase[i];
    if (keep && k < cap_v) { out[3 * k] = verts[3 * i]; out[3 * k + 1] = verts[3 * i + 1]; out[3 * k + 2] = verts[3 * i + 2]; }
    vflag[i] = keep ? (int32_t)k : -1;
}

__global__ __launch_bounds__(MESH_BLOCK) void k_mclean_tgather(int64_t n_t, const int32_t* __restrict__ tris, const int32_t* __restrict__ tflag,
                                                                 const int32_t* __restrict__ tbase, const int32_t* __restrict__ vbase, int32_t* __restrict__ out,
                                                                 int64_t cap_t) {
    const int64_t t = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (t >= n_t || tflag[t] == 0) return;
    const int64_t k = tbase[t];
    if (k >= cap_t) return;
    out[3 * k] = vbase[tris[3 * t]]; out[3 * k + 1] = vbase[tris[3 * t + 1]]; out[3 * k + 2] = vbase[tris[3 * t + 2]];
}

// the three edge differences of a triangle, b - a, c - b, a - c; the terms of a corner are one of them and the negation of another, and
// a - b == -(b - a) exactly in fp32
struct MsmoothEdges { F3 ab, bc, ca; bool fab, fbc, fca; };
DEV MsmoothEdges msmooth_edges(const float* __restrict__ x, int64_t i0, int64_t i1, int64_t i2) {
    const F3 a = ld3(x + 3 * i0), b = ld3(x + 3 * i1), c = ld3(x + 3 * i2);
    MsmoothEdges e;
    e.ab = sub3(b, a); e.bc = sub3(c, b); e.ca = sub3(a, c);
    e.fab = finite3(e.ab); e.fbc = finite3(e.bc); e.fca = finite3(e.ca);
    return e;
}
DEV float msmooth_amax(F3 d) { return fmaxf(fmaxf(fabsf(d.x), fabsf(d.y)), fabsf(d.z)); }

// mbits: max over the contributing terms of the bits of their largest |component| (every id valid: checked before the first step)
__global__ __launch_bounds__(MESH_BLOCK) void k_msmooth_scan(const float* __restrict__ x, int64_t n_t, const int32_t* __restrict__ tris, uint32_t* __restrict__ mbits) {
    __shared__ uint32_t wave_max[MESH_BLOCK / 64];
    const int64_t t = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    uint32_t m = 0;
    if (t < n_t) {
        const MsmoothEdges e = msmooth_edges(x, tris[3 * t], tris[3 * t + 1], tris[3 * t + 2]);
        float f = 0.0f;
        if (e.fab) f = fmaxf(f, msmooth_amax(e.ab));
        if (e.fbc) f = fmaxf(f, msmooth_amax(e.bc));
        if (e.fca) f = fmaxf(f, msmooth_amax(e.ca));
        m = __float_as_uint(f);
    }
    block_max(m, wave_max, mbits);
}

// a term that is not finite adds nothing
DEV Q3 msmooth_q(F3 d, bool finite, double S) {
    if (!finite) return Q3{0, 0, 0};
    return quantise3(d, S);
}
// corner i with the terms +p (when fp) and -m (when fm): acc[3 i + c] += p_c - m_c, cnt[i] += the number of the two that are finite
DEV void msmooth_corner(unsigned long long* __restrict__ acc, int32_t* __restrict__ cnt, int64_t i, Q3 p, bool fp, Q3 m, bool fm) {
    if (!fp && !fm) return;
    atomicAdd(acc + 3 * i, (unsigned long long)(p.x - m.x));
    atomicAdd(acc + 3 * i + 1, (unsigned long long)(p.y - m.y));
    atomicAdd(acc + 3 * i + 2, (unsigned long long)(p.z - m.z));
    atomicAdd(cnt + i, (fp ? 1 : 0) + (fm ? 1 : 0));
}

// llrint(-v) == -llrint(v) under round-half-even, so the term x_a - x_b is the negated integer of x_b - x_a
__global__ __launch_bounds__(MESH_BLOCK) void k_msmooth_accum(const float* __restrict__ x, int64_t n_t, const int32_t* __restrict__ tris,
                                                                const uint32_t* __restrict__ mbits, unsigned long long* __restrict__ acc, int32_t* __restrict__ cnt) {
    const int64_t t = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (t >= n_t) return;
    const uint32_t mb = *mbits;
    if (mb == 0u) return;
    const double S = pow2(30 - exponent(mb));
    const int64_t i0 = tris[3 * t], i1 = tris[3 * t + 1], i2 = tris[3 * t + 2];
    const MsmoothEdges e = msmooth_edges(x, i0, i1, i2);
    const Q3 ab = msmooth_q(e.ab, e.fab, S), bc = msmooth_q(e.bc, e.fbc, S), ca = msmooth_q(e.ca, e.fca, S);
    msmooth_corner(acc, cnt, i0, ab, e.fab, ca, e.fca);  // (b - a) + (c - a)
    msmooth_corner(acc, cnt, i1, bc, e.fbc, ab, e.fab);  // (c - b) + (a - b)
    msmooth_corner(acc, cnt, i2, ca, e.fca, bc, e.fbc);  // (a - c) + (b - c)
}

// x_i' = (float)((double)x_i + (double)f * (((double)A_i * 2^(E - 30)) / (double)c_i)); a vertex without a term, and every vertex of a
// step whose M is 0, keeps its bytes
__global__ __launch_bounds__(MESH_BLOCK) void k_msmooth_update(int64_t n_v, const float* __restrict__ xin, float* __restrict__ xout, float f,
                                                                 const uint32_t* __restrict__ mbits, long long* __restrict__ acc, int32_t* __restrict__ cnt) {
    const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (i >= n_v) return;
    const uint32_t mb = *mbits;
    const int32_t c = cnt[i];
    const uint32_t* bin = reinterpret_cast<const uint32_t*>(xin);
    uint32_t* bout = reinterpret_cast<uint32_t*>(xout);
    if (mb == 0u || c == 0) {
        bout[3 * i] = bin[3 * i]; bout[3 * i + 1] = bin[3 * i + 1]; bout[3 * i + 2] = bin[3 * i + 2];
        return;
    }
    const double back = pow2(exponent(mb) - 30), cd = (double)c, fd = (double)f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double u = ((double)acc[3 * i + k] * back) / cd;
        xout[3 * i + k] = (float)((double)xin[3 * i + k] + fd * u);
        acc[3 * i + k] = 0;
    }
    cnt[i] = 0;
}

void mvsk_mesh_check_ids(int64_t n_v, int64_t n_t, const int32_t* tris, uint32_t* bad, hipStream_t st) { MESH_LAUNCH(k_mclean_check, n_t, n_v, n_t, tris, bad); }
void mvsk_mesh_components(int64_t n_v, int64_t n_t, const int32_t* tris, int32_t* parent, int32_t* size, unsigned long long* ncomp, hipStream_t st) {
    MESH_LAUNCH(k_mclean_init, n_v, n_v, parent, size);
    MESH_LAUNCH(k_mclean_union, n_t, n_t, tris, parent);
    MESH_LAUNCH(k_mclean_flatten, n_v, n_v, parent);
    MESH_LAUNCH(k_mclean_count, n_t, n_t, tris, parent, size);
    MESH_LAUNCH(k_mclean_spread, n_v, n_v, parent, size, ncomp);
}
void mvsk_mesh_flatten(int64_t n_v, int32_t* parent, hipStream_t st) { MESH_LAUNCH(k_mclean_flatten, n_v, n_v, parent); }
void mvsk_mesh_largest(int64_t n_v, const int32_t* parent, const int32_t* size, unsigned long long* best, hipStream_t st) {
    MESH_LAUNCH(k_mclean_largest, n_v, n_v, parent, size, best);
}
void mvsk_mesh_keep(int64_t n_t, const int32_t* tris, const int32_t* parent, const int32_t* size, int64_t min_triangles, int largest_only,
                    const unsigned long long* best, int32_t* tflag, int32_t* vflag, hipStream_t st) {
    MESH_LAUNCH(k_mclean_keep, n_t, n_t, tris, parent, size, min_triangles, largest_only, best, tflag, vflag);
}
void mvsk_mesh_gather(int64_t n_v, const float* verts, int32_t* vflag, const int32_t* vbase, float* out_verts, int64_t cap_v, int64_t n_t, const int32_t* tris,
                      const int32_t* tflag, const int32_t* tbase, int32_t* out_tris, int64_t cap_t, hipStream_t st) {
    MESH_LAUNCH(k_mclean_tgather, n_t, n_t, tris, tflag, tbase, vbase, out_tris, cap_t);
    MESH_LAUNCH(k_mclean_vgather, n_v, n_v, reinterpret_cast<const uint32_t*>(verts), vflag, vbase, reinterpret_cast<uint32_t*>(out_verts), cap_v);
}
void mvsk_mesh_smooth_step(int64_t n_v, const float* xin, float* xout, float f, int64_t n_t, const int32_t* tris, uint32_t* mbits, long long* acc, int32_t* cnt,
                           hipStream_t st) {
    MESH_LAUNCH(k_msmooth_scan, n_t, xin, n_t, tris, mbits);
    MESH_LAUNCH(k_msmooth_accum, n_t, xin, n_t, tris, mbits, reinterpret_cast<unsigned long long*>(acc), cnt);
    MESH_LAUNCH(k_msmooth_update, n_v, n_v, xin, xout, f, mbits, acc, cnt);
}
