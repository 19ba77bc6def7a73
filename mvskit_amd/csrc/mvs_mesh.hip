// mvs_mesh.hip -- a triangle mesh from the dense maps: a truncated signed distance volume over the rendered planes, then marching
// tetrahedra (mvs_engine_tsdf, mvs_engine_extract_mesh and mvs_engine_mesh in mvs_engine.cpp drive it; the definitions are in
// include/mvskit_engine.h).  A lane per lattice point everywhere, p = (k ny + j) nx + i with i fastest.
//   k_mesh_tsdf     the views in ascending order, wave-uniform: the point's pixel in the view, that pixel's plane cut by the view's ray
//                   through the point -> the truncated signed distance, averaged over the views that see the point
//   k_mesh_state    a byte per point: bit 0 OBSERVED, bit 1 INSIDE
//   k_mesh_edges    a byte per point: bit d - 1 = the edge from p in direction d carries a vertex; and the number of set bits
//   k_mesh_verts    the vertices behind the exclusive scan of those numbers: ascending (p, slot)
//   k_mesh_tcount   the triangles of the cube whose corner 0 is p (0 to 12)
//   k_mesh_tris     the triangles behind the exclusive scan of those numbers
// No atomics: every position comes from a scan.  Arithmetic as everywhere in the engine: fp32, no contraction, dot products as
// left-to-right fmaf chains; every deciding comparison is written so that a NaN fails it.  Stores are plain vector stores.
#include <hip/hip_runtime.h>

#include "mvs_camera.cuh"
#include "mvs_common.cuh"
#include "mvs_kernels.h"

using namespace mvsdev;

DEV bool mesh_finite_nonzero(float a) { return fabsf(a) > 0.0f && fabsf(a) < __int_as_float(0x7f800000); }

struct MeshIdx { int i, j, k; };
DEV MeshIdx mesh_idx(const MeshVol& vol, int64_t p) {
    const int64_t row = p / vol.nx;
    return {(int)(p - row * vol.nx), (int)(row % vol.ny), (int)(row / vol.ny)};
}
// origin + (float)idx * voxel: one multiplication, one addition
DEV F3 mesh_pos(const MeshVol& vol, int i, int j, int k) {
    return {vol.origin[0] + (float)i * vol.voxel, vol.origin[1] + (float)j * vol.voxel, vol.origin[2] + (float)k * vol.voxel};
}
// the lattice point one step from p along direction / cube corner c = dx + 2 dy + 4 dz
DEV int64_t mesh_step(const MeshVol& vol, int64_t p, int c) {
    return p + (c & 1) + (int64_t)((c >> 1) & 1) * vol.nx + (int64_t)((c >> 2) & 1) * vol.nx * vol.ny;
}

// ids / usable: all views, view v's slice at a.pix_base[v]; usable = the flag byte of k_maps_flag without dedupe
__global__ __launch_bounds__(256) void k_mesh_tsdf(DParams prm, MapsArgs a, MeshVol vol, int64_t npoints, const int32_t* __restrict__ ids,
                                                   const uint8_t* __restrict__ usable, float* __restrict__ tsdf, int32_t* __restrict__ count) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= npoints) return;
    const MeshIdx ix = mesh_idx(vol, p);
    const F3 X = mesh_pos(vol, ix.i, ix.j, ix.k);
    const F4 X1{X.x, X.y, X.z, 1.0f};
    float sum = 0.0f;
    int n = 0;
    for (int v = 0; v < prm.nviews; ++v) {
        const DView* vw = prm.views + v;
        const int W = vw->W[prm.level], H = vw->H[prm.level];
        const F3 ic = project(vw, X1, prm.level);
        const float fx = floorf(ic.x + 0.5f), fy = floorf(ic.y + 0.5f);
        if (!(ic.z > 0.0f && fx >= 0.0f && fx < (float)W && fy >= 0.0f && fy < (float)H)) continue;
        const int64_t pix = a.pix_base[v] + (int64_t)(int)fy * W + (int)fx;
        if (!usable[pix]) continue;
        const int32_t idq = ids[pix];
        if (idq < 0 || (int64_t)idq >= prm.pool_n) continue;
        const DPatch* q = prm.pool + idq;
        const F4 X0q = ld4(q->coord), nq4 = ld4(q->normal);
        const F3 nq{nq4.x, nq4.y, nq4.z};
        const F4 C = ld4(vw->center);
        const float den = dot3(nq, F3{X.x - C.x, X.y - C.y, X.z - C.z});
        const float num = dot3(nq, F3{X0q.x - C.x, X0q.y - C.y, X0q.z - C.z});
        if (!mesh_finite_nonzero(den)) continue;
        const float s = num / den;
        const float dz = dot4(ld4(vw->oaxis), X1);
        if (!(dz > 0.0f)) continue;
        const float sd = (s - 1.0f) * dz;
        if (!(sd >= -vol.trunc)) continue;
        sum = sum + fminf(sd / vol.trunc, 1.0f);
        n = n + 1;
    }
    count[p] = n;
    tsdf[p] = n > 0 ? sum / (float)n : __int_as_float(0x7fc00000);
}

__global__ __launch_bounds__(256) void k_mesh_state(int64_t npoints, const float* __restrict__ tsdf, const int32_t* __restrict__ count, int min_count,
                                                    uint8_t* __restrict__ state) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= npoints) return;
    const float f = tsdf[p];
    const bool obs = f == f && (!count || count[p] >= min_count);
    state[p] = (uint8_t)((obs ? 1 : 0) | (obs && f < 0.0f ? 2 : 0));
}

__global__ __launch_bounds__(256) void k_mesh_edges(MeshVol vol, int64_t npoints, const uint8_t* __restrict__ state, uint8_t* __restrict__ mask,
                                                    int32_t* __restrict__ cnt) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= npoints) return;
    const MeshIdx ix = mesh_idx(vol, p);
    const uint32_t sa = state[p];
    uint32_t m = 0;
    if (sa & 1u) {
        const bool ex = ix.i + 1 < vol.nx, ey = ix.j + 1 < vol.ny, ez = ix.k + 1 < vol.nz;
#pragma unroll
        for (int d = 1; d < 8; ++d) {
            if (((d & 1) && !ex) || ((d & 2) && !ey) || ((d & 4) && !ez)) continue;
            const uint32_t sb = state[mesh_step(vol, p, d)];
            if ((sb & 1u) && ((sa ^ sb) & 2u)) m |= 1u << (d - 1);
        }
    }
    mask[p] = (uint8_t)m;
    cnt[p] = __popc(m);
}

// t = Fa / (Fa - Fb), pos = pa + t (pb - pa) per component
__global__ __launch_bounds__(256) void k_mesh_verts(MeshVol vol, int64_t npoints, const float* __restrict__ tsdf, const uint8_t* __restrict__ mask,
                                                    const int32_t* __restrict__ vbase, float* __restrict__ verts, int64_t cap_v) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= npoints) return;
    const uint32_t m = mask[p];
    if (!m) return;
    const MeshIdx ix = mesh_idx(vol, p);
    const F3 pa = mesh_pos(vol, ix.i, ix.j, ix.k);
    const float Fa = tsdf[p];
    int64_t k = vbase[p];
#pragma unroll
    for (int d = 1; d < 8; ++d) {
        if (!(m & (1u << (d - 1)))) continue;
        const float Fb = tsdf[mesh_step(vol, p, d)];
        const F3 pb = mesh_pos(vol, ix.i + (d & 1), ix.j + ((d >> 1) & 1), ix.k + ((d >> 2) & 1));
        const float t = Fa / (Fa - Fb);
        if (k >= 0 && k < cap_v) {
            verts[3 * k] = pa.x + t * (pb.x - pa.x);
            verts[3 * k + 1] = pa.y + t * (pb.y - pa.y);
            verts[3 * k + 2] = pa.z + t * (pb.z - pa.z);
        }
        ++k;
    }
}

// The six tetrahedra of the Kuhn split as cube corners, four bits each from the lowest position up: (0,1,3,7) (0,1,5,7) (0,2,3,7)
// (0,2,6,7) (0,4,5,7) (0,4,6,7).  Along a tetrahedron every corner's bits contain those of the one before, so the edge between positions
// x < y starts at corner x and runs in direction corner y - corner x.
DEV int mesh_tet_corner(int t, int x) {
    const uint32_t tets[6] = {0x7310u, 0x7510u, 0x7320u, 0x7620u, 0x7540u, 0x7640u};
    return (int)((tets[t] >> (4 * x)) & 15u);
}
// Bit m of a tetrahedron's word, m = the INSIDE flags of its four positions: the triangles of that case, in the order the contract lists
// their vertices, face the inside corners and are emitted with the second and third vertex swapped.  Decided on the edge midpoints; the
// two classes are the two handednesses of the split's tetrahedra.
DEV bool mesh_tet_flip(int t, uint32_t m) {
    const uint32_t flip[6] = {0x4d24u, 0x32dau, 0x32dau, 0x4d24u, 0x4d24u, 0x32dau};
    return (flip[t] >> m) & 1u;
}
// the corner states of the cube at p as eight INSIDE bits, or -1 when p has no cube or a corner is not OBSERVED
DEV int mesh_cube(const MeshVol& vol, int64_t p, const uint8_t* __restrict__ state) {
    const MeshIdx ix = mesh_idx(vol, p);
    if (!(ix.i + 1 < vol.nx && ix.j + 1 < vol.ny && ix.k + 1 < vol.nz)) return -1;
    uint32_t all = 1u, in = 0u;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const uint32_t s = state[mesh_step(vol, p, c)];
        all &= s;
        in |= ((s >> 1) & 1u) << c;
    }
    return all ? (int)in : -1;
}
DEV uint32_t mesh_tet_case(int t, int in) {
    uint32_t m = 0;
#pragma unroll
    for (int x = 0; x < 4; ++x) m |= (((uint32_t)in >> mesh_tet_corner(t, x)) & 1u) << x;
    return m;
}

__global__ __launch_bounds__(256) void k_mesh_tcount(MeshVol vol, int64_t npoints, const uint8_t* __restrict__ state, int32_t* __restrict__ cnt) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= npoints) return;
    const int in = mesh_cube(vol, p, state);
    int n = 0;
    if (in > 0 && in < 255) {
#pragma unroll
        for (int t = 0; t < 6; ++t) {
            const uint32_t m = mesh_tet_case(t, in);
            if (m != 0u && m != 15u) n += __popc(m) == 2 ? 2 : 1;
        }
    }
    cnt[p] = n;
}

// the vertex on the edge between positions x and y of tetrahedron t of the cube at p
DEV int32_t mesh_edge_vertex(const MeshVol& vol, int64_t p, int t, int x, int y, const uint8_t* __restrict__ mask, const int32_t* __restrict__ vbase) {
    const int lo = mesh_tet_corner(t, x < y ? x : y), hi = mesh_tet_corner(t, x < y ? y : x);
    const int64_t q = mesh_step(vol, p, lo);
    const int slot = hi - lo - 1;
    return vbase[q] + __popc((uint32_t)mask[q] & ((1u << slot) - 1u));
}

__global__ __launch_bounds__(256) void k_mesh_tris(MeshVol vol, int64_t npoints, const uint8_t* __restrict__ state, const uint8_t* __restrict__ mask,
                                                   const int32_t* __restrict__ vbase, const int64_t* __restrict__ tbase, int32_t* __restrict__ tris,
                                                   int64_t cap_t) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= npoints) return;
    const int in = mesh_cube(vol, p, state);
    if (!(in > 0 && in < 255)) return;
    int64_t k = tbase[p];
    for (int t = 0; t < 6; ++t) {
        const uint32_t m = mesh_tet_case(t, in);
        if (m == 0u || m == 15u) continue;
        const bool flip = mesh_tet_flip(t, m);
        int32_t q[4];
        int nq;
        if (__popc(m) == 2) {
            // inside a < b, outside c < d: e(a,c), e(a,d), e(b,d), e(b,c)
            const int a = __ffs(m) - 1, b = 31 - __clz(m);
            const uint32_t o = ~m & 15u;
            const int c = __ffs(o) - 1, d = 31 - __clz(o);
            q[0] = mesh_edge_vertex(vol, p, t, a, c, mask, vbase);
            q[1] = mesh_edge_vertex(vol, p, t, a, d, mask, vbase);
            q[2] = mesh_edge_vertex(vol, p, t, b, d, mask, vbase);
            q[3] = mesh_edge_vertex(vol, p, t, b, c, mask, vbase);
            nq = 4;
        } else {
            // the corner a that differs from the other three, those ascending
            const int a = __ffs(__popc(m) == 1 ? m : (~m & 15u)) - 1;
            int n = 0;
            for (int x = 0; x < 4; ++x)
                if (x != a) q[n++] = mesh_edge_vertex(vol, p, t, a, x, mask, vbase);
            q[3] = 0;
            nq = 3;
        }
        for (int f = 0; f + 2 < nq; ++f, ++k) {
            if (k < 0 || k >= cap_t) continue;
            tris[3 * k] = q[0];
            tris[3 * k + 1] = flip ? q[f + 2] : q[f + 1];
            tris[3 * k + 2] = flip ? q[f + 1] : q[f + 2];
        }
    }
}


void mvsk_mesh_tsdf(const DParams& prm, const MapsArgs& a, const MeshVol& vol, const int32_t* ids, const uint8_t* usable, float* tsdf, int32_t* count,
                    hipStream_t st) {
    const int64_t n = mesh_npoints(vol);
    hipLaunchKernelGGL(k_mesh_tsdf, dim3(nblk(n, 256)), dim3(256), 0, st, prm, a, vol, n, ids, usable, tsdf, count);
}
void mvsk_mesh_state(const MeshVol& vol, const float* tsdf, const int32_t* count, uint8_t* state, hipStream_t st) {
    const int64_t n = mesh_npoints(vol);
    hipLaunchKernelGGL(k_mesh_state, dim3(nblk(n, 256)), dim3(256), 0, st, n, tsdf, count, vol.min_count, state);
}
void mvsk_mesh_edges(const MeshVol& vol, const uint8_t* state, uint8_t* mask, int32_t* cnt, hipStream_t st) {
    const int64_t n = mesh_npoints(vol);
    hipLaunchKernelGGL(k_mesh_edges, dim3(nblk(n, 256)), dim3(256), 0, st, vol, n, state, mask, cnt);
}
void mvsk_mesh_verts(const MeshVol& vol, const float* tsdf, const uint8_t* mask, const int32_t* vbase, float* verts, int64_t cap_v, hipStream_t st) {
    const int64_t n = mesh_npoints(vol);
    hipLaunchKernelGGL(k_mesh_verts, dim3(nblk(n, 256)), dim3(256), 0, st, vol, n, tsdf, mask, vbase, verts, cap_v);
}
void mvsk_mesh_tcount(const MeshVol& vol, const uint8_t* state, int32_t* cnt, hipStream_t st) {
    const int64_t n = mesh_npoints(vol);
    hipLaunchKernelGGL(k_mesh_tcount, dim3(nblk(n, 256)), dim3(256), 0, st, vol, n, state, cnt);
}
void mvsk_mesh_tris(const MeshVol& vol, const uint8_t* state, const uint8_t* mask, const int32_t* vbase, const int64_t* tbase, int32_t* tris,
                    int64_t cap_t, hipStream_t st) {
    const int64_t n = mesh_npoints(vol);
    hipLaunchKernelGGL(k_mesh_tris, dim3(nblk(n, 256)), dim3(256), 0, st, vol, n, state, mask, vbase, tbase, tris, cap_t);
}
