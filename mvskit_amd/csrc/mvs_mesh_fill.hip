// mvs_mesh_fill.hip -- the boundary loops of a triangle mesh and their filling with centroid fans (mvs_engine_mesh_boundaries and
// mvs_engine_mesh_fill in mvs_engine_mesh.cpp drive it; the definitions are in include/mvskit_engine.h).  A lane per triangle, per
// vertex or per table slot, 256-thread blocks.  No sort: the directed edges are counted in one open-addressing table of 64-bit keys,
// the loops are the components of a union-find over the boundary half-edges, and the fill triangles lie behind a scan over the vertices.
//   k_mfill_init       a lane per vertex: parent[i] = i
//   k_mfill_edges      a lane per triangle with three different ids: each directed edge a -> b claims the slot of its key (a << 30) | b
//                      with table_claim (a plain look, then a 64-bit compare-and-swap: a slot never changes once it is taken) and
//                      adds 1 to the slot's count
//   k_mfill_classify   a lane per slot, so once per distinct directed edge: one lookup of the reverse key.  (1, 0) is a boundary
//                      half-edge: out[a] += 1, in[b] += 1, next[a] = b, and the union of a and b (the smaller id becomes the root).
//                      Anything but (1, 1) and (1, 0) is irregular: a 1 on both ends, and the pair counted where a < b or the reverse
//                      is absent, one add per wave
//   (k_mclean_flatten  of mvs_mesh_clean.hip, through mvsk_mesh_flatten: parent[i] = its root, found without path compression)
//   k_mfill_count      a lane per vertex on a boundary: hed[root] += out[i], and a 1 on the root when the vertex is not simple.  The rim
//                      of an open surface puts tens of thousands of adds on one root: the lanes that share the first such lane's root
//                      (first_group) are summed in the wave first and add once
//   k_mfill_spread     a lane per vertex: its label and its component's length (negated when complex); the loops and the complex
//                      components counted at their roots, one add per wave and kind
//   k_mfill_plan       a lane per vertex: the fill triangles it is the origin of (0 or 1) and whether it brings a new vertex (the label
//                      of a filled loop of 4 or more), for the two scans; one atomic OR per wave that met a non-finite vertex of a
//                      filled loop; the filled loops counted at their labels; the largest |component| of the vertices whose loop gets a
//                      centroid, through block_max
//   k_mfill_sum        a lane per vertex of such a loop: its position scaled to 31-bit integers (quantise3) and added to the label's row,
//                      three 64-bit integer atomic adds, the lanes of a wave that share the first one's label summed in the wave first
//                      (first_group)
//   k_mfill_emit       a lane per vertex of a filled loop: its triangle at the row the scan gives it; the label's lane the centroid in
//                      fp64 and the cast
// Every probe loop ends after as many steps as the table has slots and raises *fail when it found nothing.  The atomics are vector
// memory atomics, none but the compare-and-swaps returns a value; stores are plain vector stores.  fp32 / fp64 without contraction.
#include <hip/hip_runtime.h>

#include "mvs_mesh_common.cuh"
#include "mvs_kernels.h"

using namespace mvsdev;

#define MFILL_IDMASK 0x3fffffffull

DEV u64 mfill_key(int32_t a, int32_t b) { return (u64)(uint32_t)a << 30 | (u64)(uint32_t)b; }

__global__ __launch_bounds__(MESH_BLOCK) void k_mfill_init(int64_t n_v, int* __restrict__ parent) {
    const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (i < n_v) parent[i] = (int)i;
}

// tkey: mask + 1 slots, all ones before the launch; tval: their counts, zero before it
DEV void mfill_insert(u64 k, u64* tkey, int32_t* tval, u64 mask, uint32_t* __restrict__ fail) {
    u64 h;
    if (table_claim(k, tkey, mask, h)) atomicAdd(&tval[h], 1);
    else atomicOr(fail, 1u);
}

__global__ __launch_bounds__(MESH_BLOCK) void k_mfill_edges(int64_t n_t, const int32_t* __restrict__ tris, u64* tkey, int32_t* tval, u64 mask,
                                                             uint32_t* __restrict__ fail) {
    const int64_t t = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (t >= n_t) return;
    const int32_t a = tris[3 * t], b = tris[3 * t + 1], c = tris[3 * t + 2];
    if (a == b || b == c || a == c) return;  // no edges here
    mfill_insert(mfill_key(a, b), tkey, tval, mask, fail);
    mfill_insert(mfill_key(b, c), tkey, tval, mask, fail);
    mfill_insert(mfill_key(c, a), tkey, tval, mask, fail);
}

// outc, inc, cplx, next zero before the launch, parent[i] = i; the table is only read
__global__ __launch_bounds__(MESH_BLOCK) void k_mfill_classify(int64_t slots, const u64* __restrict__ tkey, const int32_t* __restrict__ tval, u64 mask,
                                                                int32_t* __restrict__ outc, int32_t* __restrict__ inc, int32_t* __restrict__ cplx,
                                                                int32_t* __restrict__ next, int* parent, u64* __restrict__ nirr, uint32_t* __restrict__ fail) {
    const int64_t s = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    const u64 k = s < slots ? tkey[s] : MESH_EMPTY;
    bool counted = false;
    if (k != MESH_EMPTY) {
        const int32_t a = (int32_t)(k >> 30), b = (int32_t)(k & MFILL_IDMASK);
        const int32_t f = tval[s];
        const u64 rk = mfill_key(b, a);
        int32_t r = 0;
        // the lookup restated, not a helper of mvs_mesh_common.cuh: through one (four spellings) this kernel's machine code changed
        bool ended = false;
        u64 h = hash64(rk) & mask;
        for (u64 step = 0; step <= mask; ++step) {
            const u64 cur = tkey[h];
            if (cur == rk) { r = tval[h]; ended = true; break; }
            if (cur == MESH_EMPTY) { ended = true; break; }
            h = (h + 1) & mask;
        }
        if (!ended) atomicOr(fail, 1u);
        if (f == 1 && r == 0) {  // BOUNDARY
            atomicAdd(outc + a, 1);
            atomicAdd(inc + b, 1);
            next[a] = b;  // read only where out[a] == 1: one writer
            uf_union(parent, a, b);
        } else if (!(f == 1 && r == 1)) {  // IRREGULAR
            cplx[a] = 1; cplx[b] = 1;
            counted = a < b || r == 0;
        }
    }
    const u64 m = ballot(counted);
    if (m != 0ull && lane_id() == __ffsll((long long)m) - 1) atomicAdd(nirr, (u64)__popcll(m));
}

// hed and rbad zero before the launch
__global__ __launch_bounds__(MESH_BLOCK) void k_mfill_count(int64_t n_v, const int* __restrict__ parent, const int32_t* __restrict__ outc, const int32_t* __restrict__ inc,
                                                             const int32_t* __restrict__ cplx, int32_t* __restrict__ hed, int32_t* __restrict__ rbad) {
    const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    int32_t r = -1, o = 0;
    if (i < n_v) {
        o = outc[i];
        const int32_t n = inc[i];
        if (o > 0 || n > 0) {
            r = parent[i];
            if (!(o == 1 && n == 1 && cplx[i] == 0)) rbad[r] = 1;
        }
    }
    u64 group;
    const bool same = first_group(r, group);
    if (__popcll(group) > 1) {  // uniform over the wave
        int32_t sum = same ? o : 0;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
        if (same) {
            if (lane_id() != __ffsll((long long)group) - 1) return;
            o = sum;
        }
    }
    if (r < 0 || o == 0) return;
    atomicAdd(hed + r, o);
}

// counts[0] += the loops, counts[1] += the complex components
__global__ __launch_bounds__(MESH_BLOCK) void k_mfill_spread(int64_t n_v, const int* __restrict__ parent, const int32_t* __restrict__ outc, const int32_t* __restrict__ inc,
                                                              const int32_t* __restrict__ hed, const int32_t* __restrict__ rbad, int32_t* __restrict__ loop,
                                                              int32_t* __restrict__ length, u64* __restrict__ counts) {
    const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    bool is_loop = false, is_complex = false;
    if (i < n_v) {
        int32_t l = -1, len = 0;
        if (outc[i] > 0 || inc[i] > 0) {
            l = parent[i];
            const bool cx = rbad[l] != 0;
            len = cx ? -hed[l] : hed[l];
            is_loop = l == (int32_t)i && !cx;
            is_complex = l == (int32_t)i && cx;
        }
        loop[i] = l; length[i] = len;
    }
    const u64 ml = ballot(is_loop), mc = ballot(is_complex);
    if (ml != 0ull && lane_id() == __ffsll((long long)ml) - 1) atomicAdd(counts, (u64)__popcll(ml));
    if (mc != 0ull && lane_id() == __ffsll((long long)mc) - 1) atomicAdd(counts + 1, (u64)__popcll(mc));
}

DEV bool mfill_filled(int32_t len, int32_t max_edges) { return len >= 3 && len <= max_edges; }

// *mbits, *bad, *nfilled zero before the launch
__global__ __launch_bounds__(MESH_BLOCK) void k_mfill_plan(int64_t n_v, const float* __restrict__ x, const int32_t* __restrict__ loop, const int32_t* __restrict__ length,
                                                            int32_t max_edges, int32_t* __restrict__ tcnt, int32_t* __restrict__ vcnt, uint32_t* __restrict__ mbits,
                                                            uint32_t* __restrict__ bad, u64* __restrict__ nfilled) {
    __shared__ uint32_t wave_max[MESH_BLOCK / 64];
    const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    uint32_t m = 0;
    bool wrong = false, label = false;
    if (i < n_v) {
        const int32_t len = length[i];
        int32_t tc = 0, vc = 0;
        if (mfill_filled(len, max_edges)) {
            label = loop[i] == (int32_t)i;
            tc = (len >= 4 || label) ? 1 : 0;
            vc = (len >= 4 && label) ? 1 : 0;
            const F3 p = ld3(x + 3 * i);
            wrong = !finite3(p);
            if (!wrong && len >= 4) m = __float_as_uint(fmaxf(fmaxf(fabsf(p.x), fabsf(p.y)), fabsf(p.z)));
        }
        tcnt[i] = tc; vcnt[i] = vc;
    }
    if (ballot(wrong) != 0ull && lane_id() == 0) atomicOr(bad, 1u);
    const u64 ml = ballot(label);
    if (ml != 0ull && lane_id() == __ffsll((long long)ml) - 1) atomicAdd(nfilled, (u64)__popcll(ml));
    block_max(m, wave_max, mbits);
}

// acc zero before the launch; every vertex of a filled loop finite (the host refuses otherwise)
__global__ __launch_bounds__(MESH_BLOCK) void k_mfill_sum(int64_t n_v, const float* __restrict__ x, const int32_t* __restrict__ loop, const int32_t* __restrict__ length,
                                                           int32_t max_edges, const uint32_t* __restrict__ mbits, u64* __restrict__ acc) {
    const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    const uint32_t mb = *mbits;
    if (mb == 0u) return;  // every such vertex is (0, 0, 0): uniform over the grid
    int32_t r = -1;
    if (i < n_v) {
        const int32_t len = length[i];
        if (len >= 4 && mfill_filled(len, max_edges)) r = loop[i];
    }
    long long qx = 0, qy = 0, qz = 0;
    if (r >= 0) {
        const double S = pow2(30 - exponent(mb));
        qx = quantise(x[3 * i], S); qy = quantise(x[3 * i + 1], S); qz = quantise(x[3 * i + 2], S);
    }
    u64 group;
    const bool same = first_group(r, group);
    if (__popcll(group) > 1) {  // uniform over the wave; the sum restated here and in k_mdec_sum: through a helper both kernels' machine code changed
        u64 sx = same ? (u64)qx : 0ull, sy = same ? (u64)qy : 0ull, sz = same ? (u64)qz : 0ull;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { sx += shfl_xor64(sx, off); sy += shfl_xor64(sy, off); sz += shfl_xor64(sz, off); }
        if (same) {
            if (lane_id() != __ffsll((long long)group) - 1) return;
            qx = (long long)sx; qy = (long long)sy; qz = (long long)sz;
        }
    }
    if (r < 0) return;
    atomicAdd(acc + 3 * (int64_t)r, (u64)qx);
    atomicAdd(acc + 3 * (int64_t)r + 1, (u64)qy);
    atomicAdd(acc + 3 * (int64_t)r + 2, (u64)qz);
}

// tbase / vbase: the exclusive scans of k_mfill_plan's counts.  add_tris: the rows behind the n_t input triangles, add_verts: those behind
// the n_v input vertices; nothing at or beyond cap_t / cap_v.  Length 3, a -> b -> c -> a with a the label: (b, a, c) at a's row.  Length
// >= 4: (b, a, w) at a's row for every half-edge a -> b, w = n_v + vbase[label]; p = (float)(((double)A * 2^(E - 30)) / (double)length),
// +0 in all three components when M == 0
__global__ __launch_bounds__(MESH_BLOCK) void k_mfill_emit(int64_t n_v, const int32_t* __restrict__ loop, const int32_t* __restrict__ length, int32_t max_edges,
                                                            const int32_t* __restrict__ next, const int32_t* __restrict__ tbase, const int32_t* __restrict__ vbase,
                                                            const uint32_t* __restrict__ mbits, const long long* __restrict__ acc, int32_t* __restrict__ add_tris,
                                                            int64_t cap_t, float* __restrict__ add_verts, int64_t cap_v) {
    const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (i >= n_v) return;
    const int32_t len = length[i];
    if (!mfill_filled(len, max_edges)) return;
    const int32_t a = (int32_t)i, l = loop[i], b = next[i];
    const int64_t k = tbase[i];
    if (len >= 4) {
        const int64_t row = vbase[l];
        if (k < cap_t) { add_tris[3 * k] = b; add_tris[3 * k + 1] = a; add_tris[3 * k + 2] = (int32_t)(n_v + row); }
        if (l != a || row >= cap_v) return;
        const uint32_t mb = *mbits;
        if (mb == 0u) { add_verts[3 * row] = 0.0f; add_verts[3 * row + 1] = 0.0f; add_verts[3 * row + 2] = 0.0f; return; }
        const double back = pow2(exponent(mb) - 30), nd = (double)len;
#pragma unroll
        for (int c = 0; c < 3; ++c) add_verts[3 * row + c] = (float)(((double)acc[3 * i + c] * back) / nd);
    } else if (l == a && k < cap_t) {
        add_tris[3 * k] = b; add_tris[3 * k + 1] = a; add_tris[3 * k + 2] = next[b];
    }
}

void mvsk_mfill_boundaries(int64_t n_v, int64_t n_t, const int32_t* tris, unsigned long long* tkey, int32_t* tval, int64_t slots, int32_t* parent, int32_t* outc,
                           int32_t* inc, int32_t* cplx, int32_t* next, int32_t* hed, int32_t* rbad, int32_t* loop, int32_t* length, unsigned long long* counts,
                           uint32_t* fail, hipStream_t st) {
    MESH_LAUNCH(k_mfill_init, n_v, n_v, parent);
    if (n_t > 0) {
        MESH_LAUNCH(k_mfill_edges, n_t, n_t, tris, tkey, tval, (u64)(slots - 1), fail);
        MESH_LAUNCH(k_mfill_classify, slots, slots, tkey, tval, (u64)(slots - 1), outc, inc, cplx, next, parent, counts + 2, fail);
        mvsk_mesh_flatten(n_v, parent, st);
        MESH_LAUNCH(k_mfill_count, n_v, n_v, parent, outc, inc, cplx, hed, rbad);
    }
    MESH_LAUNCH(k_mfill_spread, n_v, n_v, parent, outc, inc, hed, rbad, loop, length, counts);
}
void mvsk_mfill_plan(int64_t n_v, const float* verts, const int32_t* loop, const int32_t* length, int32_t max_edges, int32_t* tcnt, int32_t* vcnt, uint32_t* mbits,
                     uint32_t* bad, unsigned long long* nfilled, hipStream_t st) {
    MESH_LAUNCH(k_mfill_plan, n_v, n_v, verts, loop, length, max_edges, tcnt, vcnt, mbits, bad, nfilled);
}
void mvsk_mfill_emit(int64_t n_v, const float* verts, const int32_t* loop, const int32_t* length, int32_t max_edges, const int32_t* next, const int32_t* tbase,
                     const int32_t* vbase, const uint32_t* mbits, long long* acc, int32_t* add_tris, int64_t cap_t, float* add_verts, int64_t cap_v, hipStream_t st) {
    MESH_LAUNCH(k_mfill_sum, n_v, n_v, verts, loop, length, max_edges, mbits, reinterpret_cast<u64*>(acc));
    MESH_LAUNCH(k_mfill_emit, n_v, n_v, loop, length, max_edges, next, tbase, vbase, mbits, acc, add_tris, cap_t, add_verts, cap_v);
}
