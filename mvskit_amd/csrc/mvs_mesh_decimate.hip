// mvs_mesh_decimate.hip -- vertex clustering of a triangle mesh on a caller's grid (mvs_engine_mesh_decimate in mvs_engine_mesh.cpp
// drives it; the definition is in include/mvskit_engine.h).  A lane per triangle or per vertex, 256-thread blocks.  No sort: clusters
// and duplicate triangles are both found with one open-addressing table of 64-bit keys that is filled, read and cleared three times.
//   k_mdec_used      a lane per triangle: used[id] = 1 for its three ids (plain stores of one value)
//   k_mdec_member    a lane per vertex: the packed cell of a member (all ones for an unused vertex), one atomic OR per wave that met a
//                    member that is not finite or lies outside the grid, and the largest |component| of the members, through block_max
//   k_mdec_insert    a lane per item: its key claims a slot of the table (table_claim: a 64-bit compare-and-swap after a plain look, a
//                    slot never changes once it is taken), the item's index goes into the slot's value by a 32-bit atomic minimum.  A lane whose
//                    left neighbour in the wave carries the same key leaves both to that neighbour, whose index is smaller: the members
//                    of a cell follow each other in a mesh that came from a lattice, and a mesh that lies in one cell costs one pair of
//                    atomics a wave instead of 64 on one word
//   k_mdec_find      a lane per item: the value of its key's slot (-1 for an item without a key)
//   k_mdec_tkey1     a lane per triangle: its three representatives sorted to a < b < c, the key (a << 30) | b; all ones when two of them
//                    are equal (COLLAPSED)
//   k_mdec_tkey2     a lane per surviving triangle: the key (e << 30) | c, e = the smallest triangle index with the same (a, b)
//   k_mdec_keep      a lane per triangle: kept when it is the smallest triangle index with its (e, c); a 1 on each of its representatives
//   k_mdec_sum       a lane per member: its position scaled to 31-bit integers and added to its representative's row, three 64-bit
//                    integer atomic adds and one count.  The lanes of a wave that share the first member's representative (first_group)
//                    are summed in the wave first (integer addition is associative) and add once
//   k_mdec_mean      a lane per flagged representative: the mean in fp64 and the cast, at the row the scan gives it; one member: its bytes
//   k_mdec_nearest   a lane per member of a flagged cluster: a 64-bit unsigned atomic minimum over (bits(d2) << 32) | id, the wave's lanes
//                    that share the first one's representative reduced first
//   k_mdec_pick      a lane per flagged representative: the bytes of the member that won
//   k_mdec_vmap / k_mdec_tgather   the vertex map; the kept triangles behind the scan of their flags, ids rewritten
// Every probe loop ends after as many steps as the table has slots and raises *fail when it found nothing.  The atomics are vector
// memory atomics, none but the compare-and-swap returns a value; stores are plain vector stores.  fp32 / fp64 without contraction.
#include <hip/hip_runtime.h>

#include "mvs_mesh_common.cuh"
#include "mvs_kernels.h"

using namespace mvsdev;

#define MDEC_GMAX 1048576  // 2^20: a cell index lies in -2^20 .. 2^20 - 1

__global__ __launch_bounds__(MESH_BLOCK) void k_mdec_used(int64_t n_t, const int32_t* __restrict__ tris, int32_t* __restrict__ used) {
    const int64_t t = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (t >= n_t) return;
    used[tris[3 * t]] = 1; used[tris[3 * t + 1]] = 1; used[tris[3 * t + 2]] = 1;
}

// g = floorf((x - o) / cell) when it lies in the grid; ok cleared otherwise (a NaN fails both comparisons)
DEV uint32_t mdec_cell(float x, float o, float cell, bool& ok) {
    const float g = floorf((x - o) / cell);
    ok = ok && g >= -(float)MDEC_GMAX && g <= (float)(MDEC_GMAX - 1);
    return ok ? (uint32_t)((int)g + MDEC_GMAX) : 0u;
}

__global__ __launch_bounds__(MESH_BLOCK) void k_mdec_member(int64_t n_v, const float* __restrict__ x, const int32_t* __restrict__ used, float ox, float oy, float oz,
                                                            float cell, u64* __restrict__ key, uint32_t* __restrict__ mbits, uint32_t* __restrict__ bad) {
    __shared__ uint32_t wave_max[MESH_BLOCK / 64];
    const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    uint32_t m = 0;
    bool wrong = false;
    if (i < n_v) {
        u64 k = MESH_EMPTY;
        if (used[i] != 0) {
            const F3 p = ld3(x + 3 * i);
            const float inf = __int_as_float(0x7f800000);
            bool ok = fabsf(p.x) < inf && fabsf(p.y) < inf && fabsf(p.z) < inf;  // finite3 restated: through the helper this kernel's machine code changed
            const uint32_t gx = mdec_cell(p.x, ox, cell, ok), gy = mdec_cell(p.y, oy, cell, ok), gz = mdec_cell(p.z, oz, cell, ok);
            wrong = !ok;
            if (ok) {
                k = (u64)gx << 42 | (u64)gy << 21 | (u64)gz;
                m = __float_as_uint(fmaxf(fmaxf(fabsf(p.x), fabsf(p.y)), fabsf(p.z)));
            }
        }
        key[i] = k;
    }
    if (ballot(wrong) != 0ull && lane_id() == 0) atomicOr(bad, 1u);
    block_max(m, wave_max, mbits);
}

// tkey: mask + 1 slots, all ones before the first insert; tval: their values, at least 2^30 before it
__global__ __launch_bounds__(MESH_BLOCK) void k_mdec_insert(int64_t n, const u64* __restrict__ key, u64* tkey, int32_t* tval, u64 mask,
                                                            uint32_t* __restrict__ fail) {
    const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    const u64 k = i < n ? key[i] : MESH_EMPTY;
    const u64 left = shfl_up1_64(k);  // every lane of the wave is here
    if (k == MESH_EMPTY || (lane_id() != 0 && left == k)) return;
    u64 h;
    if (table_claim(k, tkey, mask, h)) atomicMin(&tval[h], (int32_t)i);
    else atomicOr(fail, 1u);
}

__global__ __launch_bounds__(MESH_BLOCK) void k_mdec_find(int64_t n, const u64* __restrict__ key, const u64* __restrict__ tkey,
                                                          const int32_t* __restrict__ tval, u64 mask, int32_t* __restrict__ out, uint32_t* __restrict__ fail) {
    const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (i >= n) return;
    const u64 k = key[i];
    int32_t v = -1;
    if (k != MESH_EMPTY) {
        // the lookup restated, not a helper of mvs_mesh_common.cuh: through one (four spellings) this kernel's machine code changed
        bool found = false;
        u64 h = hash64(k) & mask;
        for (u64 step = 0; step <= mask; ++step) {
            const u64 cur = tkey[h];
            if (cur == k) { v = tval[h]; found = true; break; }
            if (cur == MESH_EMPTY) break;
            h = (h + 1) & mask;
        }
        if (!found) atomicOr(fail, 1u);
    }
    out[i] = v;
}

// the three representatives of triangle t, every id a member's: rep >= 0 (k_mdec_tkey1 lets no other triangle through)
struct MdecTri { int32_t a, b, c; };
DEV MdecTri mdec_reps(const int32_t* __restrict__ tris, const int32_t* __restrict__ rep, int64_t t) {
    return MdecTri{rep[tris[3 * t]], rep[tris[3 * t + 1]], rep[tris[3 * t + 2]]};
}

__global__ __launch_bounds__(MESH_BLOCK) void k_mdec_tkey1(int64_t n_t, const int32_t* __restrict__ tris, const int32_t* __restrict__ rep, u64* __restrict__ key) {
    const int64_t t = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (t >= n_t) return;
    const MdecTri r = mdec_reps(tris, rep, t);
    const int32_t lo = min(r.a, min(r.b, r.c)), hi = max(r.a, max(r.b, r.c));
    const int32_t mid = (int32_t)((int64_t)r.a + r.b + r.c - lo - hi);
    const bool collapsed = r.a == r.b || r.b == r.c || r.a == r.c || lo < 0;  // lo < 0: a cell that was not found, the host refuses
    key[t] = collapsed ? MESH_EMPTY : ((u64)(uint32_t)lo << 30 | (u64)(uint32_t)mid);
}

// first[t]: the smallest triangle index with t's (a, b); -1 for a collapsed triangle, whose key stays all ones
__global__ __launch_bounds__(MESH_BLOCK) void k_mdec_tkey2(int64_t n_t, const int32_t* __restrict__ tris, const int32_t* __restrict__ rep,
                                                           const int32_t* __restrict__ first, u64* __restrict__ key) {
    const int64_t t = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (t >= n_t) return;
    const int32_t e = first[t];
    if (e < 0) return;
    const MdecTri r = mdec_reps(tris, rep, t);
    key[t] = (u64)(uint32_t)e << 30 | (u64)(uint32_t)max(r.a, max(r.b, r.c));
}

// winner[t]: the smallest triangle index with t's three clusters (-1: collapsed); vflag zero before the launch
__global__ __launch_bounds__(MESH_BLOCK) void k_mdec_keep(int64_t n_t, const int32_t* __restrict__ tris, const int32_t* __restrict__ rep,
                                                          const int32_t* __restrict__ winner, int32_t* __restrict__ tflag, int32_t* __restrict__ vflag) {
    const int64_t t = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (t >= n_t) return;
    const bool keep = (int64_t)winner[t] == t;
    tflag[t] = keep ? 1 : 0;
    if (keep) {
        const MdecTri r = mdec_reps(tris, rep, t);
        vflag[r.a] = 1; vflag[r.b] = 1; vflag[r.c] = 1;
    }
}

// rep[i] >= 0: vertex i is a member and rep[i] its cluster's smallest member; acc and cnt zero before the launch
__global__ __launch_bounds__(MESH_BLOCK) void k_mdec_sum(int64_t n_v, const float* __restrict__ x, const int32_t* __restrict__ rep, const uint32_t* __restrict__ mbits,
                                                         u64* __restrict__ acc, int32_t* __restrict__ cnt) {
    const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    const uint32_t mb = *mbits;
    if (mb == 0u) return;  // every member is (0, 0, 0): uniform over the grid
    const int32_t r = i < n_v ? rep[i] : -1;
    long long qx = 0, qy = 0, qz = 0;
    if (r >= 0) {
        const double S = pow2(30 - exponent(mb));
        qx = quantise(x[3 * i], S); qy = quantise(x[3 * i + 1], S); qz = quantise(x[3 * i + 2], S);
    }
    u64 group;
    const bool same = first_group(r, group);
    int32_t n = 1;
    if (__popcll(group) > 1) {  // uniform over the wave; the sum restated here and in k_mfill_sum: through a helper both kernels' machine code changed
        u64 sx = same ? (u64)qx : 0ull, sy = same ? (u64)qy : 0ull, sz = same ? (u64)qz : 0ull;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { sx += shfl_xor64(sx, off); sy += shfl_xor64(sy, off); sz += shfl_xor64(sz, off); }
        if (same) {
            if (lane_id() != __ffsll((long long)group) - 1) return;
            qx = (long long)sx; qy = (long long)sy; qz = (long long)sz; n = (int32_t)__popcll(group);
        }
    }
    if (r < 0) return;
    atomicAdd(acc + 3 * (int64_t)r, (u64)qx);
    atomicAdd(acc + 3 * (int64_t)r + 1, (u64)qy);
    atomicAdd(acc + 3 * (int64_t)r + 2, (u64)qz);
    atomicAdd(cnt + r, n);
}

// p = (float)(((double)A * 2^(E - 30)) / (double)n) at out[3 vbase[i] ..] for every flagged representative i; n == 1, and every cluster
// when M == 0, copies the representative's bytes
__global__ __launch_bounds__(MESH_BLOCK) void k_mdec_mean(int64_t n_v, const uint32_t* __restrict__ xbits, const int32_t* __restrict__ vflag,
                                                          const int32_t* __restrict__ vbase, const uint32_t* __restrict__ mbits, const long long* __restrict__ acc,
                                                          const int32_t* __restrict__ cnt, float* __restrict__ out, int64_t cap_v) {
    const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (i >= n_v || vflag[i] == 0) return;
    const int64_t k = vbase[i];
    if (k >= cap_v) return;
    const uint32_t mb = *mbits;
    const int32_t n = cnt[i];
    if (mb == 0u || n <= 1) {
        uint32_t* o = reinterpret_cast<uint32_t*>(out);
        o[3 * k] = xbits[3 * i]; o[3 * k + 1] = xbits[3 * i + 1]; o[3 * k + 2] = xbits[3 * i + 2];
        return;
    }
    const double back = pow2(exponent(mb) - 30), nd = (double)n;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[3 * k + c] = (float)(((double)acc[3 * i + c] * back) / nd);
}

// out: k_mdec_mean's rows; best all ones before the launch
__global__ __launch_bounds__(MESH_BLOCK) void k_mdec_nearest(int64_t n_v, const float* __restrict__ x, const int32_t* __restrict__ rep, const int32_t* __restrict__ vflag,
                                                             const int32_t* __restrict__ vbase, const float* __restrict__ out, int64_t cap_v, u64* __restrict__ best) {
    const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    int32_t r = i < n_v ? rep[i] : -1;
    if (r >= 0 && (vflag[r] == 0 || (int64_t)vbase[r] >= cap_v)) r = -1;
    u64 w = MESH_EMPTY;
    if (r >= 0) {
        const int64_t k = vbase[r];
        const float dx = x[3 * i] - out[3 * k], dy = x[3 * i + 1] - out[3 * k + 1], dz = x[3 * i + 2] - out[3 * k + 2];
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        w = (u64)__float_as_uint(d2) << 32 | (u64)(uint32_t)i;
    }
    u64 group;
    const bool same = first_group(r, group);
    if (__popcll(group) > 1) {  // uniform over the wave
        u64 m = same ? w : MESH_EMPTY;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { const u64 o = shfl_xor64(m, off); m = o < m ? o : m; }
        if (same) {
            if (lane_id() != __ffsll((long long)group) - 1) return;
            w = m;
        }
    }
    if (r < 0) return;
    atomicMin(best + r, w);
}

__global__ __launch_bounds__(MESH_BLOCK) void k_mdec_pick(int64_t n_v, const uint32_t* __restrict__ xbits, const int32_t* __restrict__ vflag,
                                                          const int32_t* __restrict__ vbase, const u64* __restrict__ best, uint32_t* __restrict__ out, int64_t cap_v) {
    const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (i >= n_v || vflag[i] == 0) return;
    const int64_t k = vbase[i];
    if (k >= cap_v) return;
    const int64_t j = (int64_t)(best[i] & 0xffffffffull);
    if (j >= n_v) return;  // no member answered: the mean stays
    out[3 * k] = xbits[3 * j]; out[3 * k + 1] = xbits[3 * j + 1]; out[3 * k + 2] = xbits[3 * j + 2];
}

__global__ __launch_bounds__(MESH_BLOCK) void k_mdec_vmap(int64_t n_v, const int32_t* __restrict__ rep, const int32_t* __restrict__ vflag,
                                                          const int32_t* __restrict__ vbase, int32_t* __restrict__ vmap) {
    const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (i >= n_v) return;
    const int32_t r = rep[i];
    vmap[i] = (r >= 0 && vflag[r] != 0) ? vbase[r] : -1;
}

__global__ __launch_bounds__(MESH_BLOCK) void k_mdec_tgather(int64_t n_t, const int32_t* __restrict__ tris, const int32_t* __restrict__ rep,
                                                             const int32_t* __restrict__ tflag, const int32_t* __restrict__ tbase, const int32_t* __restrict__ vbase,
                                                             int32_t* __restrict__ out, int64_t cap_t) {
    const int64_t t = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (t >= n_t || tflag[t] == 0) return;
    const int64_t k = tbase[t];
    if (k >= cap_t) return;
    const MdecTri r = mdec_reps(tris, rep, t);
    out[3 * k] = vbase[r.a]; out[3 * k + 1] = vbase[r.b]; out[3 * k + 2] = vbase[r.c];
}

void mvsk_mdec_members(int64_t n_v, const float* verts, int64_t n_t, const int32_t* tris, const float* origin, float cell, int32_t* used,
                       unsigned long long* key, uint32_t* mbits, uint32_t* bad, hipStream_t st) {
    MESH_LAUNCH(k_mdec_used, n_t, n_t, tris, used);
    MESH_LAUNCH(k_mdec_member, n_v, n_v, verts, used, origin[0], origin[1], origin[2], cell, key, mbits, bad);
}
void mvsk_mdec_table(int64_t n, const unsigned long long* key, unsigned long long* tkey, int32_t* tval, int64_t slots, int32_t* out, uint32_t* fail,
                     hipStream_t st) {
    MESH_LAUNCH(k_mdec_insert, n, n, key, tkey, tval, (u64)(slots - 1), fail);
    MESH_LAUNCH(k_mdec_find, n, n, key, tkey, tval, (u64)(slots - 1), out, fail);
}
void mvsk_mdec_tkey1(int64_t n_t, const int32_t* tris, const int32_t* rep, unsigned long long* key, hipStream_t st) {
    MESH_LAUNCH(k_mdec_tkey1, n_t, n_t, tris, rep, key);
}
void mvsk_mdec_tkey2(int64_t n_t, const int32_t* tris, const int32_t* rep, const int32_t* first, unsigned long long* key, hipStream_t st) {
    MESH_LAUNCH(k_mdec_tkey2, n_t, n_t, tris, rep, first, key);
}
void mvsk_mdec_keep(int64_t n_t, const int32_t* tris, const int32_t* rep, const int32_t* winner, int32_t* tflag, int32_t* vflag, hipStream_t st) {
    MESH_LAUNCH(k_mdec_keep, n_t, n_t, tris, rep, winner, tflag, vflag);
}
void mvsk_mdec_positions(int placement, int64_t n_v, const float* verts, const int32_t* rep, const int32_t* vflag, const int32_t* vbase, const uint32_t* mbits,
                         long long* acc, int32_t* cnt, unsigned long long* best, float* out_verts, int64_t cap_v, hipStream_t st) {
    MESH_LAUNCH(k_mdec_sum, n_v, n_v, verts, rep, mbits, reinterpret_cast<u64*>(acc), cnt);
    MESH_LAUNCH(k_mdec_mean, n_v, n_v, reinterpret_cast<const uint32_t*>(verts), vflag, vbase, mbits, acc, cnt, out_verts, cap_v);
    if (placement != 1) return;
    MESH_LAUNCH(k_mdec_nearest, n_v, n_v, verts, rep, vflag, vbase, out_verts, cap_v, best);
    MESH_LAUNCH(k_mdec_pick, n_v, n_v, reinterpret_cast<const uint32_t*>(verts), vflag, vbase, best, reinterpret_cast<uint32_t*>(out_verts), cap_v);
}
void mvsk_mdec_gather(int64_t n_v, const int32_t* rep, const int32_t* vflag, const int32_t* vbase, int32_t* vmap, int64_t n_t, const int32_t* tris,
                      const int32_t* tflag, const int32_t* tbase, int32_t* out_tris, int64_t cap_t, hipStream_t st) {
    MESH_LAUNCH(k_mdec_vmap, n_v, n_v, rep, vflag, vbase, vmap);
    MESH_LAUNCH(k_mdec_tgather, n_t, n_t, tris, rep, tflag, tbase, vbase, out_tris, cap_t);
}
