// mvs_mesh_seams.hip -- the adjacency of triangles and the view labels smoothed over it (mvs_engine_mesh_adjacency and
// mvs_engine_mesh_smooth_labels in mvs_engine_mesh.cpp drive it; the contract is in include/mvskit_seams.h).  A lane per triangle or
// per table slot, 256-thread blocks.  The kernels that need a view's texels (the seam sampler, the levelled atlas) are in
// mvs_mesh_texture.hip.
//   k_mseam_edges      a lane per triangle with three different ids: each directed edge a -> b claims the slot of its key (a << 30) | b
//                      with table_claim, adds 1 to the slot's count and stores its row as the slot's owner -- the owner is read only
//                      where the count is 1, one writer
//   k_mseam_nbr        a lane per triangle: per edge a lookup of its own key and of the reverse key; where both counts are 1 the
//                      reverse slot's owner, else -1
//   k_mseam_irregular  a lane per slot, so once per distinct directed edge: the irregular pairs as k_mfill_classify counts them, one add
//                      per wave
//   k_mseam_count      a lane per triangle: its seams towards neighbours of a higher row, summed in the wave, one add per wave
//   k_mseam_propose    a lane per triangle: three gathered neighbour labels, at most three bytes of quality; the proposal and its score
//                      (gain << 8) | quality, 0 without a gain
//   k_mseam_apply      a lane per triangle with a score: it moves when it beats every neighbour that has one; one add per wave to the
//                      iteration's move counter
// An iteration is a propose and an apply launch.  propose reads the labels and writes proposal and score; apply reads those and writes
// the labels: no kernel reads what the same launch writes, and none waits for another workgroup.  Both return at once when the iteration
// before moved nothing (its counter, written by an earlier launch): the host looks at a counter only every few iterations.  Every probe
// loop ends after as many steps as the table has slots and raises *fail when it found nothing.  Stores are plain vector stores.
#include <hip/hip_runtime.h>

#include "mvs_mesh_common.cuh"
#include "mvs_kernels.h"

using namespace mvsdev;

#define MSEAM_IDMASK 0x3fffffffull

DEV u64 mseam_key(int32_t a, int32_t b) { return (u64)(uint32_t)a << 30 | (u64)(uint32_t)b; }

DEV void mseam_insert(u64 k, int32_t row, u64* tkey, int32_t* tval, int32_t* town, u64 mask, uint32_t* __restrict__ fail) {
    u64 h;
    if (table_claim(k, tkey, mask, h)) { atomicAdd(&tval[h], 1); town[h] = row; }
    else atomicOr(fail, 1u);
}

// the slot of key k, or -1 when the table does not hold it; *fail when the probe ran out
DEV long long mseam_find(u64 k, const u64* __restrict__ tkey, u64 mask, uint32_t* __restrict__ fail) {
    u64 h = hash64(k) & mask;
    for (u64 step = 0; step <= mask; ++step) {
        const u64 cur = tkey[h];
        if (cur == k) return (long long)h;
        if (cur == MESH_EMPTY) return -1;
        h = (h + 1) & mask;
    }
    atomicOr(fail, 1u);
    return -1;
}

// tkey: mask + 1 slots, all ones before the launch; tval: their counts, zero before it; town: their owners
__global__ __launch_bounds__(MESH_BLOCK) void k_mseam_edges(int64_t n_t, const int32_t* __restrict__ tris, u64* tkey, int32_t* tval, int32_t* town, u64 mask,
                                                             uint32_t* __restrict__ fail) {
    const int64_t t = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (t >= n_t) return;
    const int32_t a = tris[3 * t], b = tris[3 * t + 1], c = tris[3 * t + 2];
    if (a == b || b == c || a == c) return;  // no edges here
    mseam_insert(mseam_key(a, b), (int32_t)t, tkey, tval, town, mask, fail);
    mseam_insert(mseam_key(b, c), (int32_t)t, tkey, tval, town, mask, fail);
    mseam_insert(mseam_key(c, a), (int32_t)t, tkey, tval, town, mask, fail);
}

__global__ __launch_bounds__(MESH_BLOCK) void k_mseam_nbr(int64_t n_t, const int32_t* __restrict__ tris, const u64* __restrict__ tkey,
                                                           const int32_t* __restrict__ tval, const int32_t* __restrict__ town, u64 mask,
                                                           int32_t* __restrict__ nbr, uint32_t* __restrict__ fail) {
    const int64_t t = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (t >= n_t) return;
    const int32_t id[3] = {tris[3 * t], tris[3 * t + 1], tris[3 * t + 2]};
    const bool edges = id[0] != id[1] && id[1] != id[2] && id[0] != id[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        int32_t u = -1;
        if (edges) {
            const int32_t a = id[k], b = id[(k + 1) % 3];
            const long long own = mseam_find(mseam_key(a, b), tkey, mask, fail);
            if (own >= 0 && tval[own] == 1) {
                const long long rev = mseam_find(mseam_key(b, a), tkey, mask, fail);
                if (rev >= 0 && tval[rev] == 1) u = town[rev];
            }
        }
        nbr[3 * t + k] = u;
    }
}

__global__ __launch_bounds__(MESH_BLOCK) void k_mseam_irregular(int64_t slots, const u64* __restrict__ tkey, const int32_t* __restrict__ tval, u64 mask,
                                                                 u64* __restrict__ nirr, uint32_t* __restrict__ fail) {
    const int64_t s = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    const u64 k = s < slots ? tkey[s] : MESH_EMPTY;
    bool counted = false;
    if (k != MESH_EMPTY) {
        const int32_t a = (int32_t)(k >> 30), b = (int32_t)(k & MSEAM_IDMASK);
        const int32_t f = tval[s];
        const long long rev = mseam_find(mseam_key(b, a), tkey, mask, fail);
        const int32_t r = rev >= 0 ? tval[rev] : 0;
        if (!(f == 1 && (r == 0 || r == 1))) counted = a < b || r == 0;
    }
    const u64 m = ballot(counted);
    if (m != 0ull && lane_id() == __ffsll((long long)m) - 1) atomicAdd(nirr, (u64)__popcll(m));
}

// *seams += the adjacent pairs (t, u), t < u, whose labels are both >= 0 and differ
__global__ __launch_bounds__(MESH_BLOCK) void k_mseam_count(int64_t n_t, const int32_t* __restrict__ nbr, const int32_t* __restrict__ label, u64* __restrict__ seams) {
    const int64_t t = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    int n = 0;
    if (t < n_t) {
        const int32_t own = label[t];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int32_t u = nbr[3 * t + k];
            if (u > t && own >= 0) {
                const int32_t l = label[u];
                n += (l >= 0 && l != own) ? 1 : 0;
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off);
    if (n != 0 && lane_id() == 0) atomicAdd(seams, (u64)n);
}

// moved: one counter an iteration; iteration `it` does nothing when iteration it - 1 moved nothing
__global__ __launch_bounds__(MESH_BLOCK) void k_mseam_propose(int it, const u64* __restrict__ moved, int64_t n_t, const int32_t* __restrict__ nbr,
                                                               const int32_t* __restrict__ label, int nviews_q, const uint8_t* __restrict__ quality, int keep,
                                                               int32_t* __restrict__ prop, int32_t* __restrict__ score) {
    if (it > 0 && moved[it - 1] == 0ull) return;
    const int64_t t = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (t >= n_t) return;
    const int32_t own = label[t];
    int32_t l[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int32_t u = nbr[3 * t + k];
        l[k] = u >= 0 ? label[u] : -1;
    }
    int best_a = 0, best_q = 0, best_l = -1, a_own = 0;
    if (own >= 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            a_own += l[k] == own ? 1 : 0;
            if (l[k] < 0 || l[k] == own) continue;
            const int q = quality[t * nviews_q + l[k]];
            if (q < keep) continue;
            const int a = (l[0] == l[k] ? 1 : 0) + (l[1] == l[k] ? 1 : 0) + (l[2] == l[k] ? 1 : 0);
            if (best_l < 0 || a > best_a || (a == best_a && (q > best_q || (q == best_q && l[k] < best_l)))) { best_a = a; best_q = q; best_l = l[k]; }
        }
    }
    const int gain = best_l >= 0 ? best_a - a_own : 0;
    prop[t] = best_l;
    score[t] = gain > 0 ? (gain << 8 | best_q) : 0;
}

// true when the ascending id triple of row t is lexicographically smaller than that of row u
DEV bool mseam_triple_less(const int32_t* __restrict__ tris, int64_t t, int64_t u) {
    int32_t x[3], y[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { x[k] = tris[3 * t + k]; y[k] = tris[3 * u + k]; }
    const int32_t x0 = min(x[0], min(x[1], x[2])), x2 = max(x[0], max(x[1], x[2])), y0 = min(y[0], min(y[1], y[2])), y2 = max(y[0], max(y[1], y[2]));
    const int64_t x1 = (int64_t)x[0] + x[1] + x[2] - x0 - x2, y1 = (int64_t)y[0] + y[1] + y[2] - y0 - y2;
    if (x0 != y0) return x0 < y0;
    if (x1 != y1) return x1 < y1;
    return x2 < y2;
}

__global__ __launch_bounds__(MESH_BLOCK) void k_mseam_apply(int it, u64* __restrict__ moved, int64_t n_t, const int32_t* __restrict__ tris,
                                                             const int32_t* __restrict__ nbr, const int32_t* __restrict__ prop, const int32_t* __restrict__ score,
                                                             int32_t* __restrict__ label) {
    if (it > 0 && moved[it - 1] == 0ull) return;
    const int64_t t = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    bool moves = false;
    if (t < n_t) {
        const int32_t mine = score[t];
        if (mine > 0) {
            moves = true;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int32_t u = nbr[3 * t + k];
                if (u < 0) continue;
                const int32_t theirs = score[u];
                if (theirs <= 0 || mine > theirs) continue;
                if (mine < theirs || !mseam_triple_less(tris, t, u)) moves = false;
            }
            if (moves) label[t] = prop[t];
        }
    }
    const u64 m = ballot(moves);
    if (m != 0ull && lane_id() == __ffsll((long long)m) - 1) atomicAdd(moved + it, (u64)__popcll(m));
}


void mvsk_mseam_adjacency(int64_t n_t, const int32_t* tris, unsigned long long* tkey, int32_t* tval, int32_t* town, int64_t slots, int32_t* nbr,
                          unsigned long long* nirr, uint32_t* fail, hipStream_t st) {
    MESH_LAUNCH(k_mseam_edges, n_t, n_t, tris, tkey, tval, town, (u64)(slots - 1), fail);
    MESH_LAUNCH(k_mseam_nbr, n_t, n_t, tris, tkey, tval, town, (u64)(slots - 1), nbr, fail);
    if (nirr && n_t > 0) MESH_LAUNCH(k_mseam_irregular, slots, slots, tkey, tval, (u64)(slots - 1), nirr, fail);
}
void mvsk_mseam_count(int64_t n_t, const int32_t* nbr, const int32_t* label, unsigned long long* seams, hipStream_t st) {
    MESH_LAUNCH(k_mseam_count, n_t, n_t, nbr, label, seams);
}
void mvsk_mseam_iteration(int it, unsigned long long* moved, int64_t n_t, const int32_t* tris, const int32_t* nbr, int nviews_q, const uint8_t* quality, int keep,
                          int32_t* prop, int32_t* score, int32_t* label, hipStream_t st) {
    MESH_LAUNCH(k_mseam_propose, n_t, it, moved, n_t, nbr, label, nviews_q, quality, keep, prop, score);
    MESH_LAUNCH(k_mseam_apply, n_t, it, moved, n_t, tris, nbr, prop, score, label);
}
