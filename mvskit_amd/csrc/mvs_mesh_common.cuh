// mvs_mesh_common.cuh -- what the mesh units behind the extraction (mvs_mesh_attr.hip, mvs_mesh_clean.hip, mvs_mesh_decimate.hip,
// mvs_mesh_fill.hip, mvs_mesh_render.hip and mvs_mesh_texture.hip) share: the block and launch of a lane-per-item kernel, the 64-bit
// wave shuffles, the open-addressing table of 64-bit keys, the lanes of a wave that share the first one's key, and the order-free fixed-point sum (a
// power-of-two scale from the bits of the largest component, three 31-bit integers a position, the block maximum that finds the scale).
// No other unit includes this file, the sweep's (which includes mvs_common.cuh) least of all: nothing here can reach its code.
// Every function is force-inlined, and every kernel that uses one holds the machine code it held with the helper's lines written into
// it.  Where a kernel's code moved through a helper it kept its own lines, and says so: the table's lookup (k_mdec_find,
// k_mfill_classify), the sum of a first_group in the wave (k_mdec_sum, k_mfill_sum), finite3 in k_mdec_member.
#pragma once
#include "mvs_common.cuh"
#include "mvs_wave.cuh"

#define MESH_BLOCK 256
#define MESH_EMPTY 0xffffffffffffffffull  // the key of a free table slot, and of an item without a key
// a lane per item of n, on the launcher's stream `st`; nothing for n == 0
#define MESH_LAUNCH(kernel, n, ...) \
    do { if ((n) > 0) hipLaunchKernelGGL(kernel, dim3(nblk(n, MESH_BLOCK)), dim3(MESH_BLOCK), 0, st, __VA_ARGS__); } while (0)

namespace mvsdev {

typedef unsigned long long u64;

DEV bool finite3(F3 d) {
    const float inf = __int_as_float(0x7f800000);
    return fabsf(d.x) < inf && fabsf(d.y) < inf && fabsf(d.z) < inf;
}

// a 64-bit value from another lane, as two 32-bit shuffles
DEV u64 shfl_xor64(u64 v, int off) {
    return (u64)(uint32_t)__shfl_xor((int)(uint32_t)v, off) | (u64)(uint32_t)__shfl_xor((int)(v >> 32), off) << 32;
}
DEV u64 shfl_up1_64(u64 v) {
    return (u64)(uint32_t)__shfl_up((int)(uint32_t)v, 1) | (u64)(uint32_t)__shfl_up((int)(v >> 32), 1) << 32;
}

// splitmix64's finaliser: keys that are neighbours (the cells of a grid, the edges of one vertex) land far apart in the table
DEV u64 hash64(u64 k) {
    k ^= k >> 30; k *= 0xbf58476d1ce4e5b9ull;
    k ^= k >> 27; k *= 0x94d049bb133111ebull;
    return k ^ (k >> 31);
}

// The open-addressing table: tkey holds mask + 1 slots, MESH_EMPTY before the first claim; a slot never changes once it is taken, and a
// probe walks on linearly for at most mask + 1 steps.
// table_claim: the slot that holds k, taken with a 64-bit compare-and-swap (after a plain look) or found taken by k; false when the
// probe ran out.  What goes into the slot's value is the caller's: an atomic minimum of the index in decimation, an add of 1 in filling.
DEV bool table_claim(u64 k, u64* tkey, u64 mask, u64& slot) {
    u64 h = hash64(k) & mask;
    for (u64 step = 0; step <= mask; ++step) {
        u64 cur = __atomic_load_n(&tkey[h], __ATOMIC_RELAXED);
        if (cur == MESH_EMPTY) cur = atomicCAS(&tkey[h], MESH_EMPTY, k);
        if (cur == MESH_EMPTY || cur == k) { slot = h; return true; }
        h = (h + 1) & mask;
    }
    return false;
}

// the lanes with r >= 0 that share the r of the first such lane: `same` for the calling lane, their ballot in `group`
DEV bool first_group(int32_t r, u64& group) {
    const u64 active = ballot(r >= 0);
    const int first = active != 0ull ? __ffsll((long long)active) - 1 : 0;
    const int32_t r0 = __shfl(r, first);
    const bool same = r >= 0 && r == r0;
    group = ballot(same);
    return same;
}

// E = floor(log2 M) for the float M > 0 with bits mb (a subnormal M has its exponent in its leading bit); 2^k as a double.  With
// S = pow2(30 - E) every |component| <= M times S is below 2^31, and the product is exact
DEV int exponent(uint32_t mb) { return mb >= 0x00800000u ? (int)(mb >> 23) - 127 : (31 - __clz(mb)) - 149; }
DEV double pow2(int k) { return __longlong_as_double((long long)(1023 + k) << 52); }
DEV long long quantise(float v, double S) { return __double2ll_rn((double)v * S); }
struct Q3 { long long x, y, z; };
DEV Q3 quantise3(F3 d, double S) { return Q3{quantise(d.x, S), quantise(d.y, S), quantise(d.z, S)}; }

// The block's maximum of m, the bits of a non-negative float (they order as the floats do), into *mbits: a wave maximum, a block maximum
// through the kernel's own __shared__ uint32_t wave_max[MESH_BLOCK / 64], then one integer atomic max a block.  Every thread of the block
// calls it.  In two halves for the kernel that has work of its own between them (k_mattr_scan).
DEV uint32_t block_max_waves(uint32_t m, uint32_t* wave_max) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, off));
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
    if (lane == 0) wave_max[wave] = m;
    return m;
}
DEV void block_max_atomic(uint32_t m, const uint32_t* wave_max, uint32_t* __restrict__ mbits) {
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < MESH_BLOCK / 64; ++w) m = max(m, wave_max[w]);
        if (m != 0u) atomicMax(mbits, m);
    }
}
DEV void block_max(uint32_t m, uint32_t* wave_max, uint32_t* __restrict__ mbits) { block_max_atomic(block_max_waves(m, wave_max), wave_max, mbits); }

}  // namespace mvsdev
