// mvs_common.cuh -- what two or more of the kernel units (mvs_*.hip) share and that needs nothing of a patch's arithmetic: the block
// count of a launch, the sortable form of a float, the lock-free union-find.  (What the units that sample a patch share beyond this:
// mvs_patch_common.cuh.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mvs_math.cuh"

// blocks of b threads that cover n items
static inline unsigned nblk(int64_t n, int b) { return (unsigned)((n + b - 1) / b); }

namespace mvsdev {

// a float as an unsigned integer of the same order: the keys of k_depth_maps, k_best_ncc_map, k_maps_select and the index build
DEV uint32_t sortable_f32(float f) {
    uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// Lock-free union-find over ids (filterSmallGroups in mvs_filter.cuh, the mesh components in mvs_mesh_clean.hip): path halving on the
// way up, the smaller root adopts the larger, so a root is the smallest id of its set in whatever order the hardware met the edges.
DEV int uf_find(int* parent, int a) {
    while (true) {
        const int pa = __atomic_load_n(&parent[a], __ATOMIC_RELAXED);
        if (pa == a) return a;
        const int gp = __atomic_load_n(&parent[pa], __ATOMIC_RELAXED);
        if (gp != pa) __atomic_store_n(&parent[a], gp, __ATOMIC_RELAXED);
        a = pa;
    }
}
DEV void uf_union(int* parent, int a, int b) {
    while (true) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return;
        if (a > b) { const int t = a; a = b; b = t; }
        if (atomicCAS(&parent[b], b, a) == b) return;
    }
}

}  // namespace mvsdev
