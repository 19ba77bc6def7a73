// mvs_common.cuh -- what two or more of the kernel units (mvs_*.hip) share and mvs_device.cuh, the arithmetic of a patch, has no place
// for: the block count of a launch, the sortable form of a float, the lock-free union-find, the launch bound of the kernels that refine,
// and the LDS a wave needs for setRefImage's textures.
#pragma once
#include "mvs_device.cuh"

// blocks of b threads that cover n items
static inline unsigned nblk(int64_t n, int b) { return (unsigned)((n + b - 1) / b); }

#ifndef MVS_SWEEP_WAVES
#define MVS_SWEEP_WAVES 3  // waves per SIMD the register allocator is asked to fit: 168 VGPRs (4 waves = 128 VGPRs spills ~110 of them; measured 19.4 vs 18.9 M patches/s)
#endif

// setRefImage: the centred textures of MVS_LISTCAP views (9408 B at wsize 7 and 16 views) + one value per view pair;
// in postProcess they lie behind the frame region (the evaluation that produces them publishes its frames there).
// The 32- and 64-view builds keep one chunk of MVS_GRAM_CH views at a time and overlay the Gram matrix on it (mvs_device.cuh).
// (mvsk_sweep_lds_bytes in mvs_sweep.cuh and mvsk_texs_lds_bytes in mvs_filter.cuh start from this.)
static inline size_t texs_gram_lds_bytes(const DParams& prm) {
#if MVS_PAIR_MFMA
    const size_t tex_f = (size_t)MVS_GRAM_CH * 3 * prm.wsz, gram_f = (size_t)prm.gram_ld * prm.gram_ld;
    return MVS_FRAME1_LDS_BYTES + (tex_f > gram_f ? tex_f : gram_f) * sizeof(float);
#else
    const size_t ln = (size_t)prm.list_n;  // min(MVS_LISTCAP, nviews): a 12-view data set keeps 12 textures, not 16
    return MVS_FRAME1_LDS_BYTES + (ln * 3 * prm.wsz + ln * (ln - 1) / 2) * sizeof(float);
#endif
}

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
