// mvs_patch_common.cuh -- what the parts of the unit that samples patches (mvs_sweep.cuh, mvs_filter.cuh, mvs_probe.cuh) share on top of
// the patch arithmetic: the launch bound of the kernels that refine, and the LDS a wave needs for setRefImage's textures.
#pragma once
#include "mvs_device.cuh"
#include "mvs_common.cuh"

#ifndef MVS_SWEEP_WAVES
#define MVS_SWEEP_WAVES 3  // waves per SIMD the register allocator is asked to fit: 168 VGPRs (4 waves = 128 VGPRs spills ~110 of them; measured 19.4 vs 18.9 M patches/s)
#endif

// setRefImage: the centred textures of MVS_LISTCAP views (9408 B at wsize 7 and 16 views) + one value per view pair;
// in postProcess they lie behind the frame region (the evaluation that produces them publishes its frames there).
// The 32- and 64-view builds keep one chunk of MVS_GRAM_CH views at a time and overlay the Gram matrix on it (mvs_eval.cuh).
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
