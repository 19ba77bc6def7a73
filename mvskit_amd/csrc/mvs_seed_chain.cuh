// mvs_seed_chain.cuh -- what the seeding front ends share on the device: the cold start (mvs_seed_random.hip, a job is a cell) and the warm
// start (mvs_seed_points.hip, a job is a point).  A front end gates its job, builds its hypotheses -- planes with a reference view each --
// and parks them in LDS; seed_chain then walks them through Optim::preProcess and PatchManager::computeNcc, keeps the best one, refines it
// (the engine's refiner) and runs Optim::postProcess; a patch that passes is staged with its keep flag set.
// The stages are the device functions of the sweep, called as mvs_engine_probe's ops 1, 0, 2 and 3 call them (k_probe, k_probe_refine,
// k_probe_refine_simplex in mvs_probe.cuh), and between two stages the candidate goes through a record (store_cand / load_cand, in LDS)
// as it does between two probe calls: a kept record has the bits that chain of probes gives.  Optim::check never runs here.
#pragma once
#include "mvs_device.cuh"

namespace mvsdev {

// The foreground gate of the pixel position (x, y) of view `vw` at m_level: the pixel floorf(. + 0.5f) lies inside the image at that level
// and, where the view has a mask, on its foreground.  The bounds are tested on the floats: a NaN passes nowhere.
DEV bool seed_foreground(const DParams& prm, const DView* vw, float x, float y) {
    const int W = vw->W[prm.level], H = vw->H[prm.level];
    const float fx = floorf(x + 0.5f), fy = floorf(y + 0.5f);
    if (!(fx >= 0.0f && fx < (float)W && fy >= 0.0f && fy < (float)H)) return false;
    if (vw->mask && vw->mask[(size_t)(int)fy * W + (int)fx] == 0) return false;
    return true;
}

// the record of a hypothesis, written by one lane: m_images = [view], no m_vimages, m_ncc = -1, scales and m_tmp 0, alive, id = k
DEV void seed_record(DPatch* rec, F4 coord, F4 normal, int view, int k) {
    rec->coord[0] = coord.x; rec->coord[1] = coord.y; rec->coord[2] = coord.z; rec->coord[3] = coord.w;
    rec->normal[0] = normal.x; rec->normal[1] = normal.y; rec->normal[2] = normal.z; rec->normal[3] = normal.w;
    rec->ncc = -1.0f; rec->dscale = 0.0f; rec->ascale = 0.0f; rec->tmp = 0.0f;
    rec->nimages = 1; rec->nvimages = 0; rec->flags = MVS_FLAG_ALIVE; rec->id = k;
    for (int j = 0; j < MVS_MAXI; ++j) { rec->images[j] = 0; rec->vimages[j] = 0; }
    rec->images[0] = (uint8_t)view;
}

// The LDS of a job's wave (one wave per block): the parked hypotheses -- plane k as 8 floats, its reference view -- and what the chain
// works in.  The cold start's hypotheses all have one view; handing it to the chain per hypothesis costs that kernel 256 B, which with
// one wave per block is far from limiting.
struct SeedChainLds {
    int scratch[192];
    float hyp[64 * 8];
    int view[64];
    DPatch rec, win;
};
// lane k parks hypothesis k
DEV void seed_park(SeedChainLds& s, int k, F4 coord, F4 normal, int view) {
    float* h = s.hyp + 8 * k;
    h[0] = coord.x; h[1] = coord.y; h[2] = coord.z; h[3] = coord.w;
    h[4] = normal.x; h[5] = normal.y; h[6] = normal.z; h[7] = normal.w;
    s.view[k] = view;
}
// hypothesis k as the wave's candidate: its record, written from the parked plane, read back by load_cand itself
DEV void seed_cand(SeedChainLds& s, int k, const WaveCtx& wc, Cand& c) {
    __syncthreads();
    if (wc.lane == 0) seed_record(&s.rec, ld4(s.hyp + 8 * k), ld4(s.hyp + 8 * k + 4), s.view[k], k);
    __syncthreads();
    load_cand(&s.rec, wc, c);
}
// a candidate between two stages: through a record, as between two probe calls (load_cand clears the lanes beyond the lists and the cells)
DEV void seed_roundtrip(SeedChainLds& s, const WaveCtx& wc, Cand& c) {
    __syncthreads();
    store_cand(&s.rec, wc, c, MVS_FLAG_ALIVE, 0);
    __syncthreads();
    load_cand(&s.rec, wc, c);
}

// The chain over the nh hypotheses parked in `s`, by a whole wave.  key: the job's HALVING draws (MVS_PROBE_REFINE's key for batch index
// `key`).  A patch that passes goes to *slot, and *kept = 1; a job that gives none writes neither.
template <bool SIMPLEX>
DEV void seed_chain(const DParams& prm, WaveCtx& wc, const SeedChainArgs& a, SeedChainLds& s, int nh, uint32_t key, DPatch* slot, int32_t* kept) {
    extern __shared__ float s_texs[];
    __syncthreads();
    // the winner: the highest score strictly above min_ncc, the lowest k among equals (a NaN never wins)
    float best = a.min_ncc;
    bool have = false;
    for (int k = 0; k < nh; ++k) {
        Cand c;
        seed_cand(s, k, wc, c);
        if (pre_process(prm, wc, s.scratch, c) != 0) continue;
        seed_roundtrip(s, wc, c);
        const float ncc = rlf(compute_ncc(prm, wc, c.coord, c.normal, c.img, c.nimg), 0);
        if (ncc > best) {
            best = ncc; have = true;
            __syncthreads();
            store_cand(&s.win, wc, c, MVS_FLAG_ALIVE, 0);
        }
    }
    if (!have) return;
    __syncthreads();
    Cand c;
    load_cand(&s.win, wc, c);
    if constexpr (SIMPLEX) (void)refine_patch_simplex(prm, wc, c, a.max_evals, a.xtol);  // a spent budget leaves the start
    else refine_patch(prm, wc, c, 0u, 0u, key, 0u);
    seed_roundtrip(s, wc, c);
    if (post_process(prm, wc, s.scratch, s_texs, prm.wsz, c) != 0) return;
    store_cand(slot, wc, c, MVS_FLAG_ALIVE, 0);
    if (wc.lane == 0) *kept = 1;
}

}  // namespace mvsdev
