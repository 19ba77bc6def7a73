// mvs_seed_random.hip -- the cold start: seed patches from random plane hypotheses, scored and refined on the device, appended to the pool
// in (view, cell) order (mvs_engine_seed_random in mvs_engine.cpp drives it).  No reference counterpart: the reference starts from a depth
// point cloud (DepthNormInit::createPatches, mvs_seed.hip); this is PatchMatch stereo's usual start for a user who has images, masks and
// cameras only.  A job is a cell of a view; one wave per job, one launch per view.
//   k_seed_random_hyp     the diagnostic window (mvs_engine_seed_random_hypotheses): lane k writes hypothesis k of a listed cell as a record
//   k_seed_random         lane k builds hypothesis k of the wave's cell -- the SAME device function -- and parks its plane in LDS; the wave
//                         then walks the K hypotheses through Optim::preProcess and PatchManager::computeNcc, keeps the best one, refines it
//                         (the engine's refiner) and runs Optim::postProcess; a patch that passes is staged at stage[cell], keep[cell] = 1
//   k_seed_random_gather  stage[cell] -> dst[base[cell]] (base = the exclusive scan of keep: no atomic decides a position)
// The stages are the device functions of the sweep, called as mvs_engine_probe's ops 1, 0, 2 and 3 call them (k_probe, k_probe_refine,
// k_probe_refine_simplex in mvs_kernels.hip), and between two stages the candidate goes through a record (store_cand / load_cand, in LDS)
// as it does between two probe calls: a kept record has the bits that chain of probes gives.  Optim::check never runs here.
#include <hip/hip_runtime.h>

#include "mvs_check.cuh"  // Filter::ortho
#include "mvs_kernels.h"

using namespace mvsdev;

// Hypothesis k of cell `cell` of view a.view: the plane (coord, normal) of the record.  Five draws u_j in [-0.5, 0.5) of the call's own
// stream, rng_uniform(seed, 0x5eed0001, view, cell, k, j):
//   pixel   the cell centre of sweep_cell, jittered by csize * (u0, u1) as the sweep's fill trial jitters it
//   depth   uniform in inverse depth over [dmin, dmax] along the optical axis: w = 1/dmax + (u2 + 0.5)(1/dmin - 1/dmax), d = 1/w, held
//           inside the range against the rounding of the two reciprocals; coord = unproject(d * (px, py, 1))
//   normal  tilted by theta = max_tilt sqrt(u3 + 0.5) (uniform over the cap's disc) from r, the unit vector towards the camera centre, in
//           the direction phi = 2 pi (u4 + 0.5) of Filter::ortho's frame (e1, e2) of r; sin and cos of phi are those of 2 pi u4, which
//           lies in pm_sincosf's range, negated.  n = cos(theta) r + sin(theta)(cos(phi) e1 + sin(phi) e2), normalised; n.w = -coord . n
DEV void seed_random_hypothesis(const DParams& prm, const SeedRandomArgs& a, int cell, int k, F4& coord, F4& normal) {
    const DView* vw = prm.views + a.view;
    const int gw = vw->gw;
    const int cx = cell % gw, cy = cell / gw;
    const float icx = (float)(prm.csize * (2 * cx + 1) - 1) / 2.0f, icy = (float)(prm.csize * (2 * cy + 1) - 1) / 2.0f;
    float u[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) u[j] = rng_uniform(a.seed, 0x5eed0001u, (uint32_t)a.view, (uint32_t)cell, (uint32_t)k, (uint32_t)j);
    const float px = icx + u[0] * (float)prm.csize, py = icy + u[1] * (float)prm.csize;
    const float wmin = rcp_rn(a.dmax), wmax = rcp_rn(a.dmin);
    const float w = fma_(u[2] + 0.5f, wmax - wmin, wmin);
    const float d = fminf(fmaxf(rcp_rn(w), a.dmin), a.dmax);
    coord = unproject(vw, F3{d * px, d * py, d}, prm.level);
    const F4 r = nrm4(sub4(ld4(vw->center), coord));
    F4 e1, e2;
    ortho(r, e1, e2);
    const float theta = a.max_tilt * sqrt_rn(u[3] + 0.5f);
    float st, ct, sp, cp;
    pm_sincosf(theta, st, ct);
    pm_sincosf(2.0f * MVS_PI * u[4], sp, cp);
    sp = -sp; cp = -cp;
    const F4 t{fma_(sp, e2.x, cp * e1.x), fma_(sp, e2.y, cp * e1.y), fma_(sp, e2.z, cp * e1.z), 0.0f};
    F4 n = nrm4(F4{fma_(st, t.x, ct * r.x), fma_(st, t.y, ct * r.y), fma_(st, t.z, ct * r.z), 0.0f});
    n.w = -dot3(F3{coord.x, coord.y, coord.z}, F3{n.x, n.y, n.z});
    normal = n;
}

// the record of a hypothesis, written by one lane: m_images = [view], no m_vimages, m_ncc = -1, scales and m_tmp 0, alive, id = k
DEV void seed_random_record(DPatch* rec, F4 coord, F4 normal, int view, int k) {
    rec->coord[0] = coord.x; rec->coord[1] = coord.y; rec->coord[2] = coord.z; rec->coord[3] = coord.w;
    rec->normal[0] = normal.x; rec->normal[1] = normal.y; rec->normal[2] = normal.z; rec->normal[3] = normal.w;
    rec->ncc = -1.0f; rec->dscale = 0.0f; rec->ascale = 0.0f; rec->tmp = 0.0f;
    rec->nimages = 1; rec->nvimages = 0; rec->flags = MVS_FLAG_ALIVE; rec->id = k;
    for (int j = 0; j < MVS_MAXI; ++j) { rec->images[j] = 0; rec->vimages[j] = 0; }
    rec->images[0] = (uint8_t)view;
}
// hypothesis k as the wave's candidate: its record, written from the plane parked in LDS (8 floats), read back by load_cand itself
DEV void seed_random_cand(DPatch* rec, const float* plane, int view, int k, const WaveCtx& wc, Cand& c) {
    __syncthreads();
    if (wc.lane == 0) seed_random_record(rec, ld4(plane), ld4(plane + 4), view, k);
    __syncthreads();
    load_cand(rec, wc, c);
}
// a candidate between two stages: through a record, as between two probe calls (load_cand clears the lanes beyond the lists and the cells)
DEV void seed_random_roundtrip(DPatch* rec, const WaveCtx& wc, Cand& c) {
    __syncthreads();
    store_cand(rec, wc, c, MVS_FLAG_ALIVE, 0);
    __syncthreads();
    load_cand(rec, wc, c);
}

__global__ __launch_bounds__(64) void k_seed_random_hyp(DParams prm, SeedRandomArgs a, int64_t ncells, const int32_t* __restrict__ cells,
                                                        DPatch* __restrict__ out) {
    const int64_t i = blockIdx.x;
    if (i >= ncells) return;
    const int k = lane_id();
    if (k >= a.K) return;
    F4 coord, normal;
    seed_random_hypothesis(prm, a, cells[i], k, coord, normal);
    seed_random_record(out + i * a.K + k, coord, normal, a.view, k);
}

template <bool SIMPLEX>
__global__ __launch_bounds__(64) void k_seed_random(DParams prm, SeedRandomArgs a, int ncells, DPatch* __restrict__ stage, int32_t* __restrict__ keep) {
    __shared__ int s_scratch[192];
    __shared__ float s_hyp[64 * 8];
    __shared__ DPatch s_rec, s_win;
    extern __shared__ float s_texs[];
    const int cell = blockIdx.x;
    if (cell >= ncells) return;
    // the mask gate: the pixel of the cell centre at m_level lies inside the image and, where the view has a mask, on the foreground
    const DView* vw = prm.views + a.view;
    {
        const int gw = vw->gw, W = vw->W[prm.level], H = vw->H[prm.level];
        const int cx = cell % gw, cy = cell / gw;
        const float icx = (float)(prm.csize * (2 * cx + 1) - 1) / 2.0f, icy = (float)(prm.csize * (2 * cy + 1) - 1) / 2.0f;
        const float fx = floorf(icx + 0.5f), fy = floorf(icy + 0.5f);
        if (!(fx >= 0.0f && fx < (float)W && fy >= 0.0f && fy < (float)H)) return;
        if (vw->mask && vw->mask[(size_t)(int)fy * W + (int)fx] == 0) return;
    }
    WaveCtx wc = make_wave_ctx(prm);
    if (wc.lane < a.K) {
        F4 coord, normal;
        seed_random_hypothesis(prm, a, cell, wc.lane, coord, normal);
        float* h = s_hyp + 8 * wc.lane;
        h[0] = coord.x; h[1] = coord.y; h[2] = coord.z; h[3] = coord.w;
        h[4] = normal.x; h[5] = normal.y; h[6] = normal.z; h[7] = normal.w;
    }
    __syncthreads();
    // the winner: the highest score strictly above min_ncc, the lowest k among equals (a NaN never wins)
    float best = a.min_ncc;
    bool have = false;
    for (int k = 0; k < a.K; ++k) {
        Cand c;
        seed_random_cand(&s_rec, s_hyp + 8 * k, a.view, k, wc, c);
        if (pre_process(prm, wc, s_scratch, c) != 0) continue;
        seed_random_roundtrip(&s_rec, wc, c);
        const float ncc = rlf(compute_ncc(prm, wc, c.coord, c.normal, c.img, c.nimg), 0);
        if (ncc > best) {
            best = ncc; have = true;
            __syncthreads();
            store_cand(&s_win, wc, c, MVS_FLAG_ALIVE, 0);
        }
    }
    if (!have) return;
    __syncthreads();
    Cand c;
    load_cand(&s_win, wc, c);
    if constexpr (SIMPLEX) (void)refine_patch_simplex(prm, wc, c, a.max_evals, a.xtol);  // a spent budget leaves the start
    else refine_patch(prm, wc, c, 0u, 0u, (uint32_t)cell, 0u);
    seed_random_roundtrip(&s_rec, wc, c);
    if (post_process(prm, wc, s_scratch, s_texs, prm.wsz, c) != 0) return;
    store_cand(stage + cell, wc, c, MVS_FLAG_ALIVE, 0);
    if (wc.lane == 0) keep[cell] = 1;
}

__global__ __launch_bounds__(256) void k_seed_random_gather(const DPatch* __restrict__ stage, const int32_t* __restrict__ keep, const int32_t* __restrict__ base,
                                                            int n, DPatch* __restrict__ dst, int32_t id0) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !keep[i]) return;
    const int32_t o = base[i];
    const uint4* s4 = reinterpret_cast<const uint4*>(stage + i);
    uint4* d4 = reinterpret_cast<uint4*>(dst + o);
    for (int w = 0; w < (int)MVS_REC_U4; ++w) d4[w] = s4[w];
    dst[o].flags = MVS_FLAG_ALIVE; dst[o].id = id0 + o;
}

void mvsk_seed_random_hypotheses(const DParams& prm, const SeedRandomArgs& a, int64_t ncells, const int32_t* cells, DPatch* out, hipStream_t st) {
    if (ncells > 0) hipLaunchKernelGGL(k_seed_random_hyp, dim3((unsigned)ncells), dim3(64), 0, st, prm, a, ncells, cells, out);
}
// keep[0, ncells) must be zero: a job that gives no patch writes nothing
void mvsk_seed_random(const DParams& prm, const SeedRandomArgs& a, int ncells, DPatch* stage, int32_t* keep, hipStream_t st) {
    if (ncells <= 0) return;
    const size_t lds = mvsk_texs_lds_bytes(prm);  // postProcess' kept textures behind the frames, as Filter::filterExact: no Optim::check here
    if (a.simplex) hipLaunchKernelGGL(k_seed_random<true>, dim3((unsigned)ncells), dim3(64), lds, st, prm, a, ncells, stage, keep);
    else hipLaunchKernelGGL(k_seed_random<false>, dim3((unsigned)ncells), dim3(64), lds, st, prm, a, ncells, stage, keep);
}
void mvsk_seed_random_gather(const DPatch* stage, const int32_t* keep, const int32_t* base, int ncells, DPatch* dst, int32_t id0, hipStream_t st) {
    if (ncells > 0) hipLaunchKernelGGL(k_seed_random_gather, dim3((unsigned)((ncells + 255) / 256)), dim3(256), 0, st, stage, keep, base, ncells, dst, id0);
}
