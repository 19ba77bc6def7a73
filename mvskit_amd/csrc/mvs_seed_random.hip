// mvs_seed_random.hip -- the cold start: seed patches from random plane hypotheses, scored and refined on the device, appended to the pool
// in (view, cell) order (mvs_engine_seed_random in mvs_engine.cpp drives it).  No reference counterpart: the reference starts from a depth
// point cloud (DepthNormInit::createPatches, mvs_seed.hip); this is PatchMatch stereo's usual start for a user who has images, masks and
// cameras only.  A job is a cell of a view; one wave per job, one launch per view.
//   k_seed_random_hyp  the diagnostic window (mvs_engine_seed_random_hypotheses): lane k writes hypothesis k of a listed cell as a record
//   k_seed_random      the gate of the cell centre; lane k builds hypothesis k of the wave's cell -- the SAME device function -- and parks
//                      it in LDS; seed_chain (mvs_seed_chain.cuh) scores the K hypotheses, refines the best one and stages a patch that
//                      passes at stage[cell], keep[cell] = 1
//   k_seed_gather      both front ends' staged append: stage[j] -> dst[base[j]] (base = the exclusive scan of keep: no atomic decides a
//                      position)
#include <hip/hip_runtime.h>

#include "mvs_check.cuh"  // Filter::ortho
#include "mvs_kernels.h"
#include "mvs_seed_chain.cuh"

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

__global__ __launch_bounds__(64) void k_seed_random_hyp(DParams prm, SeedRandomArgs a, int64_t ncells, const int32_t* __restrict__ cells,
                                                        DPatch* __restrict__ out) {
    const int64_t i = blockIdx.x;
    if (i >= ncells) return;
    const int k = lane_id();
    if (k >= a.chain.K) return;
    F4 coord, normal;
    seed_random_hypothesis(prm, a, cells[i], k, coord, normal);
    seed_record(out + i * a.chain.K + k, coord, normal, a.view, k);
}

template <bool SIMPLEX>
__global__ __launch_bounds__(64) void k_seed_random(DParams prm, SeedRandomArgs a, int ncells, DPatch* __restrict__ stage, int32_t* __restrict__ keep) {
    __shared__ SeedChainLds s;
    const int cell = blockIdx.x;
    if (cell >= ncells) return;
    // the mask gate: the cell centre of sweep_cell
    const DView* vw = prm.views + a.view;
    const int cx = cell % vw->gw, cy = cell / vw->gw;
    if (!seed_foreground(prm, vw, (float)(prm.csize * (2 * cx + 1) - 1) / 2.0f, (float)(prm.csize * (2 * cy + 1) - 1) / 2.0f)) return;
    WaveCtx wc = make_wave_ctx(prm);
    if (wc.lane < a.chain.K) {
        F4 coord, normal;
        seed_random_hypothesis(prm, a, cell, wc.lane, coord, normal);
        seed_park(s, wc.lane, coord, normal, a.view);
    }
    seed_chain<SIMPLEX>(prm, wc, a.chain, s, a.chain.K, (uint32_t)cell, stage + cell, keep + cell);
}

__global__ __launch_bounds__(256) void k_seed_gather(const DPatch* __restrict__ stage, const int32_t* __restrict__ keep, const int32_t* __restrict__ base,
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
    if (a.chain.simplex) hipLaunchKernelGGL(k_seed_random<true>, dim3((unsigned)ncells), dim3(64), lds, st, prm, a, ncells, stage, keep);
    else hipLaunchKernelGGL(k_seed_random<false>, dim3((unsigned)ncells), dim3(64), lds, st, prm, a, ncells, stage, keep);
}
void mvsk_seed_gather(const DPatch* stage, const int32_t* keep, const int32_t* base, int n, DPatch* dst, int32_t id0, hipStream_t st) {
    if (n > 0) hipLaunchKernelGGL(k_seed_gather, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, stage, keep, base, n, dst, id0);
}
