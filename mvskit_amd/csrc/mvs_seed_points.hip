// mvs_seed_points.hip -- the warm start: seed patches from a sparse point cloud without normals (the points of structure-from-motion),
// scored and refined on the device, appended to the pool in point order (mvs_engine_seed_points in mvs_engine.cpp drives it).  The second
// front end to the chain of mvs_seed_chain.cuh, beside the cold start (mvs_seed_random.hip): the job is a point, not a cell; the
// hypotheses are candidate reference views with the normal turned towards that camera, not random planes.  One wave per job, lane v looks
// at view v.
//   k_seed_points_hyp  the diagnostic window (mvs_engine_seed_points_hypotheses): the hypotheses of a point as records, and their number
//   k_seed_points      builds the hypotheses of the wave's point -- by the SAME device function -- and parks them in LDS; seed_chain scores
//                      them, refines the best one and stages a patch that passes at stage[j], keep[j] = 1 (j = the point's index in its
//                      chunk); mvsk_seed_gather then moves the staged records behind the scan of keep
//   k_depth_ranges     per view the number of points that pass its gate and the smallest and largest depth among them
#include <hip/hip_runtime.h>

#include "mvs_kernels.h"
#include "mvs_seed_chain.cuh"

using namespace mvsdev;

// The gate of view `vw` for the point `coord` (step 1): its depth d = oaxis . coord > 0 and its projection at m_level on the foreground
// (seed_foreground).  A non-finite coordinate passes nowhere: every comparison is written so that a NaN fails it.
DEV bool seed_points_gate(const DParams& prm, const DView* vw, F4 coord, float& d) {
    d = dot4(ld4(vw->oaxis), coord);
    if (!(d > 0.0f)) return false;
    const F3 ic = project(vw, coord, prm.level);
    return seed_foreground(prm, vw, ic.x, ic.y);
}

// Steps 1 and 2 for one point, by a whole wave (all 64 lanes active): lane v gates view v; the first min(K, qualifying) views in ascending
// squared distance |center_v - X|^2, the lower view index first among equals, are picked one at a time (wave_pick_min, as sort_images
// picks).  Returns their number n; lane k < n leaves with hypothesis k: its reference view and its normal r = nrm4(center - coord),
// r.w = -coord . r.  The coordinate is the point's, untouched.
DEV int seed_points_hypotheses(const DParams& prm, int K, F4 coord, int lane, int& view, F4& normal) {
    const bool in = lane < prm.nviews;
    const DView* vw = prm.views + (in ? lane : 0);
    float d;
    const bool ok = seed_points_gate(prm, vw, coord, d) && in;
    const F4 ctr = ld4(vw->center);
    const F3 t{ctr.x - coord.x, ctr.y - coord.y, ctr.z - coord.z};
    const float dist = dot3(t, t);
    unsigned long long active = ballot(ok);
    const int n = min(K, __popcll(active));
    int out = 0;
    for (int k = 0; k < n; ++k) {
        const int sel = wave_pick_min(dist, lane, active);
        if (lane == k) out = sel;
    }
    view = out;
    normal = F4{0.0f, 0.0f, 0.0f, 0.0f};
    if (lane < n) {
        F4 r = nrm4(sub4(ld4((prm.views + out)->center), coord));
        r.w = -dot3(F3{coord.x, coord.y, coord.z}, F3{r.x, r.y, r.z});
        normal = r;
    }
    return n;
}

// one wave per point of [0, n): hypothesis k of point i at out[i * K + k] for k < count[i], all-zero bytes in the slots behind
__global__ __launch_bounds__(64) void k_seed_points_hyp(DParams prm, int K, int64_t n, const float* __restrict__ xyz, DPatch* __restrict__ out,
                                                        int32_t* __restrict__ count) {
    const int64_t i = blockIdx.x;
    if (i >= n) return;
    const int lane = lane_id();
    const F4 coord{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], 1.0f};
    int view;
    F4 normal;
    const int nh = seed_points_hypotheses(prm, K, coord, lane, view, normal);
    if (lane == 0) count[i] = nh;
    if (lane >= K) return;
    DPatch* rec = out + i * K + lane;
    if (lane < nh) {
        seed_record(rec, coord, normal, view, lane);
    } else {
        uint4* r4 = reinterpret_cast<uint4*>(rec);
        for (int w = 0; w < (int)MVS_REC_U4; ++w) r4[w] = uint4{0u, 0u, 0u, 0u};
    }
}

template <bool SIMPLEX>
__global__ __launch_bounds__(64) void k_seed_points(DParams prm, SeedPointsArgs a, const float* __restrict__ xyz, DPatch* __restrict__ stage,
                                                    int32_t* __restrict__ keep) {
    __shared__ SeedChainLds s;
    const int j = blockIdx.x;  // the point's index in the chunk; a.first + j in the call
    if (j >= a.n) return;
    WaveCtx wc = make_wave_ctx(prm);
    const F4 coord{xyz[3 * (size_t)j], xyz[3 * (size_t)j + 1], xyz[3 * (size_t)j + 2], 1.0f};
    int view;
    F4 normal;
    const int nh = seed_points_hypotheses(prm, a.chain.K, coord, wc.lane, view, normal);
    if (wc.lane < nh) seed_park(s, wc.lane, coord, normal, view);
    if (nh == 0) return;
    seed_chain<SIMPLEX>(prm, wc, a.chain, s, nh, (uint32_t)(a.first + j), stage + j, keep + j);
}

// One lane per point, every lane of a wave alive to the end (the reductions are wave-wide); per view a wave reduction, then one atomic
// min / max / add per wave that has a qualifying point.  A qualifying depth is a positive float: its bits order as unsigned integers, and
// an integer min / max gives the exact extremes in any order.  lo[v] starts at 0xffffffff, hi[v] and cnt[v] at 0.
__global__ __launch_bounds__(256) void k_depth_ranges(DParams prm, int64_t n, const float* __restrict__ xyz, uint32_t* __restrict__ lo,
                                                      uint32_t* __restrict__ hi, unsigned long long* __restrict__ cnt) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool in = i < n;
    const int64_t s = in ? i : 0;
    const F4 coord{xyz[3 * s], xyz[3 * s + 1], xyz[3 * s + 2], 1.0f};
    const int lane = lane_id();
    const float inf = __int_as_float(0x7f800000);
    for (int v = 0; v < prm.nviews; ++v) {
        float d;
        const bool ok = seed_points_gate(prm, prm.views + v, coord, d) && in;
        const unsigned long long m = ballot(ok);
        if (m == 0) continue;  // wave-uniform
        const float dmin = wave_min(ok ? d : inf), dmax = -wave_min(ok ? -d : inf);
        if (lane == 0) {
            atomicMin(lo + v, (uint32_t)__float_as_int(dmin));
            atomicMax(hi + v, (uint32_t)__float_as_int(dmax));
            atomicAdd(cnt + v, (unsigned long long)__popcll(m));
        }
    }
}

void mvsk_seed_points_hypotheses(const DParams& prm, int K, int64_t n, const float* xyz, DPatch* out, int32_t* count, hipStream_t st) {
    if (n > 0) hipLaunchKernelGGL(k_seed_points_hyp, dim3((unsigned)n), dim3(64), 0, st, prm, K, n, xyz, out, count);
}
// keep[0, a.n) must be zero: a job that gives no patch writes nothing
void mvsk_seed_points(const DParams& prm, const SeedPointsArgs& a, const float* xyz, DPatch* stage, int32_t* keep, hipStream_t st) {
    if (a.n <= 0) return;
    const size_t lds = mvsk_texs_lds_bytes(prm);  // postProcess' kept textures behind the frames, as for k_seed_random
    if (a.chain.simplex) hipLaunchKernelGGL(k_seed_points<true>, dim3((unsigned)a.n), dim3(64), lds, st, prm, a, xyz, stage, keep);
    else hipLaunchKernelGGL(k_seed_points<false>, dim3((unsigned)a.n), dim3(64), lds, st, prm, a, xyz, stage, keep);
}
void mvsk_depth_ranges(const DParams& prm, int64_t n, const float* xyz, uint32_t* lo, uint32_t* hi, unsigned long long* cnt, hipStream_t st) {
    if (n > 0) hipLaunchKernelGGL(k_depth_ranges, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, prm, n, xyz, lo, hi, cnt);
}
