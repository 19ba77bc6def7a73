// mvs_seed_points.hip -- the warm start: seed patches from a sparse point cloud without normals (the points of structure-from-motion),
// scored and refined on the device, appended to the pool in point order (mvs_engine_seed_points in mvs_engine.cpp drives it).  A second
// front end to the chain of the cold start (mvs_seed_random.hip): the job is a point, not a cell; the hypotheses are candidate reference
// views with the normal turned towards that camera, not random planes.  One wave per job, lane v looks at view v.
//   k_seed_points_hyp  the diagnostic window (mvs_engine_seed_points_hypotheses): the hypotheses of a point as records, and their number
//   k_seed_points      builds the hypotheses of the wave's point -- by the SAME device function -- and parks their planes and views in LDS;
//                      the wave then walks them through Optim::preProcess and PatchManager::computeNcc, keeps the best one, refines it (the
//                      engine's refiner) and runs Optim::postProcess; a patch that passes is staged at stage[j], keep[j] = 1 (j = the
//                      point's index in its chunk); k_seed_random_gather then moves the staged records behind the scan of keep
//   k_depth_ranges     per view the number of points that pass its gate and the smallest and largest depth among them
// The stages are called as mvs_engine_probe's ops 1, 0, 2 and 3 call them, and between two stages the candidate goes through a record, as in
// k_seed_random: a kept record has the bits that chain of probes gives.  Optim::check never runs here.
#include <hip/hip_runtime.h>

#include "mvs_device.cuh"
#include "mvs_kernels.h"

using namespace mvsdev;

// The gate of view `vw` for the point `coord` (step 1): its depth d = oaxis . coord > 0, the pixel floorf(ic + 0.5f) of its projection at
// m_level inside the image at that level and, where the view has a mask, on its foreground.  A non-finite coordinate passes nowhere: every
// comparison is written so that a NaN fails it.
DEV bool seed_points_gate(const DParams& prm, const DView* vw, F4 coord, float& d) {
    d = dot4(ld4(vw->oaxis), coord);
    if (!(d > 0.0f)) return false;
    const int W = vw->W[prm.level], H = vw->H[prm.level];
    const F3 ic = project(vw, coord, prm.level);
    const float fx = floorf(ic.x + 0.5f), fy = floorf(ic.y + 0.5f);
    if (!(fx >= 0.0f && fx < (float)W && fy >= 0.0f && fy < (float)H)) return false;
    if (vw->mask && vw->mask[(size_t)(int)fy * W + (int)fx] == 0) return false;
    return true;
}

// Steps 1 and 2 for one point, by a whole wave (all 64 lanes active): lane v gates view v; the first min(K, qualifying) views in ascending
// squared distance |center_v - X|^2, the lower view index first among equals, are picked one at a time (wave_min + ballot, as sort_images
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
        const bool act = (active >> lane) & 1ull;
        const float m = wave_min(act ? dist : __int_as_float(0x7f800000));
        const unsigned long long eq = ballot(act && dist == m);
        const int sel = eq ? __ffsll((long long)eq) - 1 : __ffsll((long long)active) - 1;  // NaN guard: first remaining
        if (lane == k) out = sel;
        active &= ~(1ull << sel);
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

// the record of a hypothesis, written by one lane: m_images = [view], no m_vimages, m_ncc = -1, scales and m_tmp 0, alive, id = k (a copy
// of seed_random_record and of the two helpers below it in mvs_seed_random.hip: that file's machine code stays what it was)
DEV void seed_points_record(DPatch* rec, F4 coord, F4 normal, int view, int k) {
    rec->coord[0] = coord.x; rec->coord[1] = coord.y; rec->coord[2] = coord.z; rec->coord[3] = coord.w;
    rec->normal[0] = normal.x; rec->normal[1] = normal.y; rec->normal[2] = normal.z; rec->normal[3] = normal.w;
    rec->ncc = -1.0f; rec->dscale = 0.0f; rec->ascale = 0.0f; rec->tmp = 0.0f;
    rec->nimages = 1; rec->nvimages = 0; rec->flags = MVS_FLAG_ALIVE; rec->id = k;
    for (int j = 0; j < MVS_MAXI; ++j) { rec->images[j] = 0; rec->vimages[j] = 0; }
    rec->images[0] = (uint8_t)view;
}
// hypothesis k as the wave's candidate: its record, written from the plane parked in LDS (8 floats), read back by load_cand itself
DEV void seed_points_cand(DPatch* rec, const float* plane, int view, int k, const WaveCtx& wc, Cand& c) {
    __syncthreads();
    if (wc.lane == 0) seed_points_record(rec, ld4(plane), ld4(plane + 4), view, k);
    __syncthreads();
    load_cand(rec, wc, c);
}
// a candidate between two stages: through a record, as between two probe calls
DEV void seed_points_roundtrip(DPatch* rec, const WaveCtx& wc, Cand& c) {
    __syncthreads();
    store_cand(rec, wc, c, MVS_FLAG_ALIVE, 0);
    __syncthreads();
    load_cand(rec, wc, c);
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
        seed_points_record(rec, coord, normal, view, lane);
    } else {
        uint4* r4 = reinterpret_cast<uint4*>(rec);
        for (int w = 0; w < (int)MVS_REC_U4; ++w) r4[w] = uint4{0u, 0u, 0u, 0u};
    }
}

template <bool SIMPLEX>
__global__ __launch_bounds__(64) void k_seed_points(DParams prm, SeedPointsArgs a, const float* __restrict__ xyz, DPatch* __restrict__ stage,
                                                    int32_t* __restrict__ keep) {
    __shared__ int s_scratch[192];
    __shared__ float s_hyp[64 * 8];
    __shared__ int s_view[64];
    __shared__ DPatch s_rec, s_win;
    extern __shared__ float s_texs[];
    const int j = blockIdx.x;  // the point's index in the chunk; a.first + j in the call
    if (j >= a.n) return;
    WaveCtx wc = make_wave_ctx(prm);
    int nh;
    {
        const F4 coord{xyz[3 * (size_t)j], xyz[3 * (size_t)j + 1], xyz[3 * (size_t)j + 2], 1.0f};
        int view;
        F4 normal;
        nh = seed_points_hypotheses(prm, a.K, coord, wc.lane, view, normal);
        if (wc.lane < nh) {
            float* h = s_hyp + 8 * wc.lane;
            h[0] = coord.x; h[1] = coord.y; h[2] = coord.z; h[3] = coord.w;
            h[4] = normal.x; h[5] = normal.y; h[6] = normal.z; h[7] = normal.w;
            s_view[wc.lane] = view;
        }
    }
    if (nh == 0) return;
    __syncthreads();
    // the winner: the highest score strictly above min_ncc, the lowest k among equals (a NaN never wins)
    float best = a.min_ncc;
    bool have = false;
    for (int k = 0; k < nh; ++k) {
        Cand c;
        seed_points_cand(&s_rec, s_hyp + 8 * k, s_view[k], k, wc, c);
        if (pre_process(prm, wc, s_scratch, c) != 0) continue;
        seed_points_roundtrip(&s_rec, wc, c);
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
    else refine_patch(prm, wc, c, 0u, 0u, (uint32_t)(a.first + j), 0u);                  // MVS_PROBE_REFINE's key for batch index i
    seed_points_roundtrip(&s_rec, wc, c);
    if (post_process(prm, wc, s_scratch, s_texs, prm.wsz, c) != 0) return;
    store_cand(stage + j, wc, c, MVS_FLAG_ALIVE, 0);
    if (wc.lane == 0) keep[j] = 1;
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
    if (a.simplex) hipLaunchKernelGGL(k_seed_points<true>, dim3((unsigned)a.n), dim3(64), lds, st, prm, a, xyz, stage, keep);
    else hipLaunchKernelGGL(k_seed_points<false>, dim3((unsigned)a.n), dim3(64), lds, st, prm, a, xyz, stage, keep);
}
void mvsk_depth_ranges(const DParams& prm, int64_t n, const float* xyz, uint32_t* lo, uint32_t* hi, unsigned long long* cnt, hipStream_t st) {
    if (n > 0) hipLaunchKernelGGL(k_depth_ranges, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, prm, n, xyz, lo, hi, cnt);
}
