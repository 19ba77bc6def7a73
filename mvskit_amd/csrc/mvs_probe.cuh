// mvs_probe.cuh (part of the unit mvs_patch.hip) -- the probes: single functions of the patch arithmetic on a batch of records, one wave per record (mvs_engine_probe).
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include "mvs_patch_common.cuh"
#include "mvs_check.cuh"
#include "mvs_kernels.h"

using namespace mvsdev;

// =================================================================== probes (single functions, batched)
__global__ __launch_bounds__(64) void k_probe(DParams prm, int op, int64_t n, const DPatch* __restrict__ in, const float* __restrict__ in_f,
                                              DPatch* __restrict__ out, float* __restrict__ out_f, int32_t* __restrict__ out_i) {
    __shared__ int s_scratch[192];
    extern __shared__ float s_texs[];
    const int64_t i = blockIdx.x;
    if (i >= n) return;
    WaveCtx wc = make_wave_ctx(prm);
    const int tstride = prm.wsz;  // odd for 7x7 / 5x5 windows: the lane-per-pair reads of setRefImage fall in distinct banks
    if (op == 5) {  // MVS_PROBE_MATH
        if (wc.lane == 0) {
            const float x = in_f[i];
            out_f[5 * i] = pm_sinf(x); out_f[5 * i + 1] = pm_cosf(x); out_f[5 * i + 2] = pm_asinf(x); out_f[5 * i + 3] = pm_acosf(x);
            out_f[5 * i + 4] = pm_atanf(x);
        }
        return;
    }
    Cand c;
    load_cand(in + i, wc, c);
    if (op == 0) {  // MVS_PROBE_NCC
        const float ncc = compute_ncc(prm, wc, c.coord, c.normal, c.img, c.nimg);
        if (wc.lane == 0) out_f[i] = ncc;
    } else if (op == 1) {
        const int f = pre_process(prm, wc, s_scratch, c);
        store_cand(out + i, wc, c, 1, (int)i);
        if (wc.lane == 0) out_i[i] = f;
    } else if (op == 2) {
        refine_patch(prm, wc, c, 0u, 0u, (uint32_t)i, 0u);
        store_cand(out + i, wc, c, 1, (int)i);
    } else if (op == 3) {
        int f = post_process(prm, wc, s_scratch, s_texs, tstride, c);
        if (f == 0 && prm.depth >= 2 && prm.enable_check) {
            const CheckCtx cx{in, -1, -1, 0, s_scratch, nullptr};  // no staged ids in a probe (a null pointer here crashes clang 22)
            const int chk = check_patch(prm, wc, cx, c, s_texs, out_i + n);  // out_i[n]: overflow flag word
            if (chk < 0) { if (wc.lane == 0) atomicOr(out_i + n, 4); }       // no second tier in a probe
            else if (chk) f = -1;
        }
        store_cand(out + i, wc, c, 1, (int)i);
        if (wc.lane == 0) out_i[i] = f;
    } else if (op == 4) {
        RefineCtx rc;
        rc.center = c.coord; rc.ref = rli(c.img, 0);
        rc.ray = nrm4(sub4(c.coord, ld4((prm.views + rc.ref)->center)));
        rc.dscale = c.dscale; rc.ascale = prm.ascaleConst;
        float x[3];
        encode(prm, rc, c.coord, c.normal, x);
        double fv[4];
        cost_func4(prm, wc, rc, __shfl(c.img, wc.lane & 15), c.nimg, false, x[0], x[1], x[2], fv);
        if (wc.lane == 0) out_f[i] = (float)fv[0];
    }
}

// refinePatch alone (occupancy experiment / kernel benchmark): same arithmetic as probe op 2
__global__ __launch_bounds__(64, MVS_SWEEP_WAVES) void k_probe_refine(DParams prm, int64_t n, const DPatch* __restrict__ in, DPatch* __restrict__ out) {
    const int64_t i = blockIdx.x;
    if (i >= n) return;
    WaveCtx wc = make_wave_ctx(prm);
    Cand c;
    load_cand(in + i, wc, c);
    refine_patch(prm, wc, c, 0u, 0u, (uint32_t)i, 0u);
    store_cand(out + i, wc, c, 1, (int)i);
}
// ... with the narrow samplers (WaveCtxT<false, true>), chosen by mvsk_probe as mvsk_sweep chooses k_sweep_full_ofs
__global__ __launch_bounds__(64, MVS_SWEEP_WAVES) void k_probe_refine_ofs(DParams prm, int64_t n, const DPatch* __restrict__ in, DPatch* __restrict__ out) {
    const int64_t i = blockIdx.x;
    if (i >= n) return;
    WaveCtxT<false, true> wc;
    static_cast<WaveCtx&>(wc) = make_wave_ctx(prm);
    Cand c;
    load_cand(in + i, wc, c);
    refine_patch(prm, wc, c, 0u, 0u, (uint32_t)i, 0u);
    store_cand(out + i, wc, c, 1, (int)i);
}
// refinePatch with the CONVERGED refiner (probe ops 2 and 6): out_f[4 i ..] = the best vertex and its cost, out_i[i] = evaluations
// (negative: the budget ran out and the record is the input)
__global__ __launch_bounds__(64, MVS_SWEEP_WAVES) void k_probe_refine_simplex(DParams prm, int64_t n, const DPatch* __restrict__ in, DPatch* __restrict__ out,
                                                                              float* __restrict__ out_f, int32_t* __restrict__ out_i, int max_evals, float xtol) {
    const int64_t i = blockIdx.x;
    if (i >= n) return;
    WaveCtx wc = make_wave_ctx(prm);
    Cand c;
    load_cand(in + i, wc, c);
    float x[3];
    double f;
    const int r = refine_patch_simplex(prm, wc, c, max_evals, xtol, nullptr, x, &f);
    store_cand(out + i, wc, c, 1, (int)i);
    if (wc.lane == 0) {
        out_f[4 * i] = x[0]; out_f[4 * i + 1] = x[1]; out_f[4 * i + 2] = x[2]; out_f[4 * i + 3] = (float)f;
        out_i[i] = r;
    }
}

// =================================================================== host-callable launchers
KernelVariant mvsk_probe(const DParams& prm, int op, int64_t n, const DPatch* in, const float* in_f, DPatch* out, float* out_f, int32_t* out_i, const RefineSel& rs,
                         hipStream_t st) {
    KernelVariant v = mvsk_kernel_variant(prm);
    v.full_window = false;  // the refine probes have no full-window instantiation
    if (n <= 0) return v;
    if ((op == 2 || op == 6) && rs.simplex)
        hipLaunchKernelGGL(k_probe_refine_simplex, dim3((unsigned)n), dim3(64), MVS_FRAME_LDS_BYTES, st, prm, n, in, out, out_f, out_i, rs.max_evals, rs.xtol);
    else if (op == 2) {
        if (v.narrow) hipLaunchKernelGGL(k_probe_refine_ofs, dim3((unsigned)n), dim3(64), MVS_FRAME_LDS_BYTES, st, prm, n, in, out);
        else hipLaunchKernelGGL(k_probe_refine, dim3((unsigned)n), dim3(64), MVS_FRAME_LDS_BYTES, st, prm, n, in, out);
        v.launched = true;
    } else hipLaunchKernelGGL(k_probe, dim3((unsigned)n), dim3(64), mvsk_sweep_lds_bytes(prm), st, prm, op, n, in, in_f, out, out_f, out_i);
    return v;
}
