// mvs_image.hip -- image preparation (texels, pyramids, masks), the exclusive scan every compaction of the engine goes through, and the
// two small index utilities (gather / scatter of int32); kernels first, their launchers behind them.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "mvs_common.cuh"
#include "mvs_kernels.h"

using namespace mvsdev;

// =================================================================== K0: images
// interleaved RGB (image/image.hpp:76) -> RGBA8 texels, one 32-bit load per texel
__global__ void k_rgb_to_rgba(const uint8_t* __restrict__ rgb, uint32_t* __restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint8_t* p = rgb + 3 * i;
    out[i] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
}
__global__ void k_rgba_to_rgb(const uint32_t* __restrict__ in, uint8_t* __restrict__ rgb, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t t = in[i];
    rgb[3 * i] = t & 255u; rgb[3 * i + 1] = (t >> 8) & 255u; rgb[3 * i + 2] = (t >> 16) & 255u;
}
// Image::buildImagePyramid, image.cpp:245-315 (filter 0): 4x4 [1 3 3 1]x[1 3 3 1]/64, stride 2, taps outside
// the image dropped without renormalising (D8), round half up.
__global__ void k_pyr_down(const uint32_t* __restrict__ src, int pw, int ph, uint32_t* __restrict__ dst, int w, int h) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= w || y >= h) return;
    const float base[4] = {1.0f, 3.0f, 3.0f, 1.0f};
    float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
    for (int i = -1; i < 3; ++i) {
        const int yt = 2 * y + i;
        if (yt < 0 || ph - 1 < yt) continue;
        for (int j = -1; j < 3; ++j) {
            const int xt = 2 * x + j;
            if (xt < 0 || pw - 1 < xt) continue;
            const float m = (base[i + 1] * base[j + 1]) / 64.0f;
            const uint32_t t = src[(size_t)yt * pw + xt];
            c0 += m * (float)(t & 255u); c1 += m * (float)((t >> 8) & 255u); c2 += m * (float)((t >> 16) & 255u);
        }
    }
    const uint32_t r = (uint8_t)((int)floorf(c0 + 0.5f)), g = (uint8_t)((int)floorf(c1 + 0.5f)), b = (uint8_t)((int)floorf(c2 + 0.5f));
    dst[(size_t)y * w + x] = r | (g << 8) | (b << 16);
}
// Image::buildMaskPyramid, image.cpp:717-747 (indices clamped to the previous level)
__global__ void k_mask_down(const uint8_t* __restrict__ src, int pw, int ph, uint8_t* __restrict__ dst, int w, int h) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= w || y >= h) return;
    const int ys[2] = {2 * y, min(ph - 1, 2 * y + 1)}, xs[2] = {2 * x, min(pw - 1, 2 * x + 1)};
    int inside = 0;
    for (int j = 0; j < 2; ++j) for (int i = 0; i < 2; ++i) inside += src[(size_t)ys[j] * pw + xs[i]] ? 1 : 0;
    dst[(size_t)y * w + x] = inside > 0 ? 255 : 0;
}
__global__ void k_mask_binarise(uint8_t* m, int64_t n) {  // image.cpp:170-177
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) m[i] = m[i] > 127 ? 255 : 0;
}

// =================================================================== scan (exclusive; int32 counts in, int32 or int64 offsets out)
#define SCAN_BLOCK 256
#define SCAN_ITEMS 4
template <typename TI, typename TO>
__global__ void k_scan_block(const TI* __restrict__ in, TO* __restrict__ out, TO* __restrict__ block_sums, int64_t n_in) {
    __shared__ TO s[SCAN_BLOCK];
    const int64_t base = ((int64_t)blockIdx.x * SCAN_BLOCK + threadIdx.x) * SCAN_ITEMS;
    TO v[SCAN_ITEMS], sum = 0;
    for (int k = 0; k < SCAN_ITEMS; ++k) { v[k] = (base + k < n_in) ? (TO)in[base + k] : (TO)0; sum += v[k]; }
    s[threadIdx.x] = sum;
    __syncthreads();
    for (int off = 1; off < SCAN_BLOCK; off <<= 1) {
        TO t = (threadIdx.x >= (unsigned)off) ? s[threadIdx.x - off] : (TO)0;
        __syncthreads();
        s[threadIdx.x] += t;
        __syncthreads();
    }
    TO excl = s[threadIdx.x] - sum;
    for (int k = 0; k < SCAN_ITEMS; ++k) { if (base + k <= n_in) out[base + k] = excl; excl += v[k]; }
    if (threadIdx.x == SCAN_BLOCK - 1) block_sums[blockIdx.x] = s[threadIdx.x];
}
template <typename TO>
__global__ void k_scan_add(TO* __restrict__ out, const TO* __restrict__ block_offsets, int64_t n_out) {
    const int64_t base = ((int64_t)blockIdx.x * SCAN_BLOCK + threadIdx.x) * SCAN_ITEMS;
    const TO o = block_offsets[blockIdx.x];
    for (int k = 0; k < SCAN_ITEMS; ++k) if (base + k < n_out) out[base + k] += o;
}
// out[i] = sum of in[0..i) for i in [0, n]; out[n] is the total (out has n+1 slots, in has n; in-place allowed when the types agree).
// tmp: block sums of every recursion level, at least n/512 + 64 elements of TO.
template <typename TI, typename TO>
void launch_exclusive_scan(const TI* in, TO* out, int64_t n, TO* tmp, hipStream_t st) {
    const int64_t per = (int64_t)SCAN_BLOCK * SCAN_ITEMS;
    const int64_t nb = (n + 1 + per - 1) / per;
    hipLaunchKernelGGL((k_scan_block<TI, TO>), dim3((unsigned)nb), dim3(SCAN_BLOCK), 0, st, in, out, tmp, n);
    if (nb > 1) {
        TO* tmp2 = tmp + nb + 1;
        launch_exclusive_scan<TO, TO>(tmp, tmp, nb, tmp2, st);
        hipLaunchKernelGGL((k_scan_add<TO>), dim3((unsigned)nb), dim3(SCAN_BLOCK), 0, st, out, tmp, n + 1);
    }
}
__global__ void k_gather_i32(const int32_t* __restrict__ src, const int32_t* __restrict__ idx, int32_t* __restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = src[idx[i]];
}
__global__ void k_scatter_i32(int32_t* __restrict__ dst, const int32_t* __restrict__ idx, const int32_t* __restrict__ val, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[idx[i]] = val[i];
}

// =================================================================== host-callable launchers
void mvsk_rgb_to_rgba(const uint8_t* rgb, uint32_t* out, int64_t n, hipStream_t st) { hipLaunchKernelGGL(k_rgb_to_rgba, dim3(nblk(n, 256)), dim3(256), 0, st, rgb, out, n); }
void mvsk_rgba_to_rgb(const uint32_t* in, uint8_t* rgb, int64_t n, hipStream_t st) { hipLaunchKernelGGL(k_rgba_to_rgb, dim3(nblk(n, 256)), dim3(256), 0, st, in, rgb, n); }
void mvsk_pyr_down(const uint32_t* src, int pw, int ph, uint32_t* dst, int w, int h, hipStream_t st) {
    hipLaunchKernelGGL(k_pyr_down, dim3((w + 63) / 64, (h + 3) / 4), dim3(64, 4), 0, st, src, pw, ph, dst, w, h);
}
void mvsk_mask_down(const uint8_t* src, int pw, int ph, uint8_t* dst, int w, int h, hipStream_t st) {
    hipLaunchKernelGGL(k_mask_down, dim3((w + 63) / 64, (h + 3) / 4), dim3(64, 4), 0, st, src, pw, ph, dst, w, h);
}
void mvsk_mask_binarise(uint8_t* m, int64_t n, hipStream_t st) { hipLaunchKernelGGL(k_mask_binarise, dim3(nblk(n, 256)), dim3(256), 0, st, m, n); }
void mvsk_exclusive_scan(const int32_t* in, int32_t* out, int64_t n, int32_t* tmp, hipStream_t st) { launch_exclusive_scan<int32_t, int32_t>(in, out, n, tmp, st); }
// the per-cell counts -> 64-bit list offsets; tmp as above, in elements of csr_off_t
void mvsk_exclusive_scan_off(const int32_t* in, csr_off_t* out, int64_t n, csr_off_t* tmp, hipStream_t st) { launch_exclusive_scan<int32_t, csr_off_t>(in, out, n, tmp, st); }
void mvsk_gather_i32(const int32_t* src, const int32_t* idx, int32_t* out, int64_t n, hipStream_t st) { if (n > 0) hipLaunchKernelGGL(k_gather_i32, dim3(nblk(n, 256)), dim3(256), 0, st, src, idx, out, n); }
void mvsk_scatter_i32(int32_t* dst, const int32_t* idx, const int32_t* val, int64_t n, hipStream_t st) { if (n > 0) hipLaunchKernelGGL(k_scatter_i32, dim3(nblk(n, 256)), dim3(256), 0, st, dst, idx, val, n); }
