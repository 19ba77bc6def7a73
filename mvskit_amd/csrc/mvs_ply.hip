// mvs_ply.hip -- PatchManager::writePly (patch_manager.cpp:542-633) on the device: the vertex colour and the text or binary vertex
// records of the alive pool, one chunk of pool slots at a time (mvs_engine_export_ply in mvs_engine.cpp drives it).
//   k_ply_select   alive slots of the chunk -> their pool indices, in pool order (kill_base = exclusive scan of the alive flags)
//   k_ply_colour   one lane per alive vertex: the colour, and the length of its ASCII line
//   k_ply_emit     one lane per vertex formats its line again into LDS at (offset - block base); the block then copies its contiguous
//                  byte range out with 16-byte stores (bytes only at the two ends, where the range shares a 16-byte word with a
//                  neighbouring block)
#include <hip/hip_runtime.h>

#include "mvs_kernels.h"
#include "mvs_plyfmt.h"

#define PLY_BLOCK 256

__global__ void k_ply_select(const DPatch* __restrict__ pool, const int32_t* __restrict__ base, int64_t i0, int64_t i1, int32_t* __restrict__ idx) {
    const int64_t i = i0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= i1 || !(pool[i].flags & 1)) return;
    idx[base[i] - base[i0]] = (int32_t)i;
}

// PhotoSet::getColor summed over m_images and divided by their count (patch_manager.cpp:565-583), as the host mirror computed it:
// P of level `level` (rows 0-1 halved per level: DView::P), IEEE division, a view that the point lies behind or projects outside
// [0, W-1) x [0, H-1) of adds nothing but counts; the bilinear sample of the RGBA8 pyramid in the mirror's order of operations.
// -ffp-contract=off keeps every operation as written.  Returns r | g << 8 | b << 16.
__device__ uint32_t ply_colour(const DPatch* __restrict__ rec, const DView* __restrict__ views, int nviews, int level) {
    const float X0 = rec->coord[0], X1 = rec->coord[1], X2 = rec->coord[2], X3 = rec->coord[3];
    float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
    int denom = 0;
    const int nim = rec->nimages;
    for (int k = 0; k < nim; ++k) {
        const int image = rec->images[k];
        if (image >= nviews) continue;
        denom++;
        const DView* vw = views + image;
        const float* q = vw->P[level];
        const float z = q[8] * X0 + q[9] * X1 + q[10] * X2 + q[11] * X3;
        if (z <= 0.0f) continue;
        const float x = (q[0] * X0 + q[1] * X1 + q[2] * X2 + q[3] * X3) / z;
        const float y = (q[4] * X0 + q[5] * X1 + q[6] * X2 + q[7] * X3) / z;
        const int W = vw->W[level], H = vw->H[level];
        if (!(x >= 0.0f && y >= 0.0f && x < (float)(W - 1) && y < (float)(H - 1))) continue;
        const int lx = (int)x, ly = (int)y;
        const float dx1 = x - lx, dx0 = 1.0f - dx1, dy1 = y - ly, dy0 = 1.0f - dy1;
        const float f00 = dx0 * dy0, f01 = dx0 * dy1, f10 = dx1 * dy0, f11 = dx1 * dy1;
        const uint32_t* r0 = vw->img[level] + ((size_t)ly * W + lx);
        const uint32_t* r1 = r0 + W;
        const uint32_t a = r0[0], b = r0[1], c = r1[0], d = r1[1];  // (lx, ly), (lx+1, ly), (lx, ly+1), (lx+1, ly+1)
#define PLY_CH(v, s) ((int)(((v) >> (s)) & 0xffu))
        c0 += (PLY_CH(a, 0) * f00 + PLY_CH(c, 0) * f01) + (PLY_CH(b, 0) * f10 + PLY_CH(d, 0) * f11);
        c1 += (PLY_CH(a, 8) * f00 + PLY_CH(c, 8) * f01) + (PLY_CH(b, 8) * f10 + PLY_CH(d, 8) * f11);
        c2 += (PLY_CH(a, 16) * f00 + PLY_CH(c, 16) * f01) + (PLY_CH(b, 16) * f10 + PLY_CH(d, 16) * f11);
#undef PLY_CH
    }
    if (denom == 0) return 128u | 128u << 8 | 128u << 16;
    const float fd = (float)denom;
    const uint32_t r = (uint32_t)min(255, (int)floorf(c0 / fd + 0.5f));
    const uint32_t g = (uint32_t)min(255, (int)floorf(c1 / fd + 0.5f));
    const uint32_t b = (uint32_t)min(255, (int)floorf(c2 / fd + 0.5f));
    return r | g << 8 | b << 16;
}

__global__ __launch_bounds__(PLY_BLOCK) void k_ply_colour(const DPatch* __restrict__ pool, const int32_t* __restrict__ idx, int64_t n,
                                                         const DView* __restrict__ views, int nviews, int level, int ascii,
                                                         uint32_t* __restrict__ rgb, int32_t* __restrict__ len) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const DPatch* rec = pool + idx[k];
    const uint32_t c = ply_colour(rec, views, nviews, level);
    rgb[k] = c;
    if (ascii)
        len[k] = mvsply::format_line(rec->coord[0], rec->coord[1], rec->coord[2], rec->normal[0], rec->normal[1], rec->normal[2], c & 0xffu,
                                     (c >> 8) & 0xffu, (c >> 16) & 0xffu, nullptr);
}

// off: ASCII, the exclusive scan of the line lengths (n + 1 entries); binary: null, vertex k at 27 k.  out: the chunk's bytes.
__global__ __launch_bounds__(PLY_BLOCK) void k_ply_emit(const DPatch* __restrict__ pool, const int32_t* __restrict__ idx, int64_t n,
                                                       const uint32_t* __restrict__ rgb, const int64_t* __restrict__ off, uint8_t* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) char line[PLY_BLOCK * MVS_PLY_LINE_MAX + 16];
    const int64_t k0 = (int64_t)blockIdx.x * PLY_BLOCK;
    const int64_t k1 = min(n, k0 + PLY_BLOCK);
    const int64_t k = k0 + threadIdx.x;
    const int64_t lo = off ? off[k0] : 27 * k0, hi = off ? off[k1] : 27 * k1;
    const int64_t a0 = lo & ~(int64_t)15;  // LDS byte j holds out[a0 + j]: 16-byte words of out are 16-byte words of LDS
    if (k < n) {
        const DPatch* rec = pool + idx[k];
        const uint32_t c = rgb[k];
        char* p = line + ((off ? off[k] : 27 * k) - a0);
        if (off) {
            mvsply::format_line(rec->coord[0], rec->coord[1], rec->coord[2], rec->normal[0], rec->normal[1], rec->normal[2], c & 0xffu,
                                (c >> 8) & 0xffu, (c >> 16) & 0xffu, p);
        } else {  // binary_little_endian: 6 x float32, 3 x uint8
            const float v[6] = {rec->coord[0], rec->coord[1], rec->coord[2], rec->normal[0], rec->normal[1], rec->normal[2]};
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                const uint32_t u = __float_as_uint(v[j]);
#pragma unroll
                for (int t = 0; t < 4; ++t) p[4 * j + t] = (char)((u >> (8 * t)) & 0xffu);
            }
            p[24] = (char)(c & 0xffu); p[25] = (char)((c >> 8) & 0xffu); p[26] = (char)((c >> 16) & 0xffu);
        }
    }
    __syncthreads();
    // the 16-byte words [a0, a1) that hold [lo, hi): whole words with one vector store each, the partial first / last word byte by byte
    const int64_t a1 = (hi + 15) & ~(int64_t)15;
    const int64_t nw = (a1 - a0) >> 4;
    for (int64_t w = threadIdx.x; w < nw; w += PLY_BLOCK) {
        const int64_t g = a0 + 16 * w;
        if (g >= lo && g + 16 <= hi) {
            *reinterpret_cast<uint4*>(out + g) = *reinterpret_cast<const uint4*>(line + 16 * w);
        } else {
            for (int t = 0; t < 16; ++t)
                if (g + t >= lo && g + t < hi) out[g + t] = (uint8_t)line[16 * w + t];
        }
    }
}

static inline unsigned ply_blocks(int64_t n) { return (unsigned)((n + PLY_BLOCK - 1) / PLY_BLOCK); }

void mvsk_ply_select(const DPatch* pool, const int32_t* base, int64_t i0, int64_t i1, int32_t* idx, hipStream_t st) {
    if (i1 > i0) hipLaunchKernelGGL(k_ply_select, dim3(ply_blocks(i1 - i0)), dim3(PLY_BLOCK), 0, st, pool, base, i0, i1, idx);
}
void mvsk_ply_colour(const DPatch* pool, const int32_t* idx, int64_t n, const DView* views, int nviews, int level, int ascii, uint32_t* rgb, int32_t* len,
                     hipStream_t st) {
    if (n > 0) hipLaunchKernelGGL(k_ply_colour, dim3(ply_blocks(n)), dim3(PLY_BLOCK), 0, st, pool, idx, n, views, nviews, level, ascii, rgb, len);
}
void mvsk_ply_emit(const DPatch* pool, const int32_t* idx, int64_t n, const uint32_t* rgb, const int64_t* off, uint8_t* out, hipStream_t st) {
    if (n > 0) hipLaunchKernelGGL(k_ply_emit, dim3(ply_blocks(n)), dim3(PLY_BLOCK), 0, st, pool, idx, n, rgb, off, out);
}
