// mvs_mesh_texture.hip -- a textured mesh: the view that textures each triangle, and the atlas with its texture coordinates
// (mvs_engine_mesh_face_views and mvs_engine_mesh_texture in mvs_engine_mesh.cpp drive it; the contract is in include/mvskit_texture.h).
// The views stream one at a time through the render's per-vertex buffers (mvsk_mrender_project, mvs_mesh_render.hip).
//   k_mtex_check_labels a lane per triangle: a label outside -1 .. nviews - 1 sets *bad
//   k_mtex_best         a lane per triangle, once per view: the candidate gates (a) to (d) and the running best |area| with its view in
//                       the triangle's own slots -- the views come in ascending order and the comparison is strict: the lowest view
//                       among equals.  No atomic: a lane owns its triangle
//   k_mtex_count        a lane per triangle: n_faces[v], a ballot per view and one add per wave and view
//   k_mtex_take         a lane per triangle, once per view: for the triangles labelled with this view the nine numbers (sx, sy, d) x 3
//                       and the honoured flag, so that the texel kernel never touches a vertex
//   k_mtex_list         a lane per triangle: behind the scan of the flags, the honoured triangle k's row at list[k]
//   k_mtex_uv           a lane per triangle: the three corner texels
//   k_mtex_texels       a lane per four consecutive texels of the atlas in row order (twelve contiguous bytes, three dword stores): the
//                       cell and the half from the texel's position, the triangle from list, the perspective-correct position in the
//                       labelled view as the contract's fp64 chain, a bilinear lookup in the RGBA8 level.  A lane keeps the triangle's
//                       nine numbers as doubles while its texels stay in one triangle.  It reads no patch record
// and, for the seam calls of include/mvskit_seams.h (the drivers are next to the texture drivers; adjacency and smoothing are in
// mvs_mesh_seams.hip):
//   k_mtex_quality          a lane per triangle, once per view, behind k_mtex_best over all views: the same gates, one byte
//   k_mtex_texels_levelled  k_mtex_texels with the view's offset added to c before the rounding and the clamp to a byte
//   k_mtex_seam_samples     a lane per edge slot: a seam edge's samples in both views, summed per pair of views in the wave and in LDS,
//                           one 64-bit integer add per block, pair and component
// Every loop is bounded by its own count; no kernel waits for another workgroup, and none loads what another workgroup writes in the same
// launch.  Stores are plain vector stores.
#include <hip/hip_runtime.h>

#include "mvs_mesh_common.cuh"
#include "mvs_kernels.h"

using namespace mvsdev;

__global__ __launch_bounds__(MESH_BLOCK) void k_mtex_check_labels(int64_t n_t, const int32_t* __restrict__ label, int nviews, uint32_t* __restrict__ bad) {
    const int64_t t = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    const bool out = t < n_t && (label[t] < -1 || label[t] >= nviews);
    if (ballot(out) != 0ull && lane_id() == 0) atomicOr(bad, 1u);
}

// the signed area of triangle t in the view whose vertices are in scr / ok; false where a vertex is not usable
DEV bool mtex_area(int64_t t, const int32_t* __restrict__ tris, const int32_t* __restrict__ scr, const uint32_t* __restrict__ ok, int64_t id[3], long long& area) {
    id[0] = tris[3 * t]; id[1] = tris[3 * t + 1]; id[2] = tris[3 * t + 2];
    if (!(ok[id[0]] && ok[id[1]] && ok[id[2]])) return false;
    const long long X0 = scr[2 * id[0]], Y0 = scr[2 * id[0] + 1], X1 = scr[2 * id[1]], Y1 = scr[2 * id[1] + 1], X2 = scr[2 * id[2]], Y2 = scr[2 * id[2] + 1];
    area = (X1 - X0) * (Y2 - Y0) - (Y1 - Y0) * (X2 - X0);
    return true;
}

// want: the sign a candidate's area must have (front_only), 0 for either; visible may be null; best_area 0 and best_label -1 before the
// first view
__global__ __launch_bounds__(MESH_BLOCK) void k_mtex_best(int view, int want, int64_t n_t, const int32_t* __restrict__ tris, const int32_t* __restrict__ scr,
                                                           const uint32_t* __restrict__ ok, const u64* __restrict__ visible, int W, int H,
                                                           long long* __restrict__ best_area, int32_t* __restrict__ best_label) {
    const int64_t t = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (t >= n_t) return;
    int64_t id[3];
    long long area;
    if (!mtex_area(t, tris, scr, ok, id, area) || area == 0) return;
    if (want != 0 && (area > 0) != (want > 0)) return;
    const long long xmax = 256ll * (W - 1) - 1, ymax = 256ll * (H - 1) - 1;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const long long sx = scr[2 * id[k]], sy = scr[2 * id[k] + 1];
        if (sx < 0 || sx > xmax || sy < 0 || sy > ymax) return;
        if (visible && !((visible[id[k]] >> view) & 1ull)) return;
    }
    const long long a = area < 0 ? -area : area;
    if (a > best_area[t]) { best_area[t] = a; best_label[t] = view; }
}

// counts[v] += the triangles labelled v (zero before the launch)
__global__ __launch_bounds__(MESH_BLOCK) void k_mtex_count(int64_t n_t, const int32_t* __restrict__ label, int nviews, u64* __restrict__ counts) {
    const int64_t t = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    const int32_t l = t < n_t ? label[t] : -1;
    const int lane = lane_id();
    for (int v = 0; v < nviews; ++v) {
        const u64 m = ballot(l == v);
        if (m != 0ull && lane == 0) atomicAdd(counts + v, (u64)__popcll(m));
    }
}

// win[9 t ..] = (sx, sy, bits(d)) of the three vertices, flag[t] = 1 where triangle t is labelled `view` and the label is honoured
// (flag zero before the first view)
__global__ __launch_bounds__(MESH_BLOCK) void k_mtex_take(int view, int64_t n_t, const int32_t* __restrict__ tris, const int32_t* __restrict__ label,
                                                           const int32_t* __restrict__ scr, const float* __restrict__ vd, const uint32_t* __restrict__ ok,
                                                           int32_t* __restrict__ win, int32_t* __restrict__ flag) {
    const int64_t t = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (t >= n_t || label[t] != view) return;
    int64_t id[3];
    long long area;
    if (!mtex_area(t, tris, scr, ok, id, area) || area == 0) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        win[9 * t + 3 * k] = scr[2 * id[k]];
        win[9 * t + 3 * k + 1] = scr[2 * id[k] + 1];
        win[9 * t + 3 * k + 2] = __float_as_int(vd[id[k]]);
    }
    flag[t] = 1;
}

__global__ __launch_bounds__(MESH_BLOCK) void k_mtex_list(int64_t n_t, const int32_t* __restrict__ flag, const int32_t* __restrict__ base, int32_t* __restrict__ list,
                                                           int64_t cap) {
    const int64_t t = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (t >= n_t || !flag[t]) return;
    const int64_t k = base[t];
    if (k < cap) list[k] = (int32_t)t;
}

// uv[6 t ..] = the (column, row) of the three corner texels; an untextured triangle gets the centre texel of cell 0
__global__ __launch_bounds__(MESH_BLOCK) void k_mtex_uv(int64_t n_t, const int32_t* __restrict__ flag, const int32_t* __restrict__ base, int res, int cpr,
                                                         int32_t* __restrict__ uv) {
    const int64_t t = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (t >= n_t) return;
    const int B = res + 3;
    int c[6] = {B / 2, B / 2, B / 2, B / 2, B / 2, B / 2};
    if (flag[t]) {
        const int64_t k = base[t], q = 1 + (k >> 1);
        const int ox = (int)(q % cpr) * B, oy = (int)(q / cpr) * B;
        if (k & 1) { c[0] = ox + res + 2; c[1] = oy + res + 2; c[2] = ox + 2; c[3] = oy + res + 2; c[4] = ox + res + 2; c[5] = oy + 2; }
        else { c[0] = ox; c[1] = oy; c[2] = ox + res; c[3] = oy; c[4] = ox; c[5] = oy + res; }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) uv[6 * t + k] = c[k];
}

// the triangle under a lane's texel: its depths and screen positions, loaded when the lane's texels change triangle
struct MtexTri {
    int32_t k;  // the honoured triangle's number, -1: none loaded
    double d[3], sx[3], sy[3];
    const uint32_t* img;
    int W, H;
};

DEV void mtex_load(MtexTri& s, int32_t k, const int32_t* __restrict__ list, const int32_t* __restrict__ label, const int32_t* __restrict__ win,
                   const DView* __restrict__ views, int level) {
    const int64_t t = list[k];
    const DView& vw = views[label[t]];
    s.k = k;
    s.img = vw.img[level]; s.W = vw.W[level]; s.H = vw.H[level];
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        s.sx[m] = (double)win[9 * t + 3 * m];
        s.sy[m] = (double)win[9 * t + 3 * m + 1];
        s.d[m] = (double)__int_as_float(win[9 * t + 3 * m + 2]);
    }
}

// the three bytes of one texel of triangle s with the integer weights n1, n2 (n0 = res - n1 - n2), as the low 24 bits; grey where the
// position has no sense
DEV uint32_t mtex_texel(const MtexTri& s, int res, int n1, int n2) {
    const uint32_t grey = 0x808080u;
    if (s.W < 2 || s.H < 2) return grey;
    const double a0 = (double)(res - n1 - n2) * s.d[0], a1 = (double)n1 * s.d[1], a2 = (double)n2 * s.d[2];
    const double den = a0 + a1 + a2;
    if (!(den > 0.0) || !(den < __longlong_as_double(0x7ff0000000000000ll))) return grey;
    const double xs = (a0 * s.sx[0] + a1 * s.sx[1] + a2 * s.sx[2]) / den, ys = (a0 * s.sy[0] + a1 * s.sy[1] + a2 * s.sy[2]) / den;
    double x = xs / 256.0, y = ys / 256.0;
    if (x != x || y != y) return grey;
    x = fmin(fmax(x, 0.0), (double)(s.W - 1) - 1.0 / 256);
    y = fmin(fmax(y, 0.0), (double)(s.H - 1) - 1.0 / 256);
    const double fix = floor(x), fiy = floor(y);
    const double fx = x - fix, fy = y - fiy;
    const int ix = (int)fix, iy = (int)fiy;  // 0 .. W - 2, 0 .. H - 2
    const uint32_t* p = s.img + (int64_t)iy * s.W + ix;
    const uint32_t t00 = p[0], t10 = p[1], t01 = p[s.W], t11 = p[s.W + 1];
    uint32_t out = 0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const double c00 = (double)((t00 >> (8 * ch)) & 255u), c10 = (double)((t10 >> (8 * ch)) & 255u);
        const double c01 = (double)((t01 >> (8 * ch)) & 255u), c11 = (double)((t11 >> (8 * ch)) & 255u);
        const double top = (1.0 - fx) * c00 + fx * c10, bot = (1.0 - fx) * c01 + fx * c11;
        const double c = (1.0 - fy) * top + fy * bot;
        out |= ((uint32_t)(int)floor(c + 0.5) & 255u) << (8 * ch);
    }
    return out;
}

// rgb: 3 total bytes rounded up to whole groups of twelve; ngroups = ceil(total / 4) lanes.  total <= 2^30
__global__ __launch_bounds__(MESH_BLOCK) void k_mtex_texels(const DView* __restrict__ views, int level, int res, int width, int cpr, int64_t total, int64_t n_cells,
                                                             int64_t n_textured, const int32_t* __restrict__ list, const int32_t* __restrict__ label,
                                                             const int32_t* __restrict__ win, uint32_t* __restrict__ rgb, int64_t ngroups) {
    const int64_t g = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (g >= ngroups) return;
    const int B = res + 3;
    const uint32_t p0 = (uint32_t)(4 * g);
    uint32_t row = p0 / (uint32_t)width, col = p0 % (uint32_t)width;
    uint32_t cy = row / (uint32_t)B, j = row % (uint32_t)B, cx = col / (uint32_t)B, i = col % (uint32_t)B;
    MtexTri s;
    s.k = -1;
    uint32_t px[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        uint32_t c = 0x808080u;
        const int64_t q = (int64_t)cy * cpr + cx;
        if ((int64_t)p0 + e < total && (int)cx < cpr && q >= 1 && q < n_cells) {
            const bool upper = (int)(i + j) >= res + 3;
            const int64_t k = 2 * (q - 1) + (upper ? 1 : 0);
            if (k < n_textured) {
                if (s.k != (int32_t)k) mtex_load(s, (int32_t)k, list, label, win, views, level);
                c = mtex_texel(s, res, upper ? res + 2 - (int)i : (int)i, upper ? res + 2 - (int)j : (int)j);
            }
        }
        px[e] = c;
        // the next texel of the atlas in row order
        if (++col == (uint32_t)width) {
            col = 0; cx = 0; i = 0;
            if (++j == (uint32_t)B) { j = 0; ++cy; }
        } else if (++i == (uint32_t)B) { i = 0; ++cx; }
    }
    // four texels of three bytes as three words, in memory order
    uint32_t* out = rgb + 3 * g;
    out[0] = px[0] | px[1] << 24;
    out[1] = px[1] >> 8 | px[2] << 16;
    out[2] = px[2] >> 16 | px[3] << 8;
}

// ---- the seam calls of include/mvskit_seams.h that need the candidate gates, MtexTri or a view's texels

// gates (a) to (d) of k_mtex_best for triangle t in one view: true for a candidate, with its |area|
DEV bool mtex_candidate(int view, int want, int64_t t, const int32_t* __restrict__ tris, const int32_t* __restrict__ scr, const uint32_t* __restrict__ ok,
                        const u64* __restrict__ visible, int W, int H, long long& a) {
    int64_t id[3];
    long long area;
    if (!mtex_area(t, tris, scr, ok, id, area) || area == 0) return false;
    if (want != 0 && (area > 0) != (want > 0)) return false;
    const long long xmax = 256ll * (W - 1) - 1, ymax = 256ll * (H - 1) - 1;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const long long sx = scr[2 * id[k]], sy = scr[2 * id[k] + 1];
        if (sx < 0 || sx > xmax || sy < 0 || sy > ymax) return false;
        if (visible && !((visible[id[k]] >> view) & 1ull)) return false;
    }
    a = area < 0 ? -area : area;
    return true;
}

// quality[t][view] = max(1, 255 |area| / best_area[t]) for a candidate (quality zero before the first view; best_area from k_mtex_best
// over all views with the same gates, so a candidate's is >= its |area| > 0)
__global__ __launch_bounds__(MESH_BLOCK) void k_mtex_quality(int view, int want, int64_t n_t, const int32_t* __restrict__ tris, const int32_t* __restrict__ scr,
                                                              const uint32_t* __restrict__ ok, const u64* __restrict__ visible, int W, int H,
                                                              const long long* __restrict__ best_area, int nviews, uint8_t* __restrict__ quality) {
    const int64_t t = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (t >= n_t) return;
    long long a;
    if (!mtex_candidate(view, want, t, tris, scr, ok, visible, W, H, a)) return;
    const long long best = best_area[t];
    if (best <= 0) return;
    const long long q = 255ll * a / best;
    quality[t * nviews + view] = (uint8_t)(q < 1 ? 1 : q);
}

// TEXEL's c of the three channels before rounding, at the homogeneous position (nx, ny, den) in 1/256 pixel of the W x H image; false
// where TEXEL leaves the texel grey.  The lines of mtex_texel
DEV bool mtex_colour(const uint32_t* __restrict__ img, int W, int H, double nx, double ny, double den, double c[3]) {
    if (W < 2 || H < 2) return false;
    if (!(den > 0.0) || !(den < __longlong_as_double(0x7ff0000000000000ll))) return false;
    const double xs = nx / den, ys = ny / den;
    double x = xs / 256.0, y = ys / 256.0;
    if (x != x || y != y) return false;
    x = fmin(fmax(x, 0.0), (double)(W - 1) - 1.0 / 256);
    y = fmin(fmax(y, 0.0), (double)(H - 1) - 1.0 / 256);
    const double fix = floor(x), fiy = floor(y);
    const double fx = x - fix, fy = y - fiy;
    const int ix = (int)fix, iy = (int)fiy;  // 0 .. W - 2, 0 .. H - 2
    const uint32_t* p = img + (int64_t)iy * W + ix;
    const uint32_t t00 = p[0], t10 = p[1], t01 = p[W], t11 = p[W + 1];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const double c00 = (double)((t00 >> (8 * ch)) & 255u), c10 = (double)((t10 >> (8 * ch)) & 255u);
        const double c01 = (double)((t01 >> (8 * ch)) & 255u), c11 = (double)((t11 >> (8 * ch)) & 255u);
        const double top = (1.0 - fx) * c00 + fx * c10, bot = (1.0 - fx) * c01 + fx * c11;
        c[ch] = (1.0 - fy) * top + fy * bot;
    }
    return true;
}

// mtex_texel with the view's offset o (grey levels) added before the rounding, and the clamp to a byte
DEV uint32_t mtex_texel_levelled(const MtexTri& s, const double o[3], int res, int n1, int n2) {
    const double a0 = (double)(res - n1 - n2) * s.d[0], a1 = (double)n1 * s.d[1], a2 = (double)n2 * s.d[2];
    const double den = a0 + a1 + a2;
    double c[3];
    if (!mtex_colour(s.img, s.W, s.H, a0 * s.sx[0] + a1 * s.sx[1] + a2 * s.sx[2], a0 * s.sy[0] + a1 * s.sy[1] + a2 * s.sy[2], den, c)) return 0x808080u;
    uint32_t out = 0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) out |= (uint32_t)(int)fmin(fmax(floor(c[ch] + o[ch] + 0.5), 0.0), 255.0) << (8 * ch);
    return out;
}

// k_mtex_texels with offset[3 v ..], the levels of view v in 1/16 grey level
__global__ __launch_bounds__(MESH_BLOCK) void k_mtex_texels_levelled(const DView* __restrict__ views, int level, int res, int width, int cpr, int64_t total,
                                                                      int64_t n_cells, int64_t n_textured, const int32_t* __restrict__ list,
                                                                      const int32_t* __restrict__ label, const int32_t* __restrict__ win,
                                                                      const int32_t* __restrict__ offset, uint32_t* __restrict__ rgb, int64_t ngroups) {
    const int64_t g = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (g >= ngroups) return;
    const int B = res + 3;
    const uint32_t p0 = (uint32_t)(4 * g);
    uint32_t row = p0 / (uint32_t)width, col = p0 % (uint32_t)width;
    uint32_t cy = row / (uint32_t)B, j = row % (uint32_t)B, cx = col / (uint32_t)B, i = col % (uint32_t)B;
    MtexTri s;
    s.k = -1;
    double o[3] = {0.0, 0.0, 0.0};
    uint32_t px[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        uint32_t c = 0x808080u;
        const int64_t q = (int64_t)cy * cpr + cx;
        if ((int64_t)p0 + e < total && (int)cx < cpr && q >= 1 && q < n_cells) {
            const bool upper = (int)(i + j) >= res + 3;
            const int64_t k = 2 * (q - 1) + (upper ? 1 : 0);
            if (k < n_textured) {
                if (s.k != (int32_t)k) {
                    mtex_load(s, (int32_t)k, list, label, win, views, level);
                    const int32_t v = label[list[k]];
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) o[ch] = (double)offset[3 * v + ch] / 16.0;
                }
                c = mtex_texel_levelled(s, o, res, upper ? res + 2 - (int)i : (int)i, upper ? res + 2 - (int)j : (int)j);
            }
        }
        px[e] = c;
        // the next texel of the atlas in row order
        if (++col == (uint32_t)width) {
            col = 0; cx = 0; i = 0;
            if (++j == (uint32_t)B) { j = 0; ++cy; }
        } else if (++i == (uint32_t)B) { i = 0; ++cx; }
    }
    uint32_t* out = rgb + 3 * g;
    out[0] = px[0] | px[1] << 24;
    out[1] = px[1] >> 8 | px[2] << 16;
    out[2] = px[2] >> 16 | px[3] << 8;
}

// A lane per edge slot e = 3 t + k.  A seam edge (both triangles flagged, their labels differ, taken from the side with p < q) is sampled
// at its samples + 1 points in both views from the two triangles' own nine numbers; the lane's (N, S_r, S_g, S_b) go to
// pairs[min][max] with the sign.  A wave sums the lanes that share the first one's pair (first_group) until none is left and appends
// one entry a pair to the block's list in LDS; behind the barrier the first entry of each pair sums the block's entries of that pair and
// adds once per component.  *n_edges += the seam edges, one add per wave.  pairs and *n_edges zero before the launch
__global__ __launch_bounds__(MESH_BLOCK) void k_mtex_seam_samples(const DView* __restrict__ views, int level, int nviews, int samples, int64_t n_t,
                                                                   const int32_t* __restrict__ tris, const int32_t* __restrict__ nbr,
                                                                   const int32_t* __restrict__ label, const int32_t* __restrict__ flag,
                                                                   const int32_t* __restrict__ win, long long* __restrict__ pairs, u64* __restrict__ n_edges) {
    __shared__ int32_t s_pair[MESH_BLOCK];
    __shared__ long long s_val[MESH_BLOCK][4];
    __shared__ int s_n;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    const int64_t e = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    int32_t r = -1;
    long long val[4] = {0, 0, 0, 0};
    bool seam = false;
    if (e < 3 * n_t) {
        const int64_t t = e / 3;
        const int k = (int)(e - 3 * t), k1 = (k + 1) % 3;
        const int64_t u = nbr[e];
        const int32_t p = tris[3 * t + k], q = tris[3 * t + k1];
        if (u >= 0 && p < q && flag[t] && flag[u] && label[t] != label[u]) {
            seam = true;
            const int32_t la = label[t], lb = label[u];
            // the corner of u where the reverse edge q -> p starts
            int j = 0;
            if (tris[3 * u + 1] == q && tris[3 * u + 2] == p) j = 1;
            else if (tris[3 * u + 2] == q && tris[3 * u] == p) j = 2;
            const int j1 = (j + 1) % 3;
            const int64_t cp[2] = {9 * t + 3 * k, 9 * u + 3 * j1}, cq[2] = {9 * t + 3 * k1, 9 * u + 3 * j};
            double sxp[2], syp[2], dp[2], sxq[2], syq[2], dq[2];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                sxp[s] = (double)win[cp[s]]; syp[s] = (double)win[cp[s] + 1]; dp[s] = (double)__int_as_float(win[cp[s] + 2]);
                sxq[s] = (double)win[cq[s]]; syq[s] = (double)win[cq[s] + 1]; dq[s] = (double)__int_as_float(win[cq[s] + 2]);
            }
            const DView& va = views[la];
            const DView& vb = views[lb];
            for (int i = 0; i <= samples; ++i) {
                double c[2][3];
                bool good = true;
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const DView& vw = s == 0 ? va : vb;
                    const double ap = (double)(samples - i) * dp[s], aq = (double)i * dq[s];
                    good = mtex_colour(vw.img[level], vw.W[level], vw.H[level], ap * sxp[s] + aq * sxq[s], ap * syp[s] + aq * syq[s], ap + aq, c[s]) && good;
                }
                if (!good) continue;
                val[0] += 1;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) val[1 + ch] += (long long)floor(c[0][ch] * 16.0 + 0.5) - (long long)floor(c[1][ch] * 16.0 + 0.5);
            }
            if (la < lb) r = la * nviews + lb;
            else {
                r = lb * nviews + la;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) val[1 + ch] = -val[1 + ch];
            }
            if (val[0] == 0) r = -1;
        }
    }
    const int lane = lane_id();
    const u64 m = ballot(seam);
    if (m != 0ull && lane == 0) atomicAdd(n_edges, (u64)__popcll(m));
    for (;;) {
        u64 group;
        const bool same = first_group(r, group);
        if (group == 0ull) break;
        long long v[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            u64 x = same ? (u64)val[c] : 0ull;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) x += shfl_xor64(x, off);
            v[c] = (long long)x;
        }
        if (lane == __ffsll((long long)group) - 1) {
            const int at = atomicAdd(&s_n, 1);
            s_pair[at] = r;
#pragma unroll
            for (int c = 0; c < 4; ++c) s_val[at][c] = v[c];
        }
        if (same) r = -1;
    }
    __syncthreads();
    const int n = s_n, me = (int)threadIdx.x;
    if (me < n) {
        const int32_t mine = s_pair[me];
        bool first = true;
        for (int j = 0; j < me; ++j) first = first && s_pair[j] != mine;
        if (first) {
            long long v[4] = {s_val[me][0], s_val[me][1], s_val[me][2], s_val[me][3]};
            for (int j = me + 1; j < n; ++j)
                if (s_pair[j] == mine) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) v[c] += s_val[j][c];
                }
#pragma unroll
            for (int c = 0; c < 4; ++c) atomicAdd(reinterpret_cast<u64*>(pairs) + 4 * (int64_t)mine + c, (u64)v[c]);
        }
    }
}


void mvsk_mtex_check_labels(int64_t n_t, const int32_t* label, int nviews, uint32_t* bad, hipStream_t st) {
    MESH_LAUNCH(k_mtex_check_labels, n_t, n_t, label, nviews, bad);
}
void mvsk_mtex_best(int view, int want, int64_t n_t, const int32_t* tris, const int32_t* scr, const uint32_t* ok, const unsigned long long* visible, int W, int H,
                    long long* best_area, int32_t* best_label, hipStream_t st) {
    MESH_LAUNCH(k_mtex_best, n_t, view, want, n_t, tris, scr, ok, visible, W, H, best_area, best_label);
}
void mvsk_mtex_count(int64_t n_t, const int32_t* label, int nviews, unsigned long long* counts, hipStream_t st) {
    MESH_LAUNCH(k_mtex_count, n_t, n_t, label, nviews, counts);
}
void mvsk_mtex_take(int view, int64_t n_t, const int32_t* tris, const int32_t* label, const int32_t* scr, const float* vd, const uint32_t* ok, int32_t* win,
                    int32_t* flag, hipStream_t st) {
    MESH_LAUNCH(k_mtex_take, n_t, view, n_t, tris, label, scr, vd, ok, win, flag);
}
void mvsk_mtex_layout(int64_t n_t, const int32_t* flag, const int32_t* base, int32_t* list, int64_t n_textured, int res, int cpr, int32_t* uv, hipStream_t st) {
    MESH_LAUNCH(k_mtex_list, n_t, n_t, flag, base, list, n_textured);
    if (uv) MESH_LAUNCH(k_mtex_uv, n_t, n_t, flag, base, res, cpr, uv);
}
void mvsk_mtex_texels(const DParams& prm, int res, int width, int64_t height, int64_t n_textured, const int32_t* list, const int32_t* label, const int32_t* win,
                      uint8_t* rgb, hipStream_t st) {
    const int cpr = width / (res + 3);
    const int64_t total = (int64_t)width * height, n_cells = 1 + (n_textured + 1) / 2, ngroups = (total + 3) / 4;
    MESH_LAUNCH(k_mtex_texels, ngroups, prm.views, prm.level, res, width, cpr, total, n_cells, n_textured, list, label, win, reinterpret_cast<uint32_t*>(rgb), ngroups);
}
void mvsk_mtex_quality(int view, int want, int64_t n_t, const int32_t* tris, const int32_t* scr, const uint32_t* ok, const unsigned long long* visible, int W, int H,
                       const long long* best_area, int nviews, uint8_t* quality, hipStream_t st) {
    MESH_LAUNCH(k_mtex_quality, n_t, view, want, n_t, tris, scr, ok, visible, W, H, best_area, nviews, quality);
}
void mvsk_mtex_texels_levelled(const DParams& prm, int res, int width, int64_t height, int64_t n_textured, const int32_t* list, const int32_t* label,
                               const int32_t* win, const int32_t* offset, uint8_t* rgb, hipStream_t st) {
    const int cpr = width / (res + 3);
    const int64_t total = (int64_t)width * height, n_cells = 1 + (n_textured + 1) / 2, ngroups = (total + 3) / 4;
    MESH_LAUNCH(k_mtex_texels_levelled, ngroups, prm.views, prm.level, res, width, cpr, total, n_cells, n_textured, list, label, win, offset,
                reinterpret_cast<uint32_t*>(rgb), ngroups);
}
void mvsk_mtex_seam_samples(const DParams& prm, int nviews, int samples, int64_t n_t, const int32_t* tris, const int32_t* nbr, const int32_t* label,
                            const int32_t* flag, const int32_t* win, long long* pairs, unsigned long long* n_edges, hipStream_t st) {
    MESH_LAUNCH(k_mtex_seam_samples, 3 * n_t, prm.views, prm.level, nviews, samples, n_t, tris, nbr, label, flag, win, pairs, n_edges);
}
