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
