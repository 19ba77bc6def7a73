// mvs_engine_mesh.cpp -- the mesh calls of the C ABI in include/mvskit_engine.h: the TSDF volume over the dense maps and its extraction
// (mvs_mesh.hip), vertex normals and colours (mvs_mesh_attr.hip), components, pruning and smoothing (mvs_mesh_clean.hip), decimation
// (mvs_mesh_decimate.hip), boundary loops and hole filling (mvs_mesh_fill.hip), the mesh rendered into the views and the vertex
// visibility (mvs_mesh_render.hip), the view of each triangle and the texture atlas (mvs_mesh_texture.hip; declared in
// include/mvskit_texture.h), the adjacency of triangles, the smoothed view labels and the levels on the seams (mvs_mesh_seams.hip and
// mvs_mesh_texture.hip; declared in include/mvskit_seams.h).  The maps they start from come from
// mvs_engine_output.cpp (render_usable).  Every entry point is stateless: its working arrays live in buffers of the call, the caller's
// arrays come into them from wherever they lie, and nothing of the engine's state changes.
#include <cmath>
#include <cstdlib>

#include "mvs_engine_impl.h"
#include "mvskit_seams.h"

using namespace mvseng;

// The argument checks that the entry points share, in the order they fire, and the copy of the caller's rows
namespace {
int mesh_out_args(int64_t cap_v, int64_t cap_t, const int64_t* n_v, const int64_t* n_t, const char* who) {
    if (!n_v || !n_t) { g_err = std::string(who) + ": n_v or n_t null"; return MVS_ERR_ARG; }
    if (cap_v < 0 || cap_t < 0) { g_err = std::string(who) + ": a negative cap"; return MVS_ERR_ARG; }
    return MVS_OK;
}
#define MESH_ATTR_MAX ((int64_t)1 << 30)
int mesh_counts(int64_t n_v, int64_t n_t, const char* who) {
    if (n_v < 0 || n_t < 0 || n_v > MESH_ATTR_MAX || n_t > MESH_ATTR_MAX) { g_err = std::string(who) + ": a count negative or over 2^30"; return MVS_ERR_ARG; }
    return MVS_OK;
}
// the input mesh of an entry point that takes both arrays: the counts, then each array where its count asks for one
int mesh_in_args(int64_t n_v, const float* verts, int64_t n_t, const int32_t* tris, const char* who) {
    if (int r = mesh_counts(n_v, n_t, who)) return r;
    if (!verts && n_v > 0) { g_err = std::string(who) + ": verts null"; return MVS_ERR_ARG; }
    if (!tris && n_t > 0) { g_err = std::string(who) + ": tris null"; return MVS_ERR_ARG; }
    return MVS_OK;
}
// the caller's n rows of three (vertices or triangles) into a buffer that holds them, from wherever they lie
template <typename T> int upload_rows(mvs_engine* e, T* dst, const T* src, int64_t n) {
    if (n > 0) HIPCHK(hipMemcpyAsync(dst, src, (size_t)n * 3 * sizeof(T), hipMemcpyDefault, e->stream));
    return MVS_OK;
}
}  // namespace

extern "C" {

// Triangle mesh (mvs_mesh.hip; the definitions are in mvskit_engine.h).  Stateless like the maps calls: the volume and every working
// array live in buffers of the call.  mesh_tsdf leaves the volume on the device, mesh_extract takes one from there; the three entry
// points differ in where the volume comes from and goes to.
static_assert(sizeof(mvs_volume) == 40, "mvs_volume is 40 bytes");
namespace {
int volume_args(const mvs_volume* vol, const char* who) {
    if (!vol) { g_err = std::string(who) + ": volume null"; return MVS_ERR_ARG; }
    if (!std::isfinite(vol->voxel) || !(vol->voxel > 0.0f)) { g_err = std::string(who) + ": voxel not finite or <= 0"; return MVS_ERR_ARG; }
    if (!std::isfinite(vol->trunc) || !(vol->trunc > 0.0f)) { g_err = std::string(who) + ": trunc not finite or <= 0"; return MVS_ERR_ARG; }
    for (int c = 0; c < 3; ++c)
        if (vol->dims[c] < 2 || vol->dims[c] > 1024) { g_err = std::string(who) + ": a dimension outside 2..1024"; return MVS_ERR_ARG; }
    if ((int64_t)vol->dims[0] * vol->dims[1] * vol->dims[2] > ((int64_t)1 << 28)) { g_err = std::string(who) + ": more than 2^28 lattice points"; return MVS_ERR_ARG; }
    if (vol->min_count < 1) { g_err = std::string(who) + ": min_count < 1"; return MVS_ERR_ARG; }
    return MVS_OK;
}
MeshVol mesh_vol(const mvs_volume* vol) {
    return MeshVol{{vol->origin[0], vol->origin[1], vol->origin[2]}, vol->voxel, vol->dims[0], vol->dims[1], vol->dims[2], vol->trunc, vol->min_count};
}
struct MeshVolume {
    DevBuf<float> tsdf;
    DevBuf<int32_t> count;
};

// the volume of the engine's maps into d (the stream is idle on return)
int mesh_tsdf(mvs_engine* e, const mvs_maps_config* c, const MeshVol& mv, MeshVolume& d) {
    hipStream_t st = e->stream;
    const int64_t N = mesh_npoints(mv);
    MapsBufs b;
    if (int r = render_usable(e, c, b)) return r;
    if (d.tsdf.ensure(N) || d.count.ensure(N)) return MVS_ERR_HIP;
    const DParams p = current_params(e);
    mvsk_mesh_tsdf(p, b.args, mv, b.ids.p, b.flag8.p, d.tsdf.p, d.count.p, st);
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    return MVS_OK;
}

// marching tetrahedra over a device volume (count may be null)
int mesh_extract(mvs_engine* e, const MeshVol& mv, const float* d_tsdf, const int32_t* d_count, int64_t cap_v, float* verts, int64_t cap_t, int32_t* tris,
                 int64_t* n_v, int64_t* n_t, const char* who) {
    hipStream_t st = e->stream;
    const int64_t N = mesh_npoints(mv);
    DevBuf<uint8_t> state, mask;
    DevBuf<int32_t> cnt, vbase, d_tris;
    DevBuf<int64_t> tbase, scan;
    DevBuf<float> d_verts;
    if (state.ensure(N) || mask.ensure(N) || cnt.ensure(N + 1) || vbase.ensure(N + 1) || tbase.ensure(N + 1) || scan.ensure(N / 256 + 4096)) return MVS_ERR_HIP;
    mvsk_mesh_state(mv, d_tsdf, d_count, state.p, st);
    mvsk_mesh_edges(mv, state.p, mask.p, cnt.p, st);
    mvsk_exclusive_scan(cnt.p, vbase.p, N, reinterpret_cast<int32_t*>(scan.p), st);
    mvsk_mesh_tcount(mv, state.p, cnt.p, st);
    mvsk_exclusive_scan_off(cnt.p, tbase.p, N, scan.p, st);
    int32_t nv32 = 0;
    int64_t nt = 0;
    HIPCHK(hipMemcpyAsync(&nv32, vbase.p + N, sizeof nv32, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&nt, tbase.p + N, sizeof nt, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    const int64_t nv = nv32;
    *n_v = nv; *n_t = nt;
    if ((verts && cap_v < nv) || (tris && cap_t < nt)) { g_err = std::string(who) + ": a cap is smaller than the mesh (*n_v, *n_t)"; return MVS_ERR_CAPACITY; }
    if (!verts || !tris) return MVS_OK;
    if (nv > 0) {
        if (d_verts.ensure(3 * nv)) return MVS_ERR_HIP;
        mvsk_mesh_verts(mv, d_tsdf, mask.p, vbase.p, d_verts.p, nv, st);
        HIPCHK(hipMemcpyAsync(verts, d_verts.p, (size_t)nv * 3 * sizeof(float), hipMemcpyDefault, st));
    }
    if (nt > 0) {
        if (d_tris.ensure(3 * nt)) return MVS_ERR_HIP;
        mvsk_mesh_tris(mv, state.p, mask.p, vbase.p, tbase.p, d_tris.p, nt, st);
        HIPCHK(hipMemcpyAsync(tris, d_tris.p, (size_t)nt * 3 * sizeof(int32_t), hipMemcpyDefault, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    return MVS_OK;
}
}  // namespace

int mvs_engine_tsdf(mvs_engine* e, const mvs_maps_config* c, const mvs_volume* vol, float* tsdf, int32_t* count) {
    const char* who = "mvs_engine_tsdf";
    if (int r = maps_args(c, who)) return r;
    if (int r = volume_args(vol, who)) return r;
    if (!tsdf || !count) { g_err = std::string(who) + ": tsdf or count null"; return MVS_ERR_ARG; }
    if (int r = maps_state(e, c, who)) return r;
    HIPCHK(hipSetDevice(e->cfg.device));
    Range rg("mvs:tsdf");
    const MeshVol mv = mesh_vol(vol);
    const int64_t N = mesh_npoints(mv);
    MeshVolume d;
    if (int r = mesh_tsdf(e, c, mv, d)) return r;
    HIPCHK(hipMemcpyAsync(tsdf, d.tsdf.p, (size_t)N * sizeof(float), hipMemcpyDefault, e->stream));
    HIPCHK(hipMemcpyAsync(count, d.count.p, (size_t)N * sizeof(int32_t), hipMemcpyDefault, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return MVS_OK;
}

int mvs_engine_extract_mesh(mvs_engine* e, const mvs_volume* vol, const float* tsdf, const int32_t* count, int64_t cap_v, float* verts, int64_t cap_t,
                            int32_t* tris, int64_t* n_v, int64_t* n_t) {
    const char* who = "mvs_engine_extract_mesh";
    if (int r = volume_args(vol, who)) return r;
    if (!tsdf) { g_err = std::string(who) + ": tsdf null"; return MVS_ERR_ARG; }
    if (int r = mesh_out_args(cap_v, cap_t, n_v, n_t, who)) return r;
    if (int r = need_state(e, NEED_ENGINE, who)) return r;
    HIPCHK(hipSetDevice(e->cfg.device));
    Range rg("mvs:extract_mesh");
    const MeshVol mv = mesh_vol(vol);
    const int64_t N = mesh_npoints(mv);
    MeshVolume d;  // the caller's volume, from wherever it lies
    if (d.tsdf.ensure(N) || (count && d.count.ensure(N))) return MVS_ERR_HIP;
    HIPCHK(hipMemcpyAsync(d.tsdf.p, tsdf, (size_t)N * sizeof(float), hipMemcpyDefault, e->stream));
    if (count) HIPCHK(hipMemcpyAsync(d.count.p, count, (size_t)N * sizeof(int32_t), hipMemcpyDefault, e->stream));
    return mesh_extract(e, mv, d.tsdf.p, count ? d.count.p : nullptr, cap_v, verts, cap_t, tris, n_v, n_t, who);
}

int mvs_engine_mesh(mvs_engine* e, const mvs_maps_config* c, const mvs_volume* vol, int64_t cap_v, float* verts, int64_t cap_t, int32_t* tris,
                    int64_t* n_v, int64_t* n_t) {
    const char* who = "mvs_engine_mesh";
    if (int r = maps_args(c, who)) return r;
    if (int r = volume_args(vol, who)) return r;
    if (int r = mesh_out_args(cap_v, cap_t, n_v, n_t, who)) return r;
    if (int r = maps_state(e, c, who)) return r;
    HIPCHK(hipSetDevice(e->cfg.device));
    Range rg("mvs:mesh");
    const MeshVol mv = mesh_vol(vol);
    MeshVolume d;
    if (int r = mesh_tsdf(e, c, mv, d)) return r;
    return mesh_extract(e, mv, d.tsdf.p, d.count.p, cap_v, verts, cap_t, tris, n_v, n_t, who);
}

// Vertex normals and colours of a mesh (mvs_mesh_attr.hip; the definitions are in mvskit_engine.h).  Stateless like the mesh calls: the
// caller's arrays come into buffers of the call from wherever they lie, the results leave from there.
static_assert(sizeof(mvs_mesh_colouring) == 8, "mvs_mesh_colouring is 8 bytes");

int mvs_engine_mesh_normals(mvs_engine* e, int64_t n_v, const float* verts, int64_t n_t, const int32_t* tris, float* normals) {
    const char* who = "mvs_engine_mesh_normals";
    if (int r = mesh_in_args(n_v, verts, n_t, tris, who)) return r;
    if (!normals && n_v > 0) { g_err = std::string(who) + ": normals null"; return MVS_ERR_ARG; }
    if (int r = need_state(e, NEED_ENGINE, who)) return r;
    if (n_v == 0 && n_t == 0) return MVS_OK;
    HIPCHK(hipSetDevice(e->cfg.device));
    Range rg("mvs:mesh_normals");
    hipStream_t st = e->stream;
    DevBuf<float> d_verts, d_normals;
    DevBuf<int32_t> d_tris;
    DevBuf<long long> acc;
    DevBuf<uint32_t> words;  // [0] the bits of the largest component, [1] an index out of range
    if (d_verts.ensure(3 * n_v) || d_tris.ensure(3 * n_t) || words.ensure(2)) return MVS_ERR_HIP;
    if (int r = upload_rows(e, d_verts.p, verts, n_v)) return r;
    if (int r = upload_rows(e, d_tris.p, tris, n_t)) return r;
    HIPCHK(hipMemsetAsync(words.p, 0, 2 * sizeof(uint32_t), st));
    mvsk_mesh_normals_scan(n_v, d_verts.p, n_t, d_tris.p, words.p, words.p + 1, st);
    uint32_t bad = 0;
    if (int r = read_back(e, words.p + 1, &bad)) return r;
    HIPCHK(hipGetLastError());
    if (bad) { g_err = std::string(who) + ": a vertex index outside 0 .. n_v - 1"; return MVS_ERR_ARG; }
    if (n_v == 0) return MVS_OK;
    if (acc.ensure(3 * n_v) || d_normals.ensure(3 * n_v)) return MVS_ERR_HIP;
    HIPCHK(hipMemsetAsync(acc.p, 0, (size_t)n_v * 3 * sizeof(long long), st));
    mvsk_mesh_normals_accum(d_verts.p, n_t, d_tris.p, words.p, acc.p, st);
    mvsk_mesh_normals_finish(n_v, acc.p, d_normals.p, st);
    HIPCHK(hipMemcpyAsync(normals, d_normals.p, (size_t)n_v * 3 * sizeof(float), hipMemcpyDefault, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    return MVS_OK;
}

void mvs_default_mesh_colouring(mvs_mesh_colouring* m) {
    if (!m) return;
    m->occl_tol = 0.01f; m->min_cos = 0.1f;
}

namespace {
// both colouring calls; visible (host or device memory) may be null: no gate then, and k_mattr_colours runs as it always did
int mesh_colours(mvs_engine* e, const mvs_maps_config* c, const mvs_mesh_colouring* m, int64_t n_v, const float* verts, const float* normals,
                 const uint64_t* visible, uint8_t* rgb, uint8_t* used, const char* who) {
    if (int r = maps_args(c, who)) return r;
    if (!m) { g_err = std::string(who) + ": colouring null"; return MVS_ERR_ARG; }
    if (!std::isfinite(m->occl_tol) || !(m->occl_tol > 0.0f)) { g_err = std::string(who) + ": occl_tol not finite or <= 0"; return MVS_ERR_ARG; }
    if (!std::isfinite(m->min_cos) || !(m->min_cos >= -1.0f && m->min_cos <= 1.0f)) { g_err = std::string(who) + ": min_cos not finite or outside [-1, 1]"; return MVS_ERR_ARG; }
    if (n_v < 0 || n_v > MESH_ATTR_MAX) { g_err = std::string(who) + ": n_v negative or over 2^30"; return MVS_ERR_ARG; }
    if ((!verts || !rgb) && n_v > 0) { g_err = std::string(who) + ": verts or rgb null"; return MVS_ERR_ARG; }
    if (int r = maps_state(e, c, who)) return r;
    if (n_v == 0) return MVS_OK;
    HIPCHK(hipSetDevice(e->cfg.device));
    Range rg("mvs:mesh_colours");
    hipStream_t st = e->stream;
    DevBuf<float> d_verts, d_normals;
    DevBuf<uint8_t> d_rgb, d_used;
    DevBuf<unsigned long long> d_visible;
    if (d_rgb.ensure(3 * n_v) || d_used.ensure(n_v)) return MVS_ERR_HIP;
    int64_t alive = 0;
    if (int r = mvs_engine_num_patches(e, &alive)) return r;
    MapsBufs b;
    if (alive == 0) {  // no surface to hold a vertex against: no view counts
        HIPCHK(hipMemsetAsync(d_rgb.p, 128, (size_t)n_v * 3, st));
        HIPCHK(hipMemsetAsync(d_used.p, 0, (size_t)n_v, st));
    } else {
        if (int r = render_usable(e, c, b)) return r;
        if (d_verts.ensure(3 * n_v) || (normals && d_normals.ensure(3 * n_v))) return MVS_ERR_HIP;
        if (int r = upload_rows(e, d_verts.p, verts, n_v)) return r;
        if (normals) HIPCHK(hipMemcpyAsync(d_normals.p, normals, (size_t)n_v * 3 * sizeof(float), hipMemcpyDefault, st));
        if (visible) {
            if (d_visible.ensure(n_v)) return MVS_ERR_HIP;
            HIPCHK(hipMemcpyAsync(d_visible.p, visible, (size_t)n_v * sizeof(uint64_t), hipMemcpyDefault, st));
            mvsk_mesh_colours_visible(current_params(e), b.args, MeshColourArgs{m->occl_tol, m->min_cos}, n_v, d_verts.p, normals ? d_normals.p : nullptr,
                                      b.ids.p, b.flag8.p, d_visible.p, d_rgb.p, d_used.p, st);
        } else {
            mvsk_mesh_colours(current_params(e), b.args, MeshColourArgs{m->occl_tol, m->min_cos}, n_v, d_verts.p, normals ? d_normals.p : nullptr, b.ids.p,
                              b.flag8.p, d_rgb.p, d_used.p, st);
        }
    }
    HIPCHK(hipMemcpyAsync(rgb, d_rgb.p, (size_t)n_v * 3, hipMemcpyDefault, st));
    if (used) HIPCHK(hipMemcpyAsync(used, d_used.p, (size_t)n_v, hipMemcpyDefault, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    return MVS_OK;
}
}  // namespace

int mvs_engine_mesh_colours(mvs_engine* e, const mvs_maps_config* c, const mvs_mesh_colouring* m, int64_t n_v, const float* verts, const float* normals,
                            uint8_t* rgb, uint8_t* used) {
    return mesh_colours(e, c, m, n_v, verts, normals, nullptr, rgb, used, "mvs_engine_mesh_colours");
}

int mvs_engine_mesh_colours_visible(mvs_engine* e, const mvs_maps_config* c, const mvs_mesh_colouring* m, int64_t n_v, const float* verts, const float* normals,
                                    const uint64_t* visible, uint8_t* rgb, uint8_t* used) {
    return mesh_colours(e, c, m, n_v, verts, normals, visible, rgb, used, "mvs_engine_mesh_colours_visible");
}

// Mesh clean-up (mvs_mesh_clean.hip; the definitions are in mvskit_engine.h): components, pruning, smoothing.  Stateless like the
// attribute calls: the caller's arrays come into buffers of the call from wherever they lie, the results leave from there.
static_assert(sizeof(mvs_mesh_pruning) == 16, "mvs_mesh_pruning is 16 bytes");
static_assert(sizeof(mvs_mesh_smoothing) == 16, "mvs_mesh_smoothing is 16 bytes");
namespace {
// the caller's triangles into d_tris, their ids checked (words: one zeroed word of scratch); the stream is idle on return
int mesh_take_tris(mvs_engine* e, int64_t n_v, int64_t n_t, const int32_t* tris, DevBuf<int32_t>& d_tris, DevBuf<uint32_t>& words, const char* who) {
    hipStream_t st = e->stream;
    if (d_tris.ensure(3 * n_t) || words.ensure(2)) return MVS_ERR_HIP;
    if (int r = upload_rows(e, d_tris.p, tris, n_t)) return r;
    HIPCHK(hipMemsetAsync(words.p, 0, 2 * sizeof(uint32_t), st));
    mvsk_mesh_check_ids(n_v, n_t, d_tris.p, words.p, st);
    uint32_t bad = 0;
    if (int r = read_back(e, words.p, &bad)) return r;
    HIPCHK(hipGetLastError());
    if (bad) { g_err = std::string(who) + ": a vertex index outside 0 .. n_v - 1"; return MVS_ERR_ARG; }
    return MVS_OK;
}
// labels and per-vertex triangle counts of valid triangles on the device (launched, not waited for); ncomp: one word, zeroed here
int mesh_label(mvs_engine* e, int64_t n_v, int64_t n_t, const int32_t* d_tris, DevBuf<int32_t>& parent, DevBuf<int32_t>& size, DevBuf<unsigned long long>& ncomp) {
    if (parent.ensure(n_v) || size.ensure(n_v) || ncomp.ensure(2)) return MVS_ERR_HIP;
    HIPCHK(hipMemsetAsync(ncomp.p, 0, 2 * sizeof(unsigned long long), e->stream));
    mvsk_mesh_components(n_v, n_t, d_tris, parent.p, size.p, ncomp.p, e->stream);
    return MVS_OK;
}
}  // namespace

int mvs_engine_mesh_components(mvs_engine* e, int64_t n_v, int64_t n_t, const int32_t* tris, int32_t* label, int32_t* ntris, int64_t* n_components) {
    const char* who = "mvs_engine_mesh_components";
    if (int r = mesh_counts(n_v, n_t, who)) return r;
    if (!tris && n_t > 0) { g_err = std::string(who) + ": tris null"; return MVS_ERR_ARG; }
    if (int r = need_state(e, NEED_ENGINE, who)) return r;
    if (n_v == 0 && n_t == 0) { if (n_components) *n_components = 0; return MVS_OK; }
    HIPCHK(hipSetDevice(e->cfg.device));
    Range rg("mvs:mesh_components");
    hipStream_t st = e->stream;
    DevBuf<int32_t> d_tris, parent, size;
    DevBuf<uint32_t> words;
    DevBuf<unsigned long long> ncomp;
    if (int r = mesh_take_tris(e, n_v, n_t, tris, d_tris, words, who)) return r;
    if (int r = mesh_label(e, n_v, n_t, d_tris.p, parent, size, ncomp)) return r;
    unsigned long long nc = 0;
    if (int r = read_back(e, ncomp.p, &nc)) return r;  // a failure is known before anything is written
    HIPCHK(hipGetLastError());
    if (label && n_v > 0) HIPCHK(hipMemcpyAsync(label, parent.p, (size_t)n_v * sizeof(int32_t), hipMemcpyDefault, st));
    if (ntris && n_v > 0) HIPCHK(hipMemcpyAsync(ntris, size.p, (size_t)n_v * sizeof(int32_t), hipMemcpyDefault, st));
    HIPCHK(hipStreamSynchronize(st));
    if (n_components) *n_components = (int64_t)nc;
    return MVS_OK;
}

void mvs_default_mesh_pruning(mvs_mesh_pruning* p) {
    if (!p) return;
    p->min_triangles = 1; p->largest_only = 0; p->pad = 0;
}

int mvs_engine_mesh_prune(mvs_engine* e, const mvs_mesh_pruning* p, int64_t n_v, const float* verts, int64_t n_t, const int32_t* tris, int64_t cap_v,
                          float* out_verts, int64_t cap_t, int32_t* out_tris, int32_t* vmap, int64_t* n_v_out, int64_t* n_t_out) {
    const char* who = "mvs_engine_mesh_prune";
    if (!p) { g_err = std::string(who) + ": pruning null"; return MVS_ERR_ARG; }
    if (p->min_triangles < 1) { g_err = std::string(who) + ": min_triangles < 1"; return MVS_ERR_ARG; }
    if (p->largest_only != 0 && p->largest_only != 1) { g_err = std::string(who) + ": largest_only not 0 or 1"; return MVS_ERR_ARG; }
    if (int r = mesh_in_args(n_v, verts, n_t, tris, who)) return r;
    if (int r = mesh_out_args(cap_v, cap_t, n_v_out, n_t_out, who)) return r;
    if (int r = need_state(e, NEED_ENGINE, who)) return r;
    if (n_v == 0 && n_t == 0) { *n_v_out = 0; *n_t_out = 0; return MVS_OK; }
    HIPCHK(hipSetDevice(e->cfg.device));
    Range rg("mvs:mesh_prune");
    hipStream_t st = e->stream;
    DevBuf<int32_t> d_tris, parent, size, vflag, vbase, tflag, tbase, scan, d_out_tris;
    DevBuf<uint32_t> words;
    DevBuf<unsigned long long> ncomp;  // [0] the components, [1] the largest one's key
    DevBuf<float> d_verts, d_out_verts;
    if (int r = mesh_take_tris(e, n_v, n_t, tris, d_tris, words, who)) return r;
    if (int r = mesh_label(e, n_v, n_t, d_tris.p, parent, size, ncomp)) return r;
    if (vflag.ensure(n_v) || vbase.ensure(n_v + 1) || tflag.ensure(n_t) || tbase.ensure(n_t + 1) || scan.ensure(std::max(n_v, n_t) / 256 + 4096)) return MVS_ERR_HIP;
    if (n_v > 0) HIPCHK(hipMemsetAsync(vflag.p, 0, (size_t)n_v * sizeof(int32_t), st));
    if (p->largest_only) mvsk_mesh_largest(n_v, parent.p, size.p, ncomp.p + 1, st);
    mvsk_mesh_keep(n_t, d_tris.p, parent.p, size.p, p->min_triangles, p->largest_only, ncomp.p + 1, tflag.p, vflag.p, st);
    int64_t nv = 0, nt = 0;
    if (int r = scan_total(e, vflag.p, vbase.p, scan.p, n_v, &nv)) return r;
    if (int r = scan_total(e, tflag.p, tbase.p, scan.p, n_t, &nt)) return r;
    *n_v_out = nv; *n_t_out = nt;
    if ((out_verts && cap_v < nv) || (out_tris && cap_t < nt)) { g_err = std::string(who) + ": a cap is smaller than the pruned mesh (*n_v_out, *n_t_out)"; return MVS_ERR_CAPACITY; }
    if (!out_verts || !out_tris) return MVS_OK;
    if (d_verts.ensure(3 * n_v) || d_out_verts.ensure(3 * nv) || d_out_tris.ensure(3 * nt)) return MVS_ERR_HIP;
    if (int r = upload_rows(e, d_verts.p, verts, n_v)) return r;
    mvsk_mesh_gather(n_v, d_verts.p, vflag.p, vbase.p, d_out_verts.p, nv, n_t, d_tris.p, tflag.p, tbase.p, d_out_tris.p, nt, st);
    if (nv > 0) HIPCHK(hipMemcpyAsync(out_verts, d_out_verts.p, (size_t)nv * 3 * sizeof(float), hipMemcpyDefault, st));
    if (nt > 0) HIPCHK(hipMemcpyAsync(out_tris, d_out_tris.p, (size_t)nt * 3 * sizeof(int32_t), hipMemcpyDefault, st));
    if (vmap && n_v > 0) HIPCHK(hipMemcpyAsync(vmap, vflag.p, (size_t)n_v * sizeof(int32_t), hipMemcpyDefault, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    return MVS_OK;
}

void mvs_default_mesh_smoothing(mvs_mesh_smoothing* s) {
    if (!s) return;
    s->iterations = 10; s->lambda = 0.5f; s->mu = -0.53f; s->pad = 0;
}

int mvs_engine_mesh_smooth(mvs_engine* e, const mvs_mesh_smoothing* s, int64_t n_v, const float* verts, int64_t n_t, const int32_t* tris, float* out_verts) {
    const char* who = "mvs_engine_mesh_smooth";
    if (!s) { g_err = std::string(who) + ": smoothing null"; return MVS_ERR_ARG; }
    if (s->iterations < 0 || s->iterations > 1000) { g_err = std::string(who) + ": iterations outside 0..1000"; return MVS_ERR_ARG; }
    if (!std::isfinite(s->lambda) || !(s->lambda > 0.0f && s->lambda < 1.0f)) { g_err = std::string(who) + ": lambda not finite or outside (0, 1)"; return MVS_ERR_ARG; }
    if (!std::isfinite(s->mu) || !(s->mu > -1.0f && s->mu <= 0.0f)) { g_err = std::string(who) + ": mu not finite or outside (-1, 0]"; return MVS_ERR_ARG; }
    if (int r = mesh_counts(n_v, n_t, who)) return r;
    if (((!verts || !out_verts) && n_v > 0) || (!tris && n_t > 0)) { g_err = std::string(who) + ": verts, tris or out_verts null"; return MVS_ERR_ARG; }
    if (int r = need_state(e, NEED_ENGINE, who)) return r;
    if (n_v == 0 && n_t == 0) return MVS_OK;
    HIPCHK(hipSetDevice(e->cfg.device));
    Range rg("mvs:mesh_smooth");
    hipStream_t st = e->stream;
    const bool two = s->mu != 0.0f;
    const int steps = s->iterations * (two ? 2 : 1);
    DevBuf<int32_t> d_tris, cnt;
    DevBuf<uint32_t> words, mbits;  // mbits: the bits of the largest component, a word per step
    DevBuf<float> xa, xb;
    DevBuf<long long> acc;
    if (int r = mesh_take_tris(e, n_v, n_t, tris, d_tris, words, who)) return r;
    if (n_v == 0) return MVS_OK;
    if (xa.ensure(3 * n_v) || xb.ensure(3 * n_v) || acc.ensure(3 * n_v) || cnt.ensure(n_v) || mbits.ensure(steps + 1)) return MVS_ERR_HIP;
    if (int r = upload_rows(e, xa.p, verts, n_v)) return r;
    HIPCHK(hipMemsetAsync(acc.p, 0, (size_t)n_v * 3 * sizeof(long long), st));
    HIPCHK(hipMemsetAsync(cnt.p, 0, (size_t)n_v * sizeof(int32_t), st));
    HIPCHK(hipMemsetAsync(mbits.p, 0, (size_t)(steps + 1) * sizeof(uint32_t), st));
    float *from = xa.p, *to = xb.p;
    for (int k = 0; k < steps; ++k) {
        mvsk_mesh_smooth_step(n_v, from, to, (two && (k & 1)) ? s->mu : s->lambda, n_t, d_tris.p, mbits.p + k, acc.p, cnt.p, st);
        std::swap(from, to);
    }
    HIPCHK(hipStreamSynchronize(st));  // a failure is known before anything is written
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_verts, from, (size_t)n_v * 3 * sizeof(float), hipMemcpyDefault, st));
    HIPCHK(hipStreamSynchronize(st));
    return MVS_OK;
}

// Mesh decimation (mvs_mesh_decimate.hip; the definition is in mvskit_engine.h): vertex clustering on the caller's grid.  Stateless like
// the clean-up calls.  One table serves three fills: the cells of the members, then the two keys that find the duplicate triangles.
static_assert(sizeof(mvs_mesh_decimation) == 24, "mvs_mesh_decimation is 24 bytes");
namespace {
// the slots of an open-addressing table for n keys (decimation's and hole filling's): a power of two, at least twice n
int64_t table_slots(int64_t n) {
    int64_t s = 1024;
    while (s < 2 * n) s <<= 1;
    return s;
}
// every slot free (all ones), every byte of the values value_byte: 0x7f in front of decimation's minima, 0 in front of filling's counts
int table_reset(mvs_engine* e, unsigned long long* tkey, int32_t* tval, int64_t slots, int value_byte) {
    HIPCHK(hipMemsetAsync(tkey, 0xff, (size_t)slots * sizeof(unsigned long long), e->stream));
    HIPCHK(hipMemsetAsync(tval, value_byte, (size_t)slots * sizeof(int32_t), e->stream));
    return MVS_OK;
}
// an empty table of table_slots(n) slots, then out[i] = the smallest item that carries key[i]
int mdec_fill(mvs_engine* e, int64_t n, const unsigned long long* key, DevBuf<unsigned long long>& tkey, DevBuf<int32_t>& tval, int32_t* out, uint32_t* fail) {
    if (n == 0) return MVS_OK;
    const int64_t slots = table_slots(n);
    if (int r = table_reset(e, tkey.p, tval.p, slots, 0x7f)) return r;
    mvsk_mdec_table(n, key, tkey.p, tval.p, slots, out, fail, e->stream);
    return MVS_OK;
}
}  // namespace

void mvs_default_mesh_decimation(mvs_mesh_decimation* d) {
    if (!d) return;
    d->origin[0] = d->origin[1] = d->origin[2] = 0.0f;
    d->cell = 1.0f; d->placement = 0; d->pad = 0;
}

int mvs_engine_mesh_decimate(mvs_engine* e, const mvs_mesh_decimation* d, int64_t n_v, const float* verts, int64_t n_t, const int32_t* tris, int64_t cap_v,
                             float* out_verts, int64_t cap_t, int32_t* out_tris, int32_t* vmap, int64_t* n_v_out, int64_t* n_t_out) {
    const char* who = "mvs_engine_mesh_decimate";
    if (!d) { g_err = std::string(who) + ": decimation null"; return MVS_ERR_ARG; }
    if (!std::isfinite(d->cell) || !(d->cell > 0.0f)) { g_err = std::string(who) + ": cell not finite or <= 0"; return MVS_ERR_ARG; }
    if (!std::isfinite(d->origin[0]) || !std::isfinite(d->origin[1]) || !std::isfinite(d->origin[2])) { g_err = std::string(who) + ": origin not finite"; return MVS_ERR_ARG; }
    if (d->placement != 0 && d->placement != 1) { g_err = std::string(who) + ": placement not 0 or 1"; return MVS_ERR_ARG; }
    if (int r = mesh_in_args(n_v, verts, n_t, tris, who)) return r;
    if (int r = mesh_out_args(cap_v, cap_t, n_v_out, n_t_out, who)) return r;
    if (int r = need_state(e, NEED_ENGINE, who)) return r;
    if (n_v == 0 && n_t == 0) { *n_v_out = 0; *n_t_out = 0; return MVS_OK; }
    HIPCHK(hipSetDevice(e->cfg.device));
    Range rg("mvs:mesh_decimate");
    hipStream_t st = e->stream;
    DevBuf<int32_t> d_tris, used, rep, tval, tans, tflag, tbase, vflag, vbase, scan, cnt, d_out_tris;
    DevBuf<uint32_t> words, flags;  // flags: [0] the bits of the members' largest component, [1] a member not finite or outside the grid, [2] a probe that ran out
    DevBuf<unsigned long long> vkey, tkeys, tkey, best;
    DevBuf<long long> acc;
    DevBuf<float> d_verts, d_out_verts;
    if (int r = mesh_take_tris(e, n_v, n_t, tris, d_tris, words, who)) return r;
    const int64_t slots = table_slots(std::max(n_v, n_t));
    if (d_verts.ensure(3 * n_v) || used.ensure(n_v) || vkey.ensure(n_v) || rep.ensure(n_v) || flags.ensure(4) || tkey.ensure(slots) || tval.ensure(slots)) return MVS_ERR_HIP;
    if (int r = upload_rows(e, d_verts.p, verts, n_v)) return r;
    if (n_v > 0) HIPCHK(hipMemsetAsync(used.p, 0, (size_t)n_v * sizeof(int32_t), st));
    HIPCHK(hipMemsetAsync(flags.p, 0, 4 * sizeof(uint32_t), st));
    mvsk_mdec_members(n_v, d_verts.p, n_t, d_tris.p, d->origin, d->cell, used.p, vkey.p, flags.p, flags.p + 1, st);
    if (int r = mdec_fill(e, n_v, vkey.p, tkey, tval, rep.p, flags.p + 2)) return r;  // a refused member has no key
    uint32_t hf[4] = {0, 0, 0, 0};
    HIPCHK(hipMemcpyAsync(hf, flags.p, sizeof(hf), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    if (hf[1]) { g_err = std::string(who) + ": a member with a non-finite component or a cell index outside -2^20 .. 2^20 - 1"; return MVS_ERR_ARG; }
    if (hf[2]) { g_err = std::string(who) + ": the cell table found no slot"; return MVS_ERR_HIP; }
    if (tkeys.ensure(n_t) || tans.ensure(n_t) || tflag.ensure(n_t) || tbase.ensure(n_t + 1) || vflag.ensure(n_v) || vbase.ensure(n_v + 1) ||
        scan.ensure(std::max(n_v, n_t) / 256 + 4096))
        return MVS_ERR_HIP;
    mvsk_mdec_tkey1(n_t, d_tris.p, rep.p, tkeys.p, st);
    if (int r = mdec_fill(e, n_t, tkeys.p, tkey, tval, tans.p, flags.p + 2)) return r;
    mvsk_mdec_tkey2(n_t, d_tris.p, rep.p, tans.p, tkeys.p, st);
    if (int r = mdec_fill(e, n_t, tkeys.p, tkey, tval, tans.p, flags.p + 2)) return r;
    if (n_v > 0) HIPCHK(hipMemsetAsync(vflag.p, 0, (size_t)n_v * sizeof(int32_t), st));
    mvsk_mdec_keep(n_t, d_tris.p, rep.p, tans.p, tflag.p, vflag.p, st);
    int64_t nv = 0, nt = 0;
    if (int r = scan_total(e, vflag.p, vbase.p, scan.p, n_v, &nv)) return r;
    if (int r = scan_total(e, tflag.p, tbase.p, scan.p, n_t, &nt)) return r;
    if (int r = read_back(e, flags.p + 2, &hf[2])) return r;
    HIPCHK(hipGetLastError());
    if (hf[2]) { g_err = std::string(who) + ": the triangle table found no slot"; return MVS_ERR_HIP; }
    *n_v_out = nv; *n_t_out = nt;
    if ((out_verts && cap_v < nv) || (out_tris && cap_t < nt)) { g_err = std::string(who) + ": a cap is smaller than the decimated mesh (*n_v_out, *n_t_out)"; return MVS_ERR_CAPACITY; }
    if (!out_verts || !out_tris) return MVS_OK;
    if (acc.ensure(3 * n_v) || cnt.ensure(n_v) || (d->placement == 1 && best.ensure(n_v)) || d_out_verts.ensure(3 * nv) || d_out_tris.ensure(3 * nt)) return MVS_ERR_HIP;
    if (n_v > 0) {
        HIPCHK(hipMemsetAsync(acc.p, 0, (size_t)n_v * 3 * sizeof(long long), st));
        HIPCHK(hipMemsetAsync(cnt.p, 0, (size_t)n_v * sizeof(int32_t), st));
        if (d->placement == 1) HIPCHK(hipMemsetAsync(best.p, 0xff, (size_t)n_v * sizeof(unsigned long long), st));
    }
    mvsk_mdec_positions(d->placement, n_v, d_verts.p, rep.p, vflag.p, vbase.p, flags.p, acc.p, cnt.p, best.p, d_out_verts.p, nv, st);
    mvsk_mdec_gather(n_v, rep.p, vflag.p, vbase.p, used.p, n_t, d_tris.p, tflag.p, tbase.p, d_out_tris.p, nt, st);  // used becomes the vertex map
    HIPCHK(hipStreamSynchronize(st));  // a failure is known before anything is written
    HIPCHK(hipGetLastError());
    if (nv > 0) HIPCHK(hipMemcpyAsync(out_verts, d_out_verts.p, (size_t)nv * 3 * sizeof(float), hipMemcpyDefault, st));
    if (nt > 0) HIPCHK(hipMemcpyAsync(out_tris, d_out_tris.p, (size_t)nt * 3 * sizeof(int32_t), hipMemcpyDefault, st));
    if (vmap && n_v > 0) HIPCHK(hipMemcpyAsync(vmap, used.p, (size_t)n_v * sizeof(int32_t), hipMemcpyDefault, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    return MVS_OK;
}

// Mesh hole filling (mvs_mesh_fill.hip; the definitions are in mvskit_engine.h): the boundary loops and their centroid fans.  Stateless
// like the clean-up calls.  Both calls label the boundary components the same way; the filling goes on from there.
static_assert(sizeof(mvs_mesh_filling) == 8, "mvs_mesh_filling is 8 bytes");
namespace {
struct MfillBufs {
    DevBuf<int32_t> d_tris, tval, parent, outc, inc, cplx, next, hed, rbad, loop, length;
    DevBuf<uint32_t> words, flags;        // flags: [0] the bits of the centroids' largest component, [1] a loop vertex not finite, [2] a probe that ran out
    DevBuf<unsigned long long> tkey, counts;  // counts: [0] loops, [1] complex components, [2] irregular pairs, [3] filled loops
};
// the caller's triangles checked and labelled: b.loop, b.length, b.next and hc[0..2] (hc[3] = 0); the stream is idle on return
int mfill_label(mvs_engine* e, int64_t n_v, int64_t n_t, const int32_t* tris, MfillBufs& b, unsigned long long hc[4], const char* who) {
    hipStream_t st = e->stream;
    if (int r = mesh_take_tris(e, n_v, n_t, tris, b.d_tris, b.words, who)) return r;
    const int64_t slots = table_slots(3 * n_t);
    if (b.parent.ensure(n_v) || b.outc.ensure(n_v) || b.inc.ensure(n_v) || b.cplx.ensure(n_v) || b.next.ensure(n_v) || b.hed.ensure(n_v) || b.rbad.ensure(n_v) ||
        b.loop.ensure(n_v) || b.length.ensure(n_v) || b.flags.ensure(4) || b.counts.ensure(4) || (n_t > 0 && (b.tkey.ensure(slots) || b.tval.ensure(slots))))
        return MVS_ERR_HIP;
    for (DevBuf<int32_t>* z : {&b.outc, &b.inc, &b.cplx, &b.next, &b.hed, &b.rbad})
        if (n_v > 0) HIPCHK(hipMemsetAsync(z->p, 0, (size_t)n_v * sizeof(int32_t), st));
    HIPCHK(hipMemsetAsync(b.flags.p, 0, 4 * sizeof(uint32_t), st));
    HIPCHK(hipMemsetAsync(b.counts.p, 0, 4 * sizeof(unsigned long long), st));
    if (n_t > 0) if (int r = table_reset(e, b.tkey.p, b.tval.p, slots, 0)) return r;
    mvsk_mfill_boundaries(n_v, n_t, b.d_tris.p, b.tkey.p, b.tval.p, slots, b.parent.p, b.outc.p, b.inc.p, b.cplx.p, b.next.p, b.hed.p, b.rbad.p, b.loop.p,
                          b.length.p, b.counts.p, b.flags.p + 2, st);
    uint32_t fail = 0;
    HIPCHK(hipMemcpyAsync(hc, b.counts.p, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    if (int r = read_back(e, b.flags.p + 2, &fail)) return r;
    HIPCHK(hipGetLastError());
    if (fail) { g_err = std::string(who) + ": the edge table found no slot"; return MVS_ERR_HIP; }
    return MVS_OK;
}
}  // namespace

int mvs_engine_mesh_boundaries(mvs_engine* e, int64_t n_v, int64_t n_t, const int32_t* tris, int32_t* loop, int32_t* length, int64_t* n_loops, int64_t* n_complex,
                               int64_t* n_irregular) {
    const char* who = "mvs_engine_mesh_boundaries";
    if (int r = mesh_counts(n_v, n_t, who)) return r;
    if (!tris && n_t > 0) { g_err = std::string(who) + ": tris null"; return MVS_ERR_ARG; }
    if (int r = need_state(e, NEED_ENGINE, who)) return r;
    unsigned long long hc[4] = {0, 0, 0, 0};
    if (n_v > 0 || n_t > 0) {
        HIPCHK(hipSetDevice(e->cfg.device));
        Range rg("mvs:mesh_boundaries");
        hipStream_t st = e->stream;
        MfillBufs b;
        if (int r = mfill_label(e, n_v, n_t, tris, b, hc, who)) return r;  // a failure is known before anything is written
        if (loop && n_v > 0) HIPCHK(hipMemcpyAsync(loop, b.loop.p, (size_t)n_v * sizeof(int32_t), hipMemcpyDefault, st));
        if (length && n_v > 0) HIPCHK(hipMemcpyAsync(length, b.length.p, (size_t)n_v * sizeof(int32_t), hipMemcpyDefault, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    if (n_loops) *n_loops = (int64_t)hc[0];
    if (n_complex) *n_complex = (int64_t)hc[1];
    if (n_irregular) *n_irregular = (int64_t)hc[2];
    return MVS_OK;
}

void mvs_default_mesh_filling(mvs_mesh_filling* f) {
    if (!f) return;
    f->max_edges = 64; f->pad = 0;
}

int mvs_engine_mesh_fill(mvs_engine* e, const mvs_mesh_filling* f, int64_t n_v, const float* verts, int64_t n_t, const int32_t* tris, int64_t cap_v,
                         float* out_verts, int64_t cap_t, int32_t* out_tris, int64_t* n_v_out, int64_t* n_t_out, int64_t* n_filled) {
    const char* who = "mvs_engine_mesh_fill";
    if (!f) { g_err = std::string(who) + ": filling null"; return MVS_ERR_ARG; }
    if (f->max_edges < 3) { g_err = std::string(who) + ": max_edges < 3"; return MVS_ERR_ARG; }
    if (int r = mesh_in_args(n_v, verts, n_t, tris, who)) return r;
    if (int r = mesh_out_args(cap_v, cap_t, n_v_out, n_t_out, who)) return r;
    if (int r = need_state(e, NEED_ENGINE, who)) return r;
    if (n_v == 0 && n_t == 0) { *n_v_out = 0; *n_t_out = 0; if (n_filled) *n_filled = 0; return MVS_OK; }
    HIPCHK(hipSetDevice(e->cfg.device));
    Range rg("mvs:mesh_fill");
    hipStream_t st = e->stream;
    MfillBufs b;
    DevBuf<int32_t> tcnt, tbase, vcnt, vbase, scan, add_tris;
    DevBuf<float> d_verts, add_verts;
    DevBuf<long long> acc;
    unsigned long long hc[4] = {0, 0, 0, 0};
    if (int r = mfill_label(e, n_v, n_t, tris, b, hc, who)) return r;
    if (d_verts.ensure(3 * n_v) || tcnt.ensure(n_v) || tbase.ensure(n_v + 1) || vcnt.ensure(n_v) || vbase.ensure(n_v + 1) || scan.ensure(n_v / 256 + 4096)) return MVS_ERR_HIP;
    if (int r = upload_rows(e, d_verts.p, verts, n_v)) return r;
    mvsk_mfill_plan(n_v, d_verts.p, b.loop.p, b.length.p, f->max_edges, tcnt.p, vcnt.p, b.flags.p, b.flags.p + 1, b.counts.p + 3, st);
    int64_t nv_add = 0, nt_add = 0;
    if (int r = scan_total(e, tcnt.p, tbase.p, scan.p, n_v, &nt_add)) return r;
    if (int r = scan_total(e, vcnt.p, vbase.p, scan.p, n_v, &nv_add)) return r;
    uint32_t bad = 0;
    HIPCHK(hipMemcpyAsync(&hc[3], b.counts.p + 3, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    if (int r = read_back(e, b.flags.p + 1, &bad)) return r;
    HIPCHK(hipGetLastError());
    if (bad) { g_err = std::string(who) + ": a loop vertex with a non-finite component"; return MVS_ERR_ARG; }
    const int64_t nv = n_v + nv_add, nt = n_t + nt_add;
    if (nv > MESH_ATTR_MAX || nt > MESH_ATTR_MAX) { g_err = std::string(who) + ": the filled mesh has more than 2^30 vertices or triangles"; return MVS_ERR_CAPACITY; }
    *n_v_out = nv; *n_t_out = nt;
    if (n_filled) *n_filled = (int64_t)hc[3];
    if ((out_verts && cap_v < nv) || (out_tris && cap_t < nt)) { g_err = std::string(who) + ": a cap is smaller than the filled mesh (*n_v_out, *n_t_out)"; return MVS_ERR_CAPACITY; }
    if (!out_verts || !out_tris) return MVS_OK;
    if (nt_add > 0) {
        if (acc.ensure(3 * n_v) || add_tris.ensure(3 * nt_add) || add_verts.ensure(3 * nv_add)) return MVS_ERR_HIP;
        HIPCHK(hipMemsetAsync(acc.p, 0, (size_t)n_v * 3 * sizeof(long long), st));
        mvsk_mfill_emit(n_v, d_verts.p, b.loop.p, b.length.p, f->max_edges, b.next.p, tbase.p, vbase.p, b.flags.p, acc.p, add_tris.p, nt_add, add_verts.p, nv_add, st);
        HIPCHK(hipStreamSynchronize(st));  // a failure is known before anything is written
        HIPCHK(hipGetLastError());
    }
    if (n_v > 0) HIPCHK(hipMemcpyAsync(out_verts, d_verts.p, (size_t)n_v * 3 * sizeof(float), hipMemcpyDefault, st));
    if (n_t > 0) HIPCHK(hipMemcpyAsync(out_tris, b.d_tris.p, (size_t)n_t * 3 * sizeof(int32_t), hipMemcpyDefault, st));
    if (nv_add > 0) HIPCHK(hipMemcpyAsync(out_verts + 3 * n_v, add_verts.p, (size_t)nv_add * 3 * sizeof(float), hipMemcpyDefault, st));
    if (nt_add > 0) HIPCHK(hipMemcpyAsync(out_tris + 3 * n_t, add_tris.p, (size_t)nt_add * 3 * sizeof(int32_t), hipMemcpyDefault, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    return MVS_OK;
}

// Mesh render (mvs_mesh_render.hip; the definitions are in mvskit_engine.h): a z-buffer of the mesh in every view and the vertex
// visibility from it.  Stateless like the clean-up calls, but with views: they stream through one set of per-view buffers, as the maps do.
static_assert(sizeof(mvs_mesh_view_render) == 16, "mvs_mesh_view_render is 16 bytes");
namespace {
// the triangles a lane of k_mrender_small rasterises itself: a clipped box of at most this many pixel centres.  MVS_MRENDER_SMALL in the
// environment (mvskit_engine.h), read at every call, sets another value: the maps do not depend on it, mvs_engine_mesh_render_lists does
#define MRENDER_SMALL 32
int mrender_small_max() {
    const char* s = getenv("MVS_MRENDER_SMALL");
    const int v = s ? atoi(s) : 0;
    return v > 0 ? v : MRENDER_SMALL;
}
struct MrenderBufs {
    DevBuf<int32_t> d_tris, scr, list, tri;
    DevBuf<uint32_t> words, ok;
    DevBuf<float> d_verts, vd, depth;
    DevBuf<unsigned long long> keys, counts, visible;  // counts: a view's [0] listed triangles, [1] skipped triangles, [2] covered pixels
};
// the caller's mesh checked and on the device, the per-view buffers allocated; the stream is idle on return
int mrender_take(mvs_engine* e, int64_t n_v, const float* verts, int64_t n_t, const int32_t* tris, MrenderBufs& b, const char* who) {
    if (int r = mesh_take_tris(e, n_v, n_t, tris, b.d_tris, b.words, who)) return r;
    int64_t max_pix = 0;
    for (int v = 0; v < e->cfg.nviews; ++v) max_pix = std::max(max_pix, maps_npix(e, v));
    if (b.d_verts.ensure(3 * n_v) || b.scr.ensure(2 * n_v) || b.vd.ensure(n_v) || b.ok.ensure(n_v) || b.list.ensure(n_t) || b.keys.ensure(max_pix) ||
        b.depth.ensure(max_pix) || b.tri.ensure(max_pix) || b.counts.ensure(3 * (int64_t)MVS_MAXVIEWS))
        return MVS_ERR_HIP;
    if (int r = upload_rows(e, b.d_verts.p, verts, n_v)) return r;
    HIPCHK(hipMemsetAsync(b.counts.p, 0, 3 * (size_t)MVS_MAXVIEWS * sizeof(unsigned long long), e->stream));
    return MVS_OK;
}
// view v's vertices projected and its z-buffer filled: b.scr, b.vd, b.ok, b.keys and counts[3 v], counts[3 v + 1] (launched, not waited for)
int mrender_view(mvs_engine* e, const DParams& p, int v, int64_t n_v, int64_t n_t, int small_max, MrenderBufs& b) {
    hipStream_t st = e->stream;
    const int W = e->hviews[v].W[e->cfg.level], H = e->hviews[v].H[e->cfg.level];
    mvsk_mrender_project(p, v, n_v, b.d_verts.p, b.scr.p, b.vd.p, b.ok.p, st);
    HIPCHK(hipMemsetAsync(b.keys.p, 0xff, (size_t)W * H * sizeof(unsigned long long), st));
    mvsk_mrender_raster(n_t, b.d_tris.p, b.scr.p, b.vd.p, b.ok.p, W, H, small_max, b.keys.p, b.list.p, b.counts.p + 3 * v, st);
    return MVS_OK;
}
}  // namespace

int mvs_engine_mesh_render(mvs_engine* e, int64_t n_v, const float* verts, int64_t n_t, const int32_t* tris, mvs_mesh_view_render* out, int32_t* screen,
                           float* vdepth, int64_t* n_covered, int64_t* n_skipped) {
    const char* who = "mvs_engine_mesh_render";
    if (int r = mesh_in_args(n_v, verts, n_t, tris, who)) return r;
    if (int r = need_state(e, NEED_IDLE, who)) return r;
    HIPCHK(hipSetDevice(e->cfg.device));
    Range rg("mvs:mesh_render");
    hipStream_t st = e->stream;
    const int nviews = e->cfg.nviews, small_max = mrender_small_max();
    MrenderBufs b;
    if (int r = mrender_take(e, n_v, verts, n_t, tris, b, who)) return r;
    const DParams p = current_params(e);
    std::vector<unsigned long long> hc(3 * (size_t)nviews, 0ull);
    for (int v = 0; v < nviews; ++v) {
        const int64_t npix = maps_npix(e, v);
        const mvs_mesh_view_render o = out ? out[v] : mvs_mesh_view_render{nullptr, nullptr};
        if (int r = mrender_view(e, p, v, n_v, n_t, small_max, b)) return r;
        mvsk_mrender_resolve(npix, b.keys.p, o.depth ? b.depth.p : nullptr, o.tri ? b.tri.p : nullptr, b.counts.p + 3 * v + 2, st);
        if (o.depth) HIPCHK(hipMemcpyAsync(o.depth, b.depth.p, (size_t)npix * sizeof(float), hipMemcpyDefault, st));
        if (o.tri) HIPCHK(hipMemcpyAsync(o.tri, b.tri.p, (size_t)npix * sizeof(int32_t), hipMemcpyDefault, st));
        if (screen && n_v > 0) HIPCHK(hipMemcpyAsync(screen + 2 * n_v * v, b.scr.p, (size_t)n_v * 2 * sizeof(int32_t), hipMemcpyDefault, st));
        if (vdepth && n_v > 0) HIPCHK(hipMemcpyAsync(vdepth + n_v * v, b.vd.p, (size_t)n_v * sizeof(float), hipMemcpyDefault, st));
        HIPCHK(hipStreamSynchronize(st));  // the buffers are reused by the next view
        HIPCHK(hipGetLastError());
    }
    if (n_covered || n_skipped) {
        HIPCHK(hipMemcpyAsync(hc.data(), b.counts.p, hc.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        std::vector<int64_t> cov(nviews), skip(nviews);
        for (int v = 0; v < nviews; ++v) { skip[v] = (int64_t)hc[3 * v + 1]; cov[v] = (int64_t)hc[3 * v + 2]; }
        if (n_covered) HIPCHK(hipMemcpyAsync(n_covered, cov.data(), (size_t)nviews * sizeof(int64_t), hipMemcpyDefault, st));
        if (n_skipped) HIPCHK(hipMemcpyAsync(n_skipped, skip.data(), (size_t)nviews * sizeof(int64_t), hipMemcpyDefault, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    return MVS_OK;
}

int mvs_engine_mesh_render_lists(mvs_engine* e, int64_t n_v, const float* verts, int64_t n_t, const int32_t* tris, int64_t* n_listed) {
    const char* who = "mvs_engine_mesh_render_lists";
    if (int r = mesh_in_args(n_v, verts, n_t, tris, who)) return r;
    if (!n_listed) { g_err = std::string(who) + ": n_listed null"; return MVS_ERR_ARG; }
    if (int r = need_state(e, NEED_IDLE, who)) return r;
    HIPCHK(hipSetDevice(e->cfg.device));
    Range rg("mvs:mesh_render_lists");
    hipStream_t st = e->stream;
    const int nviews = e->cfg.nviews, small_max = mrender_small_max();
    MrenderBufs b;
    if (int r = mrender_take(e, n_v, verts, n_t, tris, b, who)) return r;
    const DParams p = current_params(e);
    for (int v = 0; v < nviews; ++v)
        if (int r = mrender_view(e, p, v, n_v, n_t, small_max, b)) return r;  // the views' counts are apart: no wait between them
    std::vector<unsigned long long> hc(3 * (size_t)nviews, 0ull);
    HIPCHK(hipMemcpyAsync(hc.data(), b.counts.p, hc.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));  // a failure is known before anything is written
    HIPCHK(hipGetLastError());
    std::vector<int64_t> listed(nviews);
    for (int v = 0; v < nviews; ++v) listed[v] = (int64_t)hc[3 * v];
    HIPCHK(hipMemcpyAsync(n_listed, listed.data(), (size_t)nviews * sizeof(int64_t), hipMemcpyDefault, st));
    HIPCHK(hipStreamSynchronize(st));
    return MVS_OK;
}

int mvs_engine_mesh_visibility(mvs_engine* e, float tol, int64_t n_v, const float* verts, int64_t n_t, const int32_t* tris, uint64_t* visible) {
    const char* who = "mvs_engine_mesh_visibility";
    if (!std::isfinite(tol) || !(tol >= 0.0f)) { g_err = std::string(who) + ": tol not finite or negative"; return MVS_ERR_ARG; }
    if (int r = mesh_in_args(n_v, verts, n_t, tris, who)) return r;
    if (!visible && n_v > 0) { g_err = std::string(who) + ": visible null"; return MVS_ERR_ARG; }
    if (int r = need_state(e, NEED_IDLE, who)) return r;
    HIPCHK(hipSetDevice(e->cfg.device));
    Range rg("mvs:mesh_visibility");
    hipStream_t st = e->stream;
    const int nviews = e->cfg.nviews, small_max = mrender_small_max();
    MrenderBufs b;
    if (int r = mrender_take(e, n_v, verts, n_t, tris, b, who)) return r;
    if (n_v == 0) return MVS_OK;
    if (b.visible.ensure(n_v)) return MVS_ERR_HIP;
    HIPCHK(hipMemsetAsync(b.visible.p, 0, (size_t)n_v * sizeof(unsigned long long), st));
    const DParams p = current_params(e);
    for (int v = 0; v < nviews; ++v) {
        if (int r = mrender_view(e, p, v, n_v, n_t, small_max, b)) return r;
        mvsk_mrender_visible(v, tol, n_v, b.scr.p, b.vd.p, b.ok.p, e->hviews[v].W[e->cfg.level], e->hviews[v].H[e->cfg.level], b.keys.p, b.visible.p, st);
    }
    HIPCHK(hipStreamSynchronize(st));  // a failure is known before anything is written
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(visible, b.visible.p, (size_t)n_v * sizeof(uint64_t), hipMemcpyDefault, st));
    HIPCHK(hipStreamSynchronize(st));
    return MVS_OK;
}

// Textured mesh (mvs_mesh_texture.hip; the definitions are in mvskit_engine.h): the view that textures each triangle, then the atlas and
// the texture coordinates.  Stateless like the render, and the views stream through the render's per-vertex buffers.
static_assert(sizeof(mvs_mesh_texturing) == 16, "mvs_mesh_texturing is 16 bytes");
namespace {
int mtex_args(const mvs_mesh_texturing* x, int64_t n_v, const float* verts, int64_t n_t, const int32_t* tris, const int32_t* label, const char* who) {
    if (!x) { g_err = std::string(who) + ": texturing null"; return MVS_ERR_ARG; }
    if (x->res < 1 || x->res > 256) { g_err = std::string(who) + ": res outside 1..256"; return MVS_ERR_ARG; }
    if (x->width < x->res + 3 || x->width > 32768) { g_err = std::string(who) + ": width outside res + 3 .. 32768"; return MVS_ERR_ARG; }
    if (int r = mesh_in_args(n_v, verts, n_t, tris, who)) return r;
    if (!label && n_t > 0) { g_err = std::string(who) + ": label null"; return MVS_ERR_ARG; }
    return MVS_OK;
}
struct MtexBufs {
    DevBuf<int32_t> d_tris, scr, label, win, flag, base, scan, list, uv;
    DevBuf<uint32_t> words, ok;
    DevBuf<float> d_verts, vd;
    DevBuf<long long> area;
    DevBuf<unsigned long long> visible, counts;
    DevBuf<uint8_t> rgb;
};
// the caller's mesh checked and on the device, the per-vertex buffers of a view allocated; the stream is idle on return
int mtex_take_mesh(mvs_engine* e, int64_t n_v, const float* verts, int64_t n_t, const int32_t* tris, MtexBufs& b, const char* who) {
    if (int r = mesh_take_tris(e, n_v, n_t, tris, b.d_tris, b.words, who)) return r;
    if (b.d_verts.ensure(3 * n_v) || b.scr.ensure(2 * n_v) || b.vd.ensure(n_v) || b.ok.ensure(n_v) || b.label.ensure(n_t)) return MVS_ERR_HIP;
    return upload_rows(e, b.d_verts.p, verts, n_v);
}
// f_v: the sign of a triangle's area in view v when its face vector points to the camera centre, -sign(det M) for P_L = [M | p]; 0 for a
// camera without an orientation
int mtex_front_sign(const mvs_engine* e, int v) {
    const float* P = e->hviews[v].P[e->cfg.level];
    const double a = P[0], b = P[1], c = P[2], d = P[4], f = P[5], g = P[6], h = P[8], i = P[9], j = P[10];
    const double det = a * (f * j - g * i) - b * (d * j - g * h) + c * (d * i - f * h);
    return det > 0.0 ? -1 : (det < 0.0 ? 1 : 0);
}
}  // namespace

void mvs_default_mesh_texturing(mvs_mesh_texturing* x) {
    if (!x) return;
    x->res = 8; x->width = 4096; x->front_only = 1; x->pad = 0;
}

int mvs_engine_mesh_face_views(mvs_engine* e, const mvs_mesh_texturing* x, int64_t n_v, const float* verts, int64_t n_t, const int32_t* tris,
                               const uint64_t* visible, int32_t* label, int64_t* area, int64_t* n_faces) {
    const char* who = "mvs_engine_mesh_face_views";
    if (int r = mtex_args(x, n_v, verts, n_t, tris, label, who)) return r;
    if (int r = need_state(e, NEED_IDLE, who)) return r;
    HIPCHK(hipSetDevice(e->cfg.device));
    Range rg("mvs:mesh_face_views");
    hipStream_t st = e->stream;
    const int nviews = e->cfg.nviews, level = e->cfg.level;
    MtexBufs b;
    if (int r = mtex_take_mesh(e, n_v, verts, n_t, tris, b, who)) return r;
    if (b.area.ensure(n_t) || b.counts.ensure(MVS_MAXVIEWS) || (visible && b.visible.ensure(n_v))) return MVS_ERR_HIP;
    if (visible && n_v > 0) HIPCHK(hipMemcpyAsync(b.visible.p, visible, (size_t)n_v * sizeof(uint64_t), hipMemcpyDefault, st));
    if (n_t > 0) {
        HIPCHK(hipMemsetAsync(b.area.p, 0, (size_t)n_t * sizeof(long long), st));
        HIPCHK(hipMemsetAsync(b.label.p, 0xff, (size_t)n_t * sizeof(int32_t), st));
    }
    HIPCHK(hipMemsetAsync(b.counts.p, 0, (size_t)MVS_MAXVIEWS * sizeof(unsigned long long), st));
    const DParams p = current_params(e);
    for (int v = 0; v < nviews; ++v) {  // one stream: a view's kernels run behind those of the view before, through the same buffers
        const int want = x->front_only ? mtex_front_sign(e, v) : 0;
        if (x->front_only && want == 0) continue;
        mvsk_mrender_project(p, v, n_v, b.d_verts.p, b.scr.p, b.vd.p, b.ok.p, st);
        mvsk_mtex_best(v, want, n_t, b.d_tris.p, b.scr.p, b.ok.p, visible ? b.visible.p : nullptr, e->hviews[v].W[level], e->hviews[v].H[level], b.area.p,
                       b.label.p, st);
    }
    mvsk_mtex_count(n_t, b.label.p, nviews, b.counts.p, st);
    std::vector<unsigned long long> hc((size_t)nviews, 0ull);
    HIPCHK(hipMemcpyAsync(hc.data(), b.counts.p, hc.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));  // a failure is known before anything is written
    HIPCHK(hipGetLastError());
    std::vector<int64_t> faces(hc.begin(), hc.end());
    if (n_t > 0) HIPCHK(hipMemcpyAsync(label, b.label.p, (size_t)n_t * sizeof(int32_t), hipMemcpyDefault, st));
    if (area && n_t > 0) HIPCHK(hipMemcpyAsync(area, b.area.p, (size_t)n_t * sizeof(int64_t), hipMemcpyDefault, st));
    if (n_faces) HIPCHK(hipMemcpyAsync(n_faces, faces.data(), (size_t)nviews * sizeof(int64_t), hipMemcpyDefault, st));
    HIPCHK(hipStreamSynchronize(st));
    return MVS_OK;
}

namespace {
// mvs_engine_mesh_texture, and with offset (host or device, or null) mvs_engine_mesh_texture_levelled
int mtex_texture(mvs_engine* e, const mvs_mesh_texturing* x, int64_t n_v, const float* verts, int64_t n_t, const int32_t* tris, const int32_t* label,
                 const int32_t* offset, int64_t cap_h, uint8_t* rgb, int32_t* uv, int64_t* height, int64_t* n_textured, const char* who) {
    if (int r = mtex_args(x, n_v, verts, n_t, tris, label, who)) return r;
    if (!height || !n_textured) { g_err = std::string(who) + ": height or n_textured null"; return MVS_ERR_ARG; }
    if (cap_h < 0) { g_err = std::string(who) + ": a negative cap_h"; return MVS_ERR_ARG; }
    if (int r = need_state(e, NEED_IDLE, who)) return r;
    HIPCHK(hipSetDevice(e->cfg.device));
    Range rg("mvs:mesh_texture");
    hipStream_t st = e->stream;
    const int nviews = e->cfg.nviews;
    MtexBufs b;
    if (int r = mtex_take_mesh(e, n_v, verts, n_t, tris, b, who)) return r;
    if (n_t > 0) HIPCHK(hipMemcpyAsync(b.label.p, label, (size_t)n_t * sizeof(int32_t), hipMemcpyDefault, st));
    mvsk_mtex_check_labels(n_t, b.label.p, nviews, b.words.p + 1, st);  // mesh_take_tris left both words zero
    uint32_t bad = 0;
    if (int r = read_back(e, b.words.p + 1, &bad)) return r;
    HIPCHK(hipGetLastError());
    if (bad) { g_err = std::string(who) + ": a label outside -1 .. nviews - 1"; return MVS_ERR_ARG; }
    if (b.win.ensure(9 * n_t) || b.flag.ensure(n_t) || b.base.ensure(n_t + 1) || b.scan.ensure(n_t / 256 + 4096)) return MVS_ERR_HIP;
    if (n_t > 0) HIPCHK(hipMemsetAsync(b.flag.p, 0, (size_t)n_t * sizeof(int32_t), st));
    const DParams p = current_params(e);
    for (int v = 0; v < nviews && n_t > 0; ++v) {
        mvsk_mrender_project(p, v, n_v, b.d_verts.p, b.scr.p, b.vd.p, b.ok.p, st);
        mvsk_mtex_take(v, n_t, b.d_tris.p, b.label.p, b.scr.p, b.vd.p, b.ok.p, b.win.p, b.flag.p, st);
    }
    int64_t nt = 0;
    if (int r = scan_total(e, b.flag.p, b.base.p, b.scan.p, n_t, &nt)) return r;
    const int64_t B = x->res + 3, cpr = x->width / B, n_cells = 1 + (nt + 1) / 2, h = (n_cells + cpr - 1) / cpr * B;
    *height = h; *n_textured = nt;
    if (h > 32768 || (int64_t)x->width * h > ((int64_t)1 << 30)) { g_err = std::string(who) + ": the atlas is higher than 32768 or holds more than 2^30 texels (*height)"; return MVS_ERR_CAPACITY; }
    if (!rgb) return MVS_OK;
    if (cap_h < h) { g_err = std::string(who) + ": cap_h is smaller than the atlas (*height)"; return MVS_ERR_CAPACITY; }
    const int64_t total = (int64_t)x->width * h;
    if (b.list.ensure(nt) || b.rgb.ensure((total + 3) / 4 * 12) || (uv && b.uv.ensure(6 * n_t))) return MVS_ERR_HIP;
    mvsk_mtex_layout(n_t, b.flag.p, b.base.p, b.list.p, nt, x->res, (int)cpr, uv ? b.uv.p : nullptr, st);
    if (offset) {
        DevBuf<int32_t>& d_off = b.scan;  // the scan is over
        if (d_off.ensure(3 * (int64_t)nviews)) return MVS_ERR_HIP;
        HIPCHK(hipMemcpyAsync(d_off.p, offset, 3 * (size_t)nviews * sizeof(int32_t), hipMemcpyDefault, st));
        mvsk_mtex_texels_levelled(p, x->res, x->width, h, nt, b.list.p, b.label.p, b.win.p, d_off.p, b.rgb.p, st);
    } else {
        mvsk_mtex_texels(p, x->res, x->width, h, nt, b.list.p, b.label.p, b.win.p, b.rgb.p, st);
    }
    HIPCHK(hipStreamSynchronize(st));  // a failure is known before anything is written
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(rgb, b.rgb.p, (size_t)total * 3, hipMemcpyDefault, st));
    if (uv && n_t > 0) HIPCHK(hipMemcpyAsync(uv, b.uv.p, (size_t)n_t * 6 * sizeof(int32_t), hipMemcpyDefault, st));
    HIPCHK(hipStreamSynchronize(st));
    return MVS_OK;
}
}  // namespace

int mvs_engine_mesh_texture(mvs_engine* e, const mvs_mesh_texturing* x, int64_t n_v, const float* verts, int64_t n_t, const int32_t* tris, const int32_t* label,
                            int64_t cap_h, uint8_t* rgb, int32_t* uv, int64_t* height, int64_t* n_textured) {
    return mtex_texture(e, x, n_v, verts, n_t, tris, label, nullptr, cap_h, rgb, uv, height, n_textured, "mvs_engine_mesh_texture");
}

// Seams of the textured mesh (mvs_mesh_seams.hip and, for what needs the gates or a view's texels, mvs_mesh_texture.hip; the contract is in
// include/mvskit_seams.h): the adjacency of triangles, the quality table, the smoothed labels, the levels on the seams and the levelled
// atlas.  Stateless like the texture calls.
static_assert(sizeof(mvs_mesh_seams) == 16, "mvs_mesh_seams is 16 bytes");
namespace {
int mseam_args(const mvs_mesh_seams* s, const char* who) {
    if (!s) { g_err = std::string(who) + ": seams null"; return MVS_ERR_ARG; }
    if (s->keep < 1 || s->keep > 255) { g_err = std::string(who) + ": keep outside 1..255"; return MVS_ERR_ARG; }
    if (s->iterations < 0 || s->iterations > 4096) { g_err = std::string(who) + ": iterations outside 0..4096"; return MVS_ERR_ARG; }
    if (s->max_shift < 0 || s->max_shift > 255) { g_err = std::string(who) + ": max_shift outside 0..255"; return MVS_ERR_ARG; }
    if (s->samples < 1 || s->samples > 16) { g_err = std::string(who) + ": samples outside 1..16"; return MVS_ERR_ARG; }
    return MVS_OK;
}
struct MseamBufs {
    DevBuf<int32_t> d_tris, tval, town, nbr;
    DevBuf<uint32_t> words;
    DevBuf<unsigned long long> tkey, counts;  // counts: [0] irregular edges, [1] seams before, [2] seams after, [3] seam edges
};
// nbr of the triangles in d_tris (checked ids) and counts zeroed, counts[0] the irregular edges when wanted; the stream is idle on return
int mseam_adjacency(mvs_engine* e, int64_t n_t, const int32_t* d_tris, MseamBufs& b, bool irregular, const char* who) {
    hipStream_t st = e->stream;
    const int64_t slots = table_slots(3 * n_t);
    if (b.counts.ensure(4) || b.words.ensure(2) || b.nbr.ensure(3 * n_t) || (n_t > 0 && (b.tkey.ensure(slots) || b.tval.ensure(slots) || b.town.ensure(slots))))
        return MVS_ERR_HIP;
    HIPCHK(hipMemsetAsync(b.counts.p, 0, 4 * sizeof(unsigned long long), st));
    HIPCHK(hipMemsetAsync(b.words.p, 0, 2 * sizeof(uint32_t), st));
    if (n_t > 0) if (int r = table_reset(e, b.tkey.p, b.tval.p, slots, 0)) return r;
    mvsk_mseam_adjacency(n_t, d_tris, b.tkey.p, b.tval.p, b.town.p, slots, b.nbr.p, irregular ? b.counts.p : nullptr, b.words.p, st);
    uint32_t fail = 0;
    if (int r = read_back(e, b.words.p, &fail)) return r;
    HIPCHK(hipGetLastError());
    if (fail) { g_err = std::string(who) + ": the edge table found no slot"; return MVS_ERR_HIP; }
    return MVS_OK;
}
// offset[v][ch] from the mirrored pair table: the header's OFFSETS, in its order of operations (this file is built without contraction)
void mseam_offsets(int n, const std::vector<int64_t>& pairs, int max_shift, std::vector<int32_t>& offset) {
    std::vector<double> A((size_t)n * n), rhs(n), g(n);
    const double lim = 16.0 * (double)max_shift;
    for (int ch = 0; ch < 3; ++ch) {
        for (int a = 0; a < n; ++a) {
            double diag = 1.0, s = 0.0;
            for (int b = 0; b < n; ++b) {
                if (b == a) continue;
                const int64_t* pr = &pairs[((size_t)a * n + b) * 4];
                diag = diag + (double)pr[0];
                s = s + (double)pr[1 + ch];
                A[(size_t)a * n + b] = -(double)pr[0];
            }
            A[(size_t)a * n + a] = diag;
            rhs[a] = -s;
        }
        for (int i = 0; i < n; ++i)
            for (int r = i + 1; r < n; ++r) {
                const double f = A[(size_t)r * n + i] / A[(size_t)i * n + i];
                for (int c = i; c < n; ++c) A[(size_t)r * n + c] = A[(size_t)r * n + c] - f * A[(size_t)i * n + c];
                rhs[r] = rhs[r] - f * rhs[i];
            }
        for (int i = n - 1; i >= 0; --i) {
            double s = rhs[i];
            for (int c = i + 1; c < n; ++c) s = s - A[(size_t)i * n + c] * g[c];
            g[i] = s / A[(size_t)i * n + i];
        }
        for (int a = 0; a < n; ++a) offset[(size_t)a * 3 + ch] = (int32_t)std::floor(std::fmin(std::fmax(g[a], -lim), lim) + 0.5);
    }
}
}  // namespace

void mvs_default_mesh_seams(mvs_mesh_seams* s) {
    if (!s) return;
    s->keep = 192; s->iterations = 64; s->max_shift = 32; s->samples = 4;
}

int mvs_engine_mesh_adjacency(mvs_engine* e, int64_t n_v, int64_t n_t, const int32_t* tris, int32_t* nbr, int64_t* n_irregular) {
    const char* who = "mvs_engine_mesh_adjacency";
    if (int r = mesh_counts(n_v, n_t, who)) return r;
    if (!tris && n_t > 0) { g_err = std::string(who) + ": tris null"; return MVS_ERR_ARG; }
    if (!nbr && n_t > 0) { g_err = std::string(who) + ": nbr null"; return MVS_ERR_ARG; }
    if (int r = need_state(e, NEED_ENGINE, who)) return r;
    unsigned long long nirr = 0;
    if (n_t > 0) {
        HIPCHK(hipSetDevice(e->cfg.device));
        Range rg("mvs:mesh_adjacency");
        hipStream_t st = e->stream;
        MseamBufs b;
        if (int r = mesh_take_tris(e, n_v, n_t, tris, b.d_tris, b.words, who)) return r;
        if (int r = mseam_adjacency(e, n_t, b.d_tris.p, b, n_irregular != nullptr, who)) return r;
        if (int r = read_back(e, b.counts.p, &nirr)) return r;  // a failure is known before anything is written
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(nbr, b.nbr.p, (size_t)n_t * 3 * sizeof(int32_t), hipMemcpyDefault, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    if (n_irregular) *n_irregular = (int64_t)nirr;
    return MVS_OK;
}

int mvs_engine_mesh_face_quality(mvs_engine* e, const mvs_mesh_texturing* x, int64_t n_v, const float* verts, int64_t n_t, const int32_t* tris,
                                 const uint64_t* visible, uint8_t* quality) {
    const char* who = "mvs_engine_mesh_face_quality";
    const int32_t no_label = -1;  // this call takes none
    if (int r = mtex_args(x, n_v, verts, n_t, tris, &no_label, who)) return r;
    if (!quality && n_t > 0) { g_err = std::string(who) + ": quality null"; return MVS_ERR_ARG; }
    if (int r = need_state(e, NEED_IDLE, who)) return r;
    HIPCHK(hipSetDevice(e->cfg.device));
    Range rg("mvs:mesh_face_quality");
    hipStream_t st = e->stream;
    const int nviews = e->cfg.nviews, level = e->cfg.level;
    MtexBufs b;
    if (int r = mtex_take_mesh(e, n_v, verts, n_t, tris, b, who)) return r;
    if (n_t == 0) return MVS_OK;
    if (b.area.ensure(n_t) || b.rgb.ensure(n_t * nviews) || (visible && b.visible.ensure(n_v))) return MVS_ERR_HIP;
    if (visible && n_v > 0) HIPCHK(hipMemcpyAsync(b.visible.p, visible, (size_t)n_v * sizeof(uint64_t), hipMemcpyDefault, st));
    HIPCHK(hipMemsetAsync(b.area.p, 0, (size_t)n_t * sizeof(long long), st));
    HIPCHK(hipMemsetAsync(b.label.p, 0xff, (size_t)n_t * sizeof(int32_t), st));
    HIPCHK(hipMemsetAsync(b.rgb.p, 0, (size_t)n_t * nviews, st));
    const DParams p = current_params(e);
    for (int pass = 0; pass < 2; ++pass)  // the best |area| over all views, then every view against it
        for (int v = 0; v < nviews; ++v) {
            const int want = x->front_only ? mtex_front_sign(e, v) : 0;
            if (x->front_only && want == 0) continue;
            const int W = e->hviews[v].W[level], H = e->hviews[v].H[level];
            mvsk_mrender_project(p, v, n_v, b.d_verts.p, b.scr.p, b.vd.p, b.ok.p, st);
            if (pass == 0) mvsk_mtex_best(v, want, n_t, b.d_tris.p, b.scr.p, b.ok.p, visible ? b.visible.p : nullptr, W, H, b.area.p, b.label.p, st);
            else mvsk_mtex_quality(v, want, n_t, b.d_tris.p, b.scr.p, b.ok.p, visible ? b.visible.p : nullptr, W, H, b.area.p, nviews, b.rgb.p, st);
        }
    HIPCHK(hipStreamSynchronize(st));  // a failure is known before anything is written
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(quality, b.rgb.p, (size_t)n_t * nviews, hipMemcpyDefault, st));
    HIPCHK(hipStreamSynchronize(st));
    return MVS_OK;
}

int mvs_engine_mesh_smooth_labels(mvs_engine* e, const mvs_mesh_seams* s, int64_t n_v, int64_t n_t, const int32_t* tris, int nviews_q, const uint8_t* quality,
                                  const int32_t* label_in, int32_t* label_out, int64_t* stats) {
    const char* who = "mvs_engine_mesh_smooth_labels";
    if (int r = mseam_args(s, who)) return r;
    if (int r = mesh_counts(n_v, n_t, who)) return r;
    if (!tris && n_t > 0) { g_err = std::string(who) + ": tris null"; return MVS_ERR_ARG; }
    if (nviews_q < 1 || nviews_q > MVS_MAXVIEWS) { g_err = std::string(who) + ": nviews_q outside 1..64"; return MVS_ERR_ARG; }
    if (!quality && n_t > 0) { g_err = std::string(who) + ": quality null"; return MVS_ERR_ARG; }
    if (!label_in && n_t > 0) { g_err = std::string(who) + ": label_in null"; return MVS_ERR_ARG; }
    if (!label_out && n_t > 0) { g_err = std::string(who) + ": label_out null"; return MVS_ERR_ARG; }
    if (!stats) { g_err = std::string(who) + ": stats null"; return MVS_ERR_ARG; }
    if (int r = need_state(e, NEED_ENGINE, who)) return r;
    int64_t hs[4] = {0, 0, 0, 0};
    HIPCHK(hipSetDevice(e->cfg.device));
    if (n_t > 0) {
        Range rg("mvs:mesh_smooth_labels");
        hipStream_t st = e->stream;
        MseamBufs b;
        DevBuf<int32_t> label, prop, score;
        DevBuf<uint8_t> d_quality;
        DevBuf<unsigned long long> moved;
        const int iters = s->iterations;
        if (int r = mesh_take_tris(e, n_v, n_t, tris, b.d_tris, b.words, who)) return r;
        if (label.ensure(n_t) || prop.ensure(n_t) || score.ensure(n_t) || d_quality.ensure(n_t * nviews_q) || moved.ensure(iters + 1)) return MVS_ERR_HIP;
        HIPCHK(hipMemcpyAsync(label.p, label_in, (size_t)n_t * sizeof(int32_t), hipMemcpyDefault, st));
        mvsk_mtex_check_labels(n_t, label.p, nviews_q, b.words.p + 1, st);  // mesh_take_tris left both words zero
        uint32_t bad = 0;
        if (int r = read_back(e, b.words.p + 1, &bad)) return r;
        HIPCHK(hipGetLastError());
        if (bad) { g_err = std::string(who) + ": a label outside -1 .. nviews_q - 1"; return MVS_ERR_ARG; }
        if (int r = mseam_adjacency(e, n_t, b.d_tris.p, b, false, who)) return r;
        HIPCHK(hipMemcpyAsync(d_quality.p, quality, (size_t)n_t * nviews_q, hipMemcpyDefault, st));
        HIPCHK(hipMemsetAsync(moved.p, 0, (size_t)(iters + 1) * sizeof(unsigned long long), st));
        mvsk_mseam_count(n_t, b.nbr.p, label.p, b.counts.p + 1, st);
        std::vector<unsigned long long> hm((size_t)iters + 1, 0ull);
        for (int it = 0; it < iters; ++it) {
            mvsk_mseam_iteration(it, moved.p, n_t, b.d_tris.p, b.nbr.p, nviews_q, d_quality.p, s->keep, prop.p, score.p, label.p, st);
            if (it % 8 == 7) {  // a look every eight iterations: the launches behind a still iteration do nothing anyway
                if (int r = read_back(e, moved.p + it, &hm[it])) return r;
                if (hm[it] == 0ull) break;
            }
        }
        mvsk_mseam_count(n_t, b.nbr.p, label.p, b.counts.p + 2, st);
        unsigned long long hc[4] = {0, 0, 0, 0};
        HIPCHK(hipMemcpyAsync(hm.data(), moved.p, hm.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(hc, b.counts.p, sizeof(hc), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));  // a failure is known before anything is written
        HIPCHK(hipGetLastError());
        hs[0] = (int64_t)hc[1]; hs[1] = (int64_t)hc[2];
        for (int it = 0; it < iters; ++it) { hs[2] += (int64_t)hm[it]; hs[3] += hm[it] != 0ull ? 1 : 0; }
        HIPCHK(hipMemcpyAsync(label_out, label.p, (size_t)n_t * sizeof(int32_t), hipMemcpyDefault, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    HIPCHK(hipMemcpy(stats, hs, sizeof(hs), hipMemcpyDefault));
    return MVS_OK;
}

int mvs_engine_mesh_seam_levels(mvs_engine* e, const mvs_mesh_seams* s, const mvs_mesh_texturing* x, int64_t n_v, const float* verts, int64_t n_t,
                                const int32_t* tris, const int32_t* label, int32_t* offset, int64_t* pairs, int64_t* n_seam_edges) {
    const char* who = "mvs_engine_mesh_seam_levels";
    if (!s) { g_err = std::string(who) + ": seams null"; return MVS_ERR_ARG; }
    if (!x) { g_err = std::string(who) + ": texturing null"; return MVS_ERR_ARG; }
    if (int r = mseam_args(s, who)) return r;
    if (int r = mtex_args(x, n_v, verts, n_t, tris, label, who)) return r;
    if (!offset) { g_err = std::string(who) + ": offset null"; return MVS_ERR_ARG; }
    if (!pairs) { g_err = std::string(who) + ": pairs null"; return MVS_ERR_ARG; }
    if (int r = need_state(e, NEED_IDLE, who)) return r;
    HIPCHK(hipSetDevice(e->cfg.device));
    Range rg("mvs:mesh_seam_levels");
    hipStream_t st = e->stream;
    const int nviews = e->cfg.nviews;
    MtexBufs b;
    MseamBufs m;
    DevBuf<long long> d_pairs;
    std::vector<int64_t> hp((size_t)nviews * nviews * 4, 0);
    unsigned long long nedges = 0;
    if (int r = mtex_take_mesh(e, n_v, verts, n_t, tris, b, who)) return r;
    if (n_t > 0) {
        HIPCHK(hipMemcpyAsync(b.label.p, label, (size_t)n_t * sizeof(int32_t), hipMemcpyDefault, st));
        mvsk_mtex_check_labels(n_t, b.label.p, nviews, b.words.p + 1, st);  // mesh_take_tris left both words zero
        uint32_t bad = 0;
        if (int r = read_back(e, b.words.p + 1, &bad)) return r;
        HIPCHK(hipGetLastError());
        if (bad) { g_err = std::string(who) + ": a label outside -1 .. nviews - 1"; return MVS_ERR_ARG; }
        if (b.win.ensure(9 * n_t) || b.flag.ensure(n_t) || d_pairs.ensure((int64_t)hp.size())) return MVS_ERR_HIP;
        if (int r = mseam_adjacency(e, n_t, b.d_tris.p, m, false, who)) return r;
        HIPCHK(hipMemsetAsync(b.flag.p, 0, (size_t)n_t * sizeof(int32_t), st));
        HIPCHK(hipMemsetAsync(d_pairs.p, 0, hp.size() * sizeof(long long), st));
        const DParams p = current_params(e);
        for (int v = 0; v < nviews; ++v) {
            mvsk_mrender_project(p, v, n_v, b.d_verts.p, b.scr.p, b.vd.p, b.ok.p, st);
            mvsk_mtex_take(v, n_t, b.d_tris.p, b.label.p, b.scr.p, b.vd.p, b.ok.p, b.win.p, b.flag.p, st);
        }
        mvsk_mtex_seam_samples(p, nviews, s->samples, n_t, b.d_tris.p, m.nbr.p, b.label.p, b.flag.p, b.win.p, d_pairs.p, m.counts.p + 3, st);
        HIPCHK(hipMemcpyAsync(hp.data(), d_pairs.p, hp.size() * sizeof(long long), hipMemcpyDeviceToHost, st));
        if (int r = read_back(e, m.counts.p + 3, &nedges)) return r;  // a failure is known before anything is written
        HIPCHK(hipGetLastError());
    }
    for (int a = 0; a < nviews; ++a)  // the device filled [min][max]: the mirror
        for (int c = a + 1; c < nviews; ++c) {
            const int64_t* up = &hp[((size_t)a * nviews + c) * 4];
            int64_t* lo = &hp[((size_t)c * nviews + a) * 4];
            lo[0] = up[0]; lo[1] = -up[1]; lo[2] = -up[2]; lo[3] = -up[3];
        }
    std::vector<int32_t> ho((size_t)nviews * 3, 0);
    mseam_offsets(nviews, hp, s->max_shift, ho);
    HIPCHK(hipMemcpyAsync(offset, ho.data(), ho.size() * sizeof(int32_t), hipMemcpyDefault, st));
    HIPCHK(hipMemcpyAsync(pairs, hp.data(), hp.size() * sizeof(int64_t), hipMemcpyDefault, st));
    HIPCHK(hipStreamSynchronize(st));
    if (n_seam_edges) *n_seam_edges = (int64_t)nedges;
    return MVS_OK;
}

int mvs_engine_mesh_texture_levelled(mvs_engine* e, const mvs_mesh_texturing* x, int64_t n_v, const float* verts, int64_t n_t, const int32_t* tris,
                                     const int32_t* label, const int32_t* offset, int64_t cap_h, uint8_t* rgb, int32_t* uv, int64_t* height, int64_t* n_textured) {
    return mtex_texture(e, x, n_v, verts, n_t, tris, label, offset, cap_h, rgb, uv, height, n_textured, "mvs_engine_mesh_texture_levelled");
}
}  // extern "C"
