// mvs_engine_output.cpp -- what the C ABI in include/mvskit_engine.h makes of the finished pool: the PLY point cloud (mvs_ply.hip) and
// the dense per-view maps and their fusion (mvs_maps.hip).  The mesh calls, which start from the same maps (render_all, render_usable),
// are in mvs_engine_mesh.cpp.  Every entry point is stateless: its working arrays live in buffers of the call, and nothing of the
// engine's state changes.
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "mvs_engine_impl.h"

using namespace mvseng;

extern "C" {

// PatchManager::writePly (patch_manager.cpp:542-633) of the alive pool, on the device (mvs_ply.hip).  The pool is walked in chunks of
// PLY_CHUNK slots, each through fixed buffers (~110 MB: the pool indices, colours, line lengths and offsets and at most 90 bytes of text
// per slot), and every chunk is copied into `out` as soon as it is formatted.  Nothing of the engine's state changes: kill_cnt /
// kill_base are scratch that every user fills first (count_pool), the scan's block sums go to scan_tmp.
#define PLY_CHUNK ((int64_t)1 << 20)
#define PLY_ASCII_LINE_MAX 90  // mvs_plyfmt.h: six numbers of at most 12 characters, three of 3, 8 blanks and the newline
static void ply_header(int64_t n, bool ascii, std::string* out) {
    char head[512];
    snprintf(head, sizeof head,
             "ply\nformat %s 1.0\nelement vertex %lld\nproperty float x\nproperty float y\nproperty float z\nproperty float nx\n"
             "property float ny\nproperty float nz\nproperty uchar diffuse_red\nproperty uchar diffuse_green\nproperty uchar diffuse_blue\n"
             "end_header\n",
             ascii ? "ascii" : "binary_little_endian", (long long)n);
    *out = head;
}
namespace {
struct PlyBufs {
    DevBuf<int32_t> idx, len;
    DevBuf<int64_t> off;
    DevBuf<uint32_t> rgb;
    DevBuf<uint8_t> bytes;
};
}  // namespace

int mvs_engine_export_ply(mvs_engine* e, int format, int64_t cap, uint8_t* out, int64_t* nbytes) {
    // the arguments first, the handle after them
    if (format != MVS_PLY_ASCII && format != MVS_PLY_BINARY_LE) { g_err = "mvs_engine_export_ply: format must be MVS_PLY_ASCII or MVS_PLY_BINARY_LE"; return MVS_ERR_ARG; }
    if (!nbytes || cap < 0) { g_err = "mvs_engine_export_ply: nbytes is null or cap negative"; return MVS_ERR_ARG; }
    if (int r = need_state(e, NEED_IDLE, "mvs_engine_export_ply")) return r;
    HIPCHK(hipSetDevice(e->cfg.device));
    Range rg("mvs:export_ply");
    hipStream_t st = e->stream;
    const bool ascii = format == MVS_PLY_ASCII;
    int64_t alive = 0;
    if (int r = mvs_engine_num_patches(e, &alive)) return r;  // count_pool: kill_base = the scan of the alive flags
    std::string head;
    ply_header(alive, ascii, &head);
    const int64_t chunk = std::min<int64_t>(PLY_CHUNK, std::max<int64_t>(e->pool_n, 1));
    PlyBufs b;
    if (alive > 0 && (b.idx.ensure(chunk) || b.rgb.ensure(chunk) || (ascii && (b.len.ensure(chunk + 1) || b.off.ensure(chunk + 1))))) return MVS_ERR_HIP;
    // one chunk of pool slots [i0, i1): its nv alive vertices listed, coloured and (ASCII) measured; *cb = the chunk's bytes
    auto measure = [&](int64_t i0, int64_t i1, int64_t* nv, int64_t* cb) -> int {
        int32_t ends[2] = {0, 0};
        HIPCHK(hipMemcpyAsync(&ends[0], e->kill_base.p + i0, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(&ends[1], e->kill_base.p + i1, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        *nv = ends[1] - ends[0];
        *cb = 27 * *nv;
        if (*nv == 0) return MVS_OK;
        mvsk_ply_select(e->pool.p, e->kill_base.p, i0, i1, b.idx.p, st);
        mvsk_ply_colour(e->pool.p, b.idx.p, *nv, e->dviews.p, e->cfg.nviews, e->cfg.level, ascii ? 1 : 0, b.rgb.p, b.len.p, st);
        if (!ascii) return MVS_OK;
        mvsk_exclusive_scan_off(b.len.p, b.off.p, *nv, reinterpret_cast<csr_off_t*>(e->scan_tmp.p), st);
        return read_back(e, b.off.p + *nv, cb);
    };
    // the size: header + 27 bytes a vertex, or (ASCII) one length pass -- skipped when `out` holds the longest file N vertices can make
    const int64_t upper = (int64_t)head.size() + (ascii ? PLY_ASCII_LINE_MAX : 27) * alive;
    if (!out || cap < upper) {
        int64_t total = (int64_t)head.size() + 27 * alive;
        if (ascii) {
            total = (int64_t)head.size();
            for (int64_t i0 = 0; i0 < e->pool_n; i0 += chunk) {
                int64_t nv = 0, cb = 0;
                if (int r = measure(i0, std::min(e->pool_n, i0 + chunk), &nv, &cb)) return r;
                total += cb;
            }
        }
        *nbytes = total;
        if (!out) return MVS_OK;
        if (cap < total) { g_err = "mvs_engine_export_ply: cap is smaller than the file (*nbytes)"; return MVS_ERR_CAPACITY; }
    }
    if (alive > 0 && b.bytes.ensure(chunk * (ascii ? PLY_ASCII_LINE_MAX : 27))) return MVS_ERR_HIP;
    memcpy(out, head.data(), head.size());
    int64_t pos = (int64_t)head.size();
    for (int64_t i0 = 0; i0 < e->pool_n; i0 += chunk) {
        int64_t nv = 0, cb = 0;
        if (int r = measure(i0, std::min(e->pool_n, i0 + chunk), &nv, &cb)) return r;
        if (nv == 0) continue;
        if (pos + cb > cap || cb > b.bytes.cap) { g_err = "mvs_engine_export_ply: a chunk outgrew its bound"; return MVS_ERR_CAPACITY; }
        mvsk_ply_emit(e->pool.p, b.idx.p, nv, b.rgb.p, ascii ? b.off.p : nullptr, b.bytes.p, st);
        HIPCHK(hipMemcpyAsync(out + pos, b.bytes.p, (size_t)cb, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        pos += cb;
    }
    *nbytes = pos;
    return MVS_OK;
}

}  // extern "C"

// Dense per-view maps and their fusion (mvs_maps.hip; the definitions are in mvskit_engine.h).  Both entry points are stateless: render_all
// fills the id and the point of every pixel of every view, the views then stream one at a time through buffers sized for the largest.
// The selection keys go where mvs_engine_depth_normal_map puts them: `best` (source 0; scratch that every user clears first, sized for
// the cells of all views) or `dpgrid` (source 1; every pass and Filter::run rebuilds it).
static_assert(sizeof(mvs_maps_config) == 24 && sizeof(mvs_view_maps) == 40 && sizeof(mvs_fused_point) == 32, "the maps structs are 24, 40 and 32 bytes");
namespace mvseng {
int maps_args(const mvs_maps_config* c, const char* who) {
    if (!c) { g_err = std::string(who) + ": config null"; return MVS_ERR_ARG; }
    if (c->source < 0 || c->source > 1) { g_err = std::string(who) + ": source must be 0 or 1"; return MVS_ERR_ARG; }
    if (c->min_consistent < 0) { g_err = std::string(who) + ": min_consistent negative"; return MVS_ERR_ARG; }
    if (!std::isfinite(c->depth_tol) || !(c->depth_tol > 0.0f)) { g_err = std::string(who) + ": depth_tol not finite or <= 0"; return MVS_ERR_ARG; }
    if (!std::isfinite(c->normal_cos) || !(c->normal_cos <= 1.0f)) { g_err = std::string(who) + ": normal_cos not finite or > 1"; return MVS_ERR_ARG; }
    return MVS_OK;
}
// The checks of the five maps-based entry points that need the handle, behind maps_args and the entry point's own argument checks:
// a handle, min_consistent against its views, then views and no pass waiting for its commit
int maps_state(const mvs_engine* e, const mvs_maps_config* c, const char* who) {
    if (int r = need_state(e, NEED_ENGINE, who)) return r;
    if (c->min_consistent > e->cfg.nviews - 1) { g_err = std::string(who) + ": min_consistent exceeds the number of other views"; return MVS_ERR_ARG; }
    return need_state(e, NEED_IDLE, who);
}
int64_t maps_npix(const mvs_engine* e, int v) { return (int64_t)e->hviews[v].W[e->cfg.level] * e->hviews[v].H[e->cfg.level]; }

// steps 1 and 2 for every view: b.ids and b.pts
int render_all(mvs_engine* e, const mvs_maps_config* c, MapsBufs& b) {
    hipStream_t st = e->stream;
    const int nviews = e->cfg.nviews;
    b.total_pix = b.max_pix = 0;
    for (int v = 0; v < nviews; ++v) {
        b.args.pix_base[v] = b.total_pix;
        b.total_pix += maps_npix(e, v);
        b.max_pix = std::max(b.max_pix, maps_npix(e, v));
    }
    for (int v = nviews; v <= MVS_MAXVIEWS; ++v) b.args.pix_base[v] = b.total_pix;
    b.args.depth_tol = c->depth_tol; b.args.normal_cos = c->normal_cos;
    if (b.max_pix > (int64_t)INT32_MAX - 4096) { g_err = "maps: a view of more than 2^31 - 4097 pixels"; return MVS_ERR_ARG; }
    if (b.ids.ensure(b.total_pix) || b.pts.ensure(3 * b.total_pix) || b.flag.ensure(b.max_pix + 1) || b.base.ensure(b.max_pix + 1) ||
        b.scan.ensure(b.max_pix / 256 + 4096))
        return MVS_ERR_HIP;
    const unsigned long long* sel = nullptr;
    if (c->source == 1) {
        if (int r = build_depth(e)) return r;
        sel = e->dpgrid.p;
    } else {
        HIPCHK(hipMemsetAsync(e->best.p, 0, (size_t)e->total_cells * sizeof(unsigned long long), st));
        mvsk_maps_select(current_params(e), e->best.p, st);
        sel = e->best.p;
    }
    const DParams p = current_params(e);
    for (int v = 0; v < nviews; ++v)
        mvsk_maps_render(p, v, e->hviews[v].W[e->cfg.level], e->hviews[v].H[e->cfg.level], c->source, sel, b.ids.p + b.args.pix_base[v],
                         b.pts.p + 3 * b.args.pix_base[v], st);
    HIPCHK(hipGetLastError());
    return MVS_OK;
}

// the maps and their usability into b: b.ids and, a byte per pixel of all views, b.flag8 (launched, not waited for)
int render_usable(mvs_engine* e, const mvs_maps_config* c, MapsBufs& b) {
    hipStream_t st = e->stream;
    if (int r = render_all(e, c, b)) return r;
    if (b.agree.ensure(b.max_pix) || b.flag8.ensure(b.total_pix)) return MVS_ERR_HIP;
    const DParams p = current_params(e);
    // usability: fused_points' counting pass without dedupe, kept as a byte per pixel of all views (the views follow each other in stream order)
    for (int v = 0; v < e->cfg.nviews; ++v) {
        const int64_t npix = maps_npix(e, v), pix0 = b.args.pix_base[v];
        mvsk_maps_agree(p, b.args, v, npix, b.ids.p, b.pts.p, b.agree.p, nullptr, nullptr, nullptr, st);
        mvsk_maps_flag(npix, v, b.ids.p + pix0, b.agree.p, c->min_consistent, 0, b.flag.p, b.flag8.p + pix0, st);
    }
    return MVS_OK;
}
}  // namespace mvseng

extern "C" {

void mvs_default_maps_config(mvs_maps_config* c) {
    if (!c) return;
    c->source = 0; c->min_consistent = 1; c->depth_tol = 0.01f; c->normal_cos = 0.9f; c->dedupe = 1; c->pad = 0;
}

int mvs_engine_render_maps(mvs_engine* e, const mvs_maps_config* c, mvs_view_maps* out, int64_t* n_valid) {
    const char* who = "mvs_engine_render_maps";
    if (int r = maps_args(c, who)) return r;
    if (int r = maps_state(e, c, who)) return r;
    HIPCHK(hipSetDevice(e->cfg.device));
    Range rg("mvs:render_maps");
    hipStream_t st = e->stream;
    MapsBufs b;
    if (int r = render_all(e, c, b)) return r;
    const DParams p = current_params(e);
    for (int v = 0; v < e->cfg.nviews; ++v) {
        const int64_t npix = maps_npix(e, v), pix0 = b.args.pix_base[v];
        const mvs_view_maps o = out ? out[v] : mvs_view_maps{nullptr, nullptr, nullptr, nullptr, nullptr};
        if (o.depth || o.normal || o.conf || o.agree) {
            if ((o.agree && b.agree.ensure(b.max_pix)) || b.maps.ensure(5 * b.max_pix)) return MVS_ERR_HIP;
            float* d_depth = b.maps.p, *d_normal = b.maps.p + b.max_pix, *d_conf = b.maps.p + 4 * b.max_pix;
            mvsk_maps_agree(p, b.args, v, npix, b.ids.p, b.pts.p, o.agree ? b.agree.p : nullptr, o.depth ? d_depth : nullptr,
                            o.normal ? d_normal : nullptr, o.conf ? d_conf : nullptr, st);
            if (o.depth) HIPCHK(hipMemcpyAsync(o.depth, d_depth, (size_t)npix * sizeof(float), hipMemcpyDefault, st));
            if (o.normal) HIPCHK(hipMemcpyAsync(o.normal, d_normal, (size_t)npix * 3 * sizeof(float), hipMemcpyDefault, st));
            if (o.conf) HIPCHK(hipMemcpyAsync(o.conf, d_conf, (size_t)npix * sizeof(float), hipMemcpyDefault, st));
            if (o.agree) HIPCHK(hipMemcpyAsync(o.agree, b.agree.p, (size_t)npix * sizeof(uint64_t), hipMemcpyDefault, st));
        }
        if (o.ids) HIPCHK(hipMemcpyAsync(o.ids, b.ids.p + pix0, (size_t)npix * sizeof(int32_t), hipMemcpyDefault, st));
        if (n_valid) {
            mvsk_maps_flag(npix, v, b.ids.p + pix0, nullptr, 0, 0, b.flag.p, nullptr, st);
            if (int r = scan_total(e, b.flag.p, b.base.p, b.scan.p, npix, &n_valid[v])) return r;
        }
        HIPCHK(hipStreamSynchronize(st));  // the buffers are reused by the next view
        HIPCHK(hipGetLastError());
    }
    return MVS_OK;
}

int mvs_engine_fused_points(mvs_engine* e, const mvs_maps_config* c, int64_t cap, mvs_fused_point* out, int64_t* n) {
    const char* who = "mvs_engine_fused_points";
    if (int r = maps_args(c, who)) return r;
    if (cap < 0 || !n) { g_err = std::string(who) + ": cap negative or n null"; return MVS_ERR_ARG; }
    if (int r = maps_state(e, c, who)) return r;
    HIPCHK(hipSetDevice(e->cfg.device));
    Range rg("mvs:fused_points");
    hipStream_t st = e->stream;
    const int nviews = e->cfg.nviews;
    MapsBufs b;
    if (int r = render_all(e, c, b)) return r;
    if (b.agree.ensure(b.max_pix) || (out && b.flag8.ensure(b.total_pix))) return MVS_ERR_HIP;
    const DParams p = current_params(e);
    // the counting pass: per view the agree words, the flags (kept as bytes for the gathering pass) and their number
    std::vector<int64_t> count((size_t)nviews, 0);
    int64_t total = 0, most = 0;
    for (int v = 0; v < nviews; ++v) {
        const int64_t npix = maps_npix(e, v), pix0 = b.args.pix_base[v];
        mvsk_maps_agree(p, b.args, v, npix, b.ids.p, b.pts.p, b.agree.p, nullptr, nullptr, nullptr, st);
        mvsk_maps_flag(npix, v, b.ids.p + pix0, b.agree.p, c->min_consistent, c->dedupe, b.flag.p, out ? b.flag8.p + pix0 : nullptr, st);
        if (int r = scan_total(e, b.flag.p, b.base.p, b.scan.p, npix, &count[(size_t)v])) return r;
        total += count[(size_t)v];
        most = std::max(most, count[(size_t)v]);
    }
    if (!out) { *n = total; return MVS_OK; }
    if (cap < total) { *n = total; g_err = std::string(who) + ": cap is smaller than the number of points (*n)"; return MVS_ERR_CAPACITY; }
    // the gathering pass: the records of a view behind the scan of its flags, copied behind those of the views before it
    if (most > 0 && b.recs.ensure(most)) return MVS_ERR_HIP;
    int64_t pos = 0;
    for (int v = 0; v < nviews; ++v) {
        const int64_t npix = maps_npix(e, v), pix0 = b.args.pix_base[v], nv = count[(size_t)v];
        if (nv == 0) continue;
        mvsk_maps_expand(npix, b.flag8.p + pix0, b.flag.p, st);
        int64_t again = 0;
        if (int r = scan_total(e, b.flag.p, b.base.p, b.scan.p, npix, &again)) return r;
        if (again != nv) { g_err = std::string(who) + ": the two passes disagree"; return MVS_ERR_HIP; }
        mvsk_maps_gather(p, v, npix, b.ids.p + pix0, b.pts.p + 3 * pix0, b.flag.p, b.base.p, b.recs.p, nv, st);
        HIPCHK(hipMemcpyAsync(out + pos, b.recs.p, (size_t)nv * sizeof(mvs_fused_point), hipMemcpyDefault, st));
        HIPCHK(hipStreamSynchronize(st));  // the buffers are reused by the next view
        HIPCHK(hipGetLastError());
        pos += nv;
    }
    *n = total;
    return MVS_OK;
}

}  // extern "C"
