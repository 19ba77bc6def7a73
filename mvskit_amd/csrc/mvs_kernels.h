// mvs_kernels.h -- launchers of the HIP kernels (internal), grouped by the unit that defines them.
#pragma once
#include <hip/hip_runtime.h>
#include "mvs_types.h"

// mvs_image.hip: texels, pyramids and masks; the exclusive scan (out has n + 1 slots, tmp at least n / 512 + 64); gather / scatter of int32
void mvsk_rgb_to_rgba(const uint8_t* rgb, uint32_t* out, int64_t n, hipStream_t st);
void mvsk_rgba_to_rgb(const uint32_t* in, uint8_t* rgb, int64_t n, hipStream_t st);
void mvsk_pyr_down(const uint32_t* src, int pw, int ph, uint32_t* dst, int w, int h, hipStream_t st);
void mvsk_mask_down(const uint8_t* src, int pw, int ph, uint8_t* dst, int w, int h, hipStream_t st);
void mvsk_mask_binarise(uint8_t* m, int64_t n, hipStream_t st);
void mvsk_exclusive_scan(const int32_t* in, int32_t* out, int64_t n, int32_t* tmp, hipStream_t st);
void mvsk_exclusive_scan_off(const int32_t* in, csr_off_t* out, int64_t n, csr_off_t* tmp, hipStream_t st);
void mvsk_gather_i32(const int32_t* src, const int32_t* idx, int32_t* out, int64_t n, hipStream_t st);
void mvsk_scatter_i32(int32_t* dst, const int32_t* idx, const int32_t* val, int64_t n, hipStream_t st);
// mvs_index.hip: the cell index and the per-cell maps of the pool
void mvsk_index_count(const DParams& prm, int32_t* cnt, int32_t* vcnt, unsigned long long* total, hipStream_t st);
void mvsk_index_fill(const DParams& prm, int vgrid, const csr_off_t* start, int32_t* cursor, unsigned long long* ids, hipStream_t st);
void mvsk_index_fill_direct(const DParams& prm, int vgrid, const csr_off_t* start, int32_t* cursor, int32_t* id32, hipStream_t st);
void mvsk_index_sort_trim(const DParams& prm, const csr_off_t* start, unsigned long long* ids, int do_trim, unsigned long long* trimmed, hipStream_t st);
void mvsk_index_finalize(const DParams& prm, int vgrid, const csr_off_t* start, unsigned long long* ids, int32_t* id32, int32_t* cnt_alive, hipStream_t st);
void mvsk_index_pack(const DParams& prm, const csr_off_t* start, const csr_off_t* start2, const int32_t* cnt_alive, const unsigned long long* ids, const int32_t* id32_in,
                     ListKey* key, int32_t* id32_out, hipStream_t st);
void mvsk_depth_maps(const DParams& prm, unsigned long long* dp, const uint32_t* dirty, hipStream_t st);
void mvsk_depth_mark_dirty(const DParams& prm, const uint8_t* kill, unsigned long long* dp, uint32_t* dirty, hipStream_t st);
void mvsk_best_ncc_map(const DParams& prm, int view, unsigned long long* best, hipStream_t st);
void mvsk_map_extract(const DParams& prm, int view, int kind, const unsigned long long* sel, float* depth, float* normal, int32_t* ids, int ncells, hipStream_t st);
// mvs_sweep.cuh (in mvs_patch.hip): the job lists, the sweep and its retry tier, the commit of a pass
// the refiner of a sweep / refine probe (mvs_engine_set_refiner): simplex = 0 is the halving search of the default kernels,
// simplex = 1 the CONVERGED refiner (k_sweep_simplex, k_sweep_retry_simplex, k_probe_refine_simplex) with these two arguments
struct RefineSel { int simplex; int max_evals; float xtol; };
// The variant of a sweep or refine-probe kernel.  full_window: the instantiation for a window in which every class-lane slot holds a
// sample (cls_full_window: the default 7x7); narrow: the samplers that take 32-bit texel offsets from DParams::pyr32 (a pyramid block
// below 4 GiB); pair: consecutive trials of a cell are refined two at a time.  mvsk_kernel_variant: what a launch on prm may use, with the
// switches MVS_SWEEP_FULLWINDOW, MVS_SAMPLER_WIDE and MVS_SWEEP_PAIR applied (launched = false).  mvsk_sweep and mvsk_probe return what
// they used: launched = false where mvsk_sweep had nothing to launch and where mvsk_probe launched anything but the refine probe of the
// default refiner (k_probe_refine, k_probe_refine_ofs) -- the engine counts the launched ones by full_window and narrow.
struct KernelVariant { bool launched, full_window, narrow, pair; };
KernelVariant mvsk_kernel_variant(const DParams& prm);
size_t mvsk_sweep_lds_bytes(const DParams& prm);
KernelVariant mvsk_sweep(const DParams& prm, const SweepArgs& a, const RefineSel& rs, hipStream_t st);
void mvsk_sweep_retry(const DParams& prm, const SweepArgs& a, int nretry, const RefineSel& rs, hipStream_t st);
void mvsk_job_work(const DParams& prm, const SweepArgs& a, int mode, int shift, int32_t* work, hipStream_t st);
// The sweep's job lists: clears job_nstage[0, njobs) and lists the jobs of [job_lo, job_hi) that run a trial, per queue.  flags and scan
// are scratch of mvsk_job_list_seg(a) * MVS_SWEEP_QUEUES (< job_hi - job_lo + 1024) and one more ints; list holds up to job_hi - job_lo
// jobs, bounds MVS_SWEEP_QUEUES + 1 ints (bounds[MVS_SWEEP_QUEUES] = the number listed; untouched when the range is empty)
int mvsk_job_list_seg(const SweepArgs& a);
void mvsk_job_list(const DParams& prm, const SweepArgs& a, int32_t* flags, int32_t* scan, int32_t* scan_tmp, int32_t* list, int32_t* bounds, hipStream_t st);
void mvsk_job_cuts(const int32_t* scan, int64_t njobs, int n, int32_t* cuts, hipStream_t st);
void mvsk_commit_count(const SweepArgs& a, int32_t* cnt, hipStream_t st);
void mvsk_commit_copy(const SweepArgs& a, const int32_t* base, DPatch* dst, int64_t dst_cap, int32_t* per_view, int keep_key, hipStream_t st);
// mvs_filter.cuh (in mvs_patch.hip): pool upkeep (the scores of patches that come without one among it) and Filter::run
void mvsk_fill_ncc(const DParams& prm, unsigned long long* evals, hipStream_t st);
void mvsk_kill_count(const uint8_t* kill, int64_t n, int32_t* cnt, hipStream_t st);
void mvsk_kill_export(const uint8_t* kill, int64_t n, const int32_t* base, int32_t* ids, int64_t cap, hipStream_t st);
void mvsk_apply_kill_flags(DPatch* pool, uint8_t* kill, int64_t n, hipStream_t st);
void mvsk_apply_kill_ids(DPatch* pool, const int32_t* ids, int64_t n, int64_t pool_n, hipStream_t st);
void mvsk_append_records(DPatch* pool, int64_t pool_n, const DPatch* recs, int64_t n, hipStream_t st);
void mvsk_alive_count(const DPatch* pool, int64_t n, int32_t* cnt, hipStream_t st);
void mvsk_alive_gather(const DPatch* pool, int64_t n, const int32_t* base, DPatch* out, int64_t cap, hipStream_t st);
void mvsk_filter_vimages(const DParams& prm, int additive, int64_t first, int64_t last, const uint32_t* dirty, hipStream_t st);
void mvsk_geo_pack(const DPatch* pool, int64_t n, float4* geo, uint8_t* ref, int* bad, hipStream_t st);
void mvsk_filter_outside(const DParams& prm, uint8_t* kill, int64_t first, int64_t last, hipStream_t st);
void mvsk_filter_exact(const DParams& prm, uint8_t* kill, unsigned long long* evals, unsigned long long* stage, int64_t first, int64_t last, hipStream_t st);
void mvsk_filter_neighbor(const DParams& prm, uint8_t* kill, int32_t* retry, int32_t* nretry, int32_t* overflow, unsigned long long* stats, int64_t first, int64_t last, hipStream_t st);
void mvsk_filter_neighbor_retry(const DParams& prm, uint8_t* kill, const int32_t* todo, int32_t ntodo, int32_t* overflow, unsigned long long* stats, hipStream_t st);
void mvsk_groups(const DParams& prm, int* parent, int* size, int threshold, uint8_t* kill, hipStream_t st);
void mvsk_groups_literal_edges(const DParams& prm, int* parent, int* size, int* edges2, int* nedges, int cap, hipStream_t st);
void mvsk_groups_kill(const DParams& prm, const int* parent, const int* size, int threshold, uint8_t* kill, hipStream_t st);
// mvs_probe.cuh (in mvs_patch.hip): op 6 needs rs.simplex (the engine checks it); op 2 follows rs
KernelVariant mvsk_probe(const DParams& prm, int op, int64_t n, const DPatch* in, const float* in_f, DPatch* out, float* out_f, int32_t* out_i, const RefineSel& rs,
                         hipStream_t st);
// mvs_engine_export_ply (mvs_ply.hip): the alive pool slots of [i0, i1) -> idx (base = exclusive scan of the alive flags); the
// colour (and ASCII line length) of each listed vertex; the vertex records into out at off[k] (ASCII) or 27 k (binary: off null)
void mvsk_ply_select(const DPatch* pool, const int32_t* base, int64_t i0, int64_t i1, int32_t* idx, hipStream_t st);
void mvsk_ply_colour(const DPatch* pool, const int32_t* idx, int64_t n, const DView* views, int nviews, int level, int ascii, uint32_t* rgb, int32_t* len,
                     hipStream_t st);
void mvsk_ply_emit(const DPatch* pool, const int32_t* idx, int64_t n, const uint32_t* rgb, const int64_t* off, uint8_t* out, hipStream_t st);
// mvs_engine_seed_patches (mvs_seed.hip): DepthNormInit::createPatches' PLY branch.  SeedView: what the accumulate launch of one view
// needs by value; SeedCam: the camera centre and pixel scale Optim::sortImages reads, one per view in device memory.
struct SeedView { float P[12]; int32_t W, H, view; };
struct SeedCam { float center[4]; float ipscale; };
// one view's pass over the points: sum[3 i ..] += map[pixel], bits[i] |= 1 << view where the point projects onto a foreground pixel
void mvsk_seed_accumulate(const SeedView& sv, const float* map, const uint8_t* mask, const float* xyz, int64_t n, float* sum, unsigned long long* bits,
                          hipStream_t st);
// keep[i] = 1 where point i gives a patch; then, with base = the exclusive scan of keep, the records at dst[base[i]]
void mvsk_seed_flags(const SeedCam* cams, int level, const float* xyz, const float* sum, const unsigned long long* bits, int64_t n, int32_t* keep,
                     hipStream_t st);
void mvsk_seed_emit(const SeedCam* cams, int nviews, int level, float thr, float tmp_unit, const float* xyz, const float* sum, const unsigned long long* bits,
                    const int32_t* keep, const int32_t* base, int64_t n, DPatch* dst, hipStream_t st);
// mvs_engine_seed_random (mvs_seed_random.hip): the cold start, the first of two front ends to one chain (mvs_seed_chain.cuh; SeedChainArgs
// in mvs_types.h is what their launches share).  SeedRandomArgs: one view's launch by value -- the call's parameters, the
// view and its depth range.
struct SeedRandomArgs { SeedChainArgs chain; uint32_t seed; float max_tilt; int32_t view; float dmin, dmax; };
size_t mvsk_texs_lds_bytes(const DParams& prm);  // mvs_filter.cuh: the dynamic LDS of a wave that runs postProcess without Optim::check
// the K hypotheses of cells[i] (cells of the view's grid) as records at out[i * K ..]
void mvsk_seed_random_hypotheses(const DParams& prm, const SeedRandomArgs& a, int64_t ncells, const int32_t* cells, DPatch* out, hipStream_t st);
// one wave per cell of the view: the patch of cell c, if it gives one, at stage[c] with keep[c] = 1 (keep zero before the launch)
void mvsk_seed_random(const DParams& prm, const SeedRandomArgs& a, int ncells, DPatch* stage, int32_t* keep, hipStream_t st);
// both front ends' staged append: with base = the exclusive scan of keep, the staged records of the n jobs to dst[base[j]] with
// id = id0 + base[j] (mvs_seed_random.hip)
void mvsk_seed_gather(const DPatch* stage, const int32_t* keep, const int32_t* base, int n, DPatch* dst, int32_t id0, hipStream_t st);
// mvs_engine_seed_points (mvs_seed_points.hip): the warm start.  xyz: 3 floats per point of the launch.
// the hypotheses of point i as records at out[i * K ..], count[i] of them, zero bytes in the slots behind
void mvsk_seed_points_hypotheses(const DParams& prm, int K, int64_t n, const float* xyz, DPatch* out, int32_t* count, hipStream_t st);
// one wave per point of the chunk: the patch of point j, if it gives one, at stage[j] with keep[j] = 1 (keep zero before the launch)
void mvsk_seed_points(const DParams& prm, const SeedPointsArgs& a, const float* xyz, DPatch* stage, int32_t* keep, hipStream_t st);
// per view: cnt[v] += the points that pass its gate, lo[v] / hi[v] = min / max with the bits of their depths (lo 0xffffffff, hi and cnt 0
// before the first launch)
void mvsk_depth_ranges(const DParams& prm, int64_t n, const float* xyz, uint32_t* lo, uint32_t* hi, unsigned long long* cnt, hipStream_t st);
// mvs_engine_render_maps / mvs_engine_fused_points (mvs_maps.hip): dense per-view maps and their fusion.  MapsArgs: what the agreement
// launch of one view needs by value -- where every view's pixels start in the all-view id and point buffers, and the two tolerances.
struct MapsArgs { int64_t pix_base[MVS_MAXVIEWS + 1]; float depth_tol, normal_cos; };
// source 0's selection of every view in one pass over the pool (k_best_ncc_map's keys; sel[0, total_cells) zero before the launch)
void mvsk_maps_select(const DParams& prm, unsigned long long* sel, hipStream_t st);
// one view (W x H at m_level): the selected plane of every pixel's cell cut by the pixel's ray -> ids[y W + x] (-1: invalid) and the point
// pts[3 (y W + x) ..] (NaN); source 0: sel = the keys above, source 1: m_dpgrids (k_depth_maps' keys)
void mvsk_maps_render(const DParams& prm, int view, int W, int H, int source, const unsigned long long* sel, int32_t* ids, float* pts, hipStream_t st);
// one view's agree words and depth / normal / conf maps (npix values each, any of them null) from the ids and points of ALL views
void mvsk_maps_agree(const DParams& prm, const MapsArgs& a, int view, int64_t npix, const int32_t* ids, const float* pts, unsigned long long* agree,
                     float* depth, float* normal, float* conf, hipStream_t st);
// flag[i] (and the byte flag8[i], if given) = pixel i of the view counts: valid and, with agree, consistent and not spoken for by a lower
// view; ids: the view's slice
void mvsk_maps_flag(int64_t npix, int view, const int32_t* ids, const unsigned long long* agree, int min_consistent, int dedupe, int32_t* flag,
                    uint8_t* flag8, hipStream_t st);
void mvsk_maps_expand(int64_t npix, const uint8_t* flag8, int32_t* flag, hipStream_t st);
// the 32-byte records (mvs_fused_point) of the view's flagged pixels at out[base[i]], base = the exclusive scan of flag; ids, pts: the view's slices
void mvsk_maps_gather(const DParams& prm, int view, int64_t npix, const int32_t* ids, const float* pts, const int32_t* flag, const int32_t* base,
                      void* out, int64_t cap, hipStream_t st);
// mvs_engine_tsdf / mvs_engine_extract_mesh / mvs_engine_mesh (mvs_mesh.hip): a truncated signed distance volume over the dense maps and
// marching tetrahedra over a volume.  MeshVol: mvs_volume by value.  Every array has one element per lattice point, p = (k ny + j) nx + i.
struct MeshVol { float origin[3]; float voxel; int32_t nx, ny, nz; float trunc; int32_t min_count; };
inline int64_t mesh_npoints(const MeshVol& vol) { return (int64_t)vol.nx * vol.ny * vol.nz; }
// ids / usable: every view's pixels (view v's at a.pix_base[v]): the id map of mvsk_maps_render and the flag bytes of mvsk_maps_flag without dedupe
void mvsk_mesh_tsdf(const DParams& prm, const MapsArgs& a, const MeshVol& vol, const int32_t* ids, const uint8_t* usable, float* tsdf, int32_t* count,
                    hipStream_t st);
// state[p]: bit 0 OBSERVED (tsdf not NaN and, with count, count >= min_count), bit 1 INSIDE (observed and tsdf < 0)
void mvsk_mesh_state(const MeshVol& vol, const float* tsdf, const int32_t* count, uint8_t* state, hipStream_t st);
// mask[p]: bit d - 1 = the edge (p, d) carries a vertex; cnt[p] = their number
void mvsk_mesh_edges(const MeshVol& vol, const uint8_t* state, uint8_t* mask, int32_t* cnt, hipStream_t st);
// the vertices of p at verts[3 (vbase[p] + rank) ..], vbase = the exclusive scan of cnt; nothing at or beyond cap_v
void mvsk_mesh_verts(const MeshVol& vol, const float* tsdf, const uint8_t* mask, const int32_t* vbase, float* verts, int64_t cap_v, hipStream_t st);
// cnt[p] = the triangles of the cube whose corner 0 is p; then, with tbase = their exclusive scan, the triangles at tris[3 tbase[p] ..]
void mvsk_mesh_tcount(const MeshVol& vol, const uint8_t* state, int32_t* cnt, hipStream_t st);
void mvsk_mesh_tris(const MeshVol& vol, const uint8_t* state, const uint8_t* mask, const int32_t* vbase, const int64_t* tbase, int32_t* tris,
                    int64_t cap_t, hipStream_t st);
// mvs_engine_mesh_normals / mvs_engine_mesh_colours (mvs_mesh_attr.hip): vertex normals as an order-free integer sum, vertex colours
// blended from the views that see the vertex.  verts: 3 floats a vertex, tris: 3 ids a triangle.
// every triangle's ids checked against n_v (*bad != 0 when one lies outside; such a triangle reads no vertex) and *mbits = the bits of
// the largest |component| of the finite face vectors; both words zero before the launch
void mvsk_mesh_normals_scan(int64_t n_v, const float* verts, int64_t n_t, const int32_t* tris, uint32_t* mbits, uint32_t* bad, hipStream_t st);
// acc[3 i ..] += the face vectors around vertex i, scaled by the power of two that *mbits gives and rounded to integers (acc zero before
// the launch, every id valid); then normals[3 i ..] = acc[3 i ..] normalised in fp64
void mvsk_mesh_normals_accum(const float* verts, int64_t n_t, const int32_t* tris, const uint32_t* mbits, long long* acc, hipStream_t st);
void mvsk_mesh_normals_finish(int64_t n_v, const long long* acc, float* normals, hipStream_t st);
// MeshColourArgs: mvs_mesh_colouring by value.  ids / usable as for mvsk_mesh_tsdf; normals and used may be null; rgb: 3 bytes a vertex
struct MeshColourArgs { float occl_tol, min_cos; };
void mvsk_mesh_colours(const DParams& prm, const MapsArgs& a, const MeshColourArgs& m, int64_t n_v, const float* verts, const float* normals,
                       const int32_t* ids, const uint8_t* usable, uint8_t* rgb, uint8_t* used, hipStream_t st);
// the same with one more gate: view v takes part for vertex i only when bit v of visible[i] is set (k_mattr_colours_visible)
void mvsk_mesh_colours_visible(const DParams& prm, const MapsArgs& a, const MeshColourArgs& m, int64_t n_v, const float* verts, const float* normals,
                               const int32_t* ids, const uint8_t* usable, const unsigned long long* visible, uint8_t* rgb, uint8_t* used, hipStream_t st);
// mvs_engine_mesh_render / mvs_engine_mesh_visibility (mvs_mesh_render.hip): a z-buffer of the mesh per view and the vertex visibility
// from it, one view at a time.  Every launcher wants valid ids.
// scr[2 i ..] = vertex i in 1/256 pixel of `view` at prm.level (saturated to int32), vd[i] = its depth, ok[i] = 1 where it is usable
void mvsk_mrender_project(const DParams& prm, int view, int64_t n_v, const float* verts, int32_t* scr, float* vd, uint32_t* ok, hipStream_t st);
// keys (W H words, all ones before) take the minimum of (bits(depth) << 32) | row over the triangles that cover each pixel centre; a
// triangle whose clipped box holds more than small_max pixels goes through list (n_t slots); counts (zero before): [0] the listed
// triangles, [1] the skipped ones
void mvsk_mrender_raster(int64_t n_t, const int32_t* tris, const int32_t* scr, const float* vd, const uint32_t* ok, int W, int H, int small_max,
                         unsigned long long* keys, int32_t* list, unsigned long long* counts, hipStream_t st);
// depth[p], tri[p] (either may be null) from keys[p], NaN and -1 where it is all ones; *covered (zero before) += the pixels with a key
void mvsk_mrender_resolve(int64_t npix, const unsigned long long* keys, float* depth, int32_t* tri, unsigned long long* covered, hipStream_t st);
// visible[i] |= 1 << view where vertex i is usable, its nearest pixel lies inside W x H and is empty or not nearer than d / (1 + tol)
void mvsk_mrender_visible(int view, float tol, int64_t n_v, const int32_t* scr, const float* vd, const uint32_t* ok, int W, int H, const unsigned long long* keys,
                          unsigned long long* visible, hipStream_t st);
// mvs_engine_mesh_face_views / mvs_engine_mesh_texture (mvs_mesh_texture.hip): the view that textures each triangle, and the atlas.  The
// views stream through mvsk_mrender_project's buffers.  Every launcher wants valid ids.
// *bad |= 1 when a label lies outside -1 .. nviews - 1 (zero before the launch)
void mvsk_mtex_check_labels(int64_t n_t, const int32_t* label, int nviews, uint32_t* bad, hipStream_t st);
// one view: where triangle t is a candidate of `view` (W x H) with |area| > best_area[t], both slots take the view's; want: the sign the
// area must have, 0 = either; visible may be null.  best_area 0 and best_label -1 before the first view, the views in ascending order
void mvsk_mtex_best(int view, int want, int64_t n_t, const int32_t* tris, const int32_t* scr, const uint32_t* ok, const unsigned long long* visible, int W, int H,
                    long long* best_area, int32_t* best_label, hipStream_t st);
// counts[v] += the triangles labelled v (zero before the launch)
void mvsk_mtex_count(int64_t n_t, const int32_t* label, int nviews, unsigned long long* counts, hipStream_t st);
// one view: for the triangles labelled `view` whose label is honoured, win[9 t ..] = (sx, sy, bits(d)) x 3 and flag[t] = 1 (flag zero
// before the first view)
void mvsk_mtex_take(int view, int64_t n_t, const int32_t* tris, const int32_t* label, const int32_t* scr, const float* vd, const uint32_t* ok, int32_t* win,
                    int32_t* flag, hipStream_t st);
// with base = the exclusive scan of flag: list[base[t]] = t for the n_textured flagged triangles; uv[6 t ..] (or null) = the corner texels
void mvsk_mtex_layout(int64_t n_t, const int32_t* flag, const int32_t* base, int32_t* list, int64_t n_textured, int res, int cpr, int32_t* uv, hipStream_t st);
// the atlas of `width` x `height` texels, three bytes each, from the level prm.level of the labelled views; rgb holds the bytes rounded
// up to a multiple of twelve
void mvsk_mtex_texels(const DParams& prm, int res, int width, int64_t height, int64_t n_textured, const int32_t* list, const int32_t* label, const int32_t* win,
                      uint8_t* rgb, hipStream_t st);
// The seam calls of include/mvskit_seams.h.  In mvs_mesh_texture.hip, with the gates and the texel chain:
// one view, behind mvsk_mtex_best over all views: quality[t * nviews + view] = max(1, 255 |area| / best_area[t]) where t is a candidate
// (quality zero before the first view)
void mvsk_mtex_quality(int view, int want, int64_t n_t, const int32_t* tris, const int32_t* scr, const uint32_t* ok, const unsigned long long* visible, int W, int H,
                       const long long* best_area, int nviews, uint8_t* quality, hipStream_t st);
// mvsk_mtex_texels with offset[3 v ..], view v's levels in 1/16 grey level, added before the rounding
void mvsk_mtex_texels_levelled(const DParams& prm, int res, int width, int64_t height, int64_t n_textured, const int32_t* list, const int32_t* label,
                               const int32_t* win, const int32_t* offset, uint8_t* rgb, hipStream_t st);
// pairs[(min * nviews + max) * 4 ..] += (N, S_r, S_g, S_b) of the seam edges between two views, *n_edges += the seam edges (both zero
// before the launch); nbr from mvsk_mseam_adjacency, flag and win from mvsk_mtex_take over all views
void mvsk_mtex_seam_samples(const DParams& prm, int nviews, int samples, int64_t n_t, const int32_t* tris, const int32_t* nbr, const int32_t* label,
                            const int32_t* flag, const int32_t* win, long long* pairs, unsigned long long* n_edges, hipStream_t st);
// In mvs_mesh_seams.hip: the edge table (tkey all ones, tval zero before; slots a power of two), nbr[3 t + k] = the triangle across edge
// k or -1, *nirr (or null) += the irregular edges; *fail != 0: a probe ran out
void mvsk_mseam_adjacency(int64_t n_t, const int32_t* tris, unsigned long long* tkey, int32_t* tval, int32_t* town, int64_t slots, int32_t* nbr,
                          unsigned long long* nirr, uint32_t* fail, hipStream_t st);
// *seams += the adjacent pairs whose labels are both >= 0 and differ
void mvsk_mseam_count(int64_t n_t, const int32_t* nbr, const int32_t* label, unsigned long long* seams, hipStream_t st);
// iteration `it` of the smoothing, a propose and an apply launch: moved[it] += the triangles that moved (moved zero before the first);
// nothing happens when moved[it - 1] == 0.  Labels in -1 .. nviews_q - 1
void mvsk_mseam_iteration(int it, unsigned long long* moved, int64_t n_t, const int32_t* tris, const int32_t* nbr, int nviews_q, const uint8_t* quality, int keep,
                          int32_t* prop, int32_t* score, int32_t* label, hipStream_t st);
// mvs_engine_mesh_components / mvs_engine_mesh_prune / mvs_engine_mesh_smooth (mvs_mesh_clean.hip): connected components by union-find,
// pruning behind two scans, Taubin smoothing as an order-free integer sum.  verts: 3 floats a vertex, tris: 3 ids a triangle.
// *bad != 0 when an id of a triangle lies outside 0 .. n_v - 1 (zero before the launch); every launcher below wants valid ids
void mvsk_mesh_check_ids(int64_t n_v, int64_t n_t, const int32_t* tris, uint32_t* bad, hipStream_t st);
// parent[i] = the smallest id of i's component, size[i] = the triangles of that component, *ncomp += the components with a triangle
void mvsk_mesh_components(int64_t n_v, int64_t n_t, const int32_t* tris, int32_t* parent, int32_t* size, unsigned long long* ncomp, hipStream_t st);
// parent[i] = the root of i in a union-find whose unions are done (the third launch of mvsk_mesh_components; mvs_mesh_fill.hip's too)
void mvsk_mesh_flatten(int64_t n_v, int32_t* parent, hipStream_t st);
// *best = max over the components with a triangle of (size << 32) | (0xffffffff - label) (zero before the launch)
void mvsk_mesh_largest(int64_t n_v, const int32_t* parent, const int32_t* size, unsigned long long* best, hipStream_t st);
// tflag[t] = triangle t is kept; vflag[i] = 1 where a kept triangle names vertex i (vflag zero before the launch); best is read with largest_only
void mvsk_mesh_keep(int64_t n_t, const int32_t* tris, const int32_t* parent, const int32_t* size, int64_t min_triangles, int largest_only,
                    const unsigned long long* best, int32_t* tflag, int32_t* vflag, hipStream_t st);
// with vbase / tbase = the exclusive scans of the flags: the kept rows in input order, ids rewritten; vflag becomes the vertex map (-1: dropped)
void mvsk_mesh_gather(int64_t n_v, const float* verts, int32_t* vflag, const int32_t* vbase, float* out_verts, int64_t cap_v, int64_t n_t, const int32_t* tris,
                      const int32_t* tflag, const int32_t* tbase, int32_t* out_tris, int64_t cap_t, hipStream_t st);
// one STEP with factor f from xin to xout: *mbits zero before the launch, acc (3 int64 a vertex) and cnt zero before and after it
void mvsk_mesh_smooth_step(int64_t n_v, const float* xin, float* xout, float f, int64_t n_t, const int32_t* tris, uint32_t* mbits, long long* acc, int32_t* cnt,
                           hipStream_t st);
// mvs_engine_mesh_decimate (mvs_mesh_decimate.hip): vertex clustering on a grid.  One open-addressing table (tkey: `slots` 64-bit keys,
// all ones = empty; tval: their values, at least 2^30 before a fill; slots a power of two >= twice the items) finds the clusters and
// the duplicate triangles.  Every launcher wants valid ids.
// used[i] = 1 where a triangle names vertex i (zero before); key[i] = the packed cell of member i, all ones for an unused vertex; *mbits =
// the bits of the members' largest |component|, *bad != 0 when a member is not finite or lies outside the grid (both zero before)
void mvsk_mdec_members(int64_t n_v, const float* verts, int64_t n_t, const int32_t* tris, const float* origin, float cell, int32_t* used,
                       unsigned long long* key, uint32_t* mbits, uint32_t* bad, hipStream_t st);
// out[i] = the smallest item index that carries key[i] (-1 for an item whose key is all ones); *fail != 0 when a probe ran out of slots
void mvsk_mdec_table(int64_t n, const unsigned long long* key, unsigned long long* tkey, int32_t* tval, int64_t slots, int32_t* out, uint32_t* fail,
                     hipStream_t st);
// key[t] = (a << 30) | b of the sorted representatives a < b < c, all ones for a collapsed triangle; then, with first[t] = the table's
// answer to that key, key[t] = (first[t] << 30) | c
void mvsk_mdec_tkey1(int64_t n_t, const int32_t* tris, const int32_t* rep, unsigned long long* key, hipStream_t st);
void mvsk_mdec_tkey2(int64_t n_t, const int32_t* tris, const int32_t* rep, const int32_t* first, unsigned long long* key, hipStream_t st);
// tflag[t] = (winner[t] == t), winner the table's answer to the second key; vflag[r] = 1 on the representatives of a kept triangle (zero before)
void mvsk_mdec_keep(int64_t n_t, const int32_t* tris, const int32_t* rep, const int32_t* winner, int32_t* tflag, int32_t* vflag, hipStream_t st);
// the output positions at out_verts[3 vbase[r] ..] of the flagged representatives r; acc (3 int64 a vertex) and cnt zero before, best
// (read with placement 1) all ones
void mvsk_mdec_positions(int placement, int64_t n_v, const float* verts, const int32_t* rep, const int32_t* vflag, const int32_t* vbase, const uint32_t* mbits,
                         long long* acc, int32_t* cnt, unsigned long long* best, float* out_verts, int64_t cap_v, hipStream_t st);
// the vertex map and the kept triangles in input order, ids rewritten
void mvsk_mdec_gather(int64_t n_v, const int32_t* rep, const int32_t* vflag, const int32_t* vbase, int32_t* vmap, int64_t n_t, const int32_t* tris,
                      const int32_t* tflag, const int32_t* tbase, int32_t* out_tris, int64_t cap_t, hipStream_t st);
// mvs_engine_mesh_boundaries / mvs_engine_mesh_fill (mvs_mesh_fill.hip): the boundary loops of a mesh and their centroid fans.  One
// open-addressing table (tkey: `slots` 64-bit keys, all ones = empty; tval: their counts, zero before the fill; slots a power of two >=
// six times the triangles) counts the directed edges.  Every launcher wants valid ids.
// loop[i] = the smallest vertex id of i's boundary component (-1: on no boundary), length[i] = its half-edges, negated when it is
// complex; counts[0..2] += the loops, the complex components, the irregular pairs; next[a] = b for the boundary half-edge a -> b of a
// simple vertex a.  outc, inc, cplx, next, hed, rbad (a word a vertex each), counts and *fail zero before; *fail != 0: a probe ran out
void mvsk_mfill_boundaries(int64_t n_v, int64_t n_t, const int32_t* tris, unsigned long long* tkey, int32_t* tval, int64_t slots, int32_t* parent, int32_t* outc,
                           int32_t* inc, int32_t* cplx, int32_t* next, int32_t* hed, int32_t* rbad, int32_t* loop, int32_t* length, unsigned long long* counts,
                           uint32_t* fail, hipStream_t st);
// tcnt[i] = the fill triangles whose half-edge starts at i, vcnt[i] = 1 at the label of a filled loop of 4 or more; *mbits = the bits of
// the largest |component| of the vertices of those loops, *bad != 0 when a vertex of a filled loop is not finite, *nfilled += the filled
// loops (all three zero before)
void mvsk_mfill_plan(int64_t n_v, const float* verts, const int32_t* loop, const int32_t* length, int32_t max_edges, int32_t* tcnt, int32_t* vcnt, uint32_t* mbits,
                     uint32_t* bad, unsigned long long* nfilled, hipStream_t st);
// with tbase / vbase = the exclusive scans of those counts: the fill triangles at add_tris[3 tbase[a] ..], the centroids at
// add_verts[3 vbase[label] ..] (their ids: n_v + vbase[label]); acc (3 int64 a vertex) zero before
void mvsk_mfill_emit(int64_t n_v, const float* verts, const int32_t* loop, const int32_t* length, int32_t max_edges, const int32_t* next, const int32_t* tbase,
                     const int32_t* vbase, const uint32_t* mbits, long long* acc, int32_t* add_tris, int64_t cap_t, float* add_verts, int64_t cap_v, hipStream_t st);
