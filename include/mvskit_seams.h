/* mvskit_seams.h -- the seam calls of the textured mesh of the MI355X PatchMatch-MVS engine: the adjacency of triangles, view labels
 * smoothed over it, and per-view colour levels computed on the seams.  An extension of mvskit_texture.h, which it includes: the handle,
 * the status codes, mvs_last_error and mvs_mesh_texturing are the earlier headers', and the calls are exported by the same libraries.
 * They have a header of their own because tests/test_mesh_texture_abi.py holds mvskit_texture.h to the three symbols it has; this one is
 * held against the binding's third table (mvskit_amd/abi.py, SEAM_SIGNATURES) in the same way by tests/test_mesh_seams_abi.py.
 *
 * Why: mvs_engine_mesh_face_views gives every triangle the view in which it projects largest.  Neighbouring triangles whose areas in
 * two views are nearly equal take different views, and every change of view across an edge shows in the atlas as a step in brightness.
 * The calls here remove most changes of view (mvs_engine_mesh_smooth_labels) and level the views' brightness where a change stays
 * (mvs_engine_mesh_seam_levels, mvs_engine_mesh_texture_levelled).  verts, tris, visible, label and the texturing struct are those of
 * mvskit_texture.h.  All calls are stateless and only read the engine; all array pointers may be host or device memory
 * (hipMemcpyDefault; the structs and the scalar outputs n_irregular, n_seam_edges, height, n_textured are host memory).  Every result is
 * an integer sum or an fp64 chain without contraction: the same bytes in any triangle order (per triangle) and across two calls.  A
 * refused call writes nothing.
 *
 * mvs_engine_mesh_adjacency (needs no views): edge k of triangle t runs from its vertex k to its vertex (k + 1) % 3.  nbr[t][k] is the
 *   row of the triangle that has the reverse directed edge when each of the two directed edges occurs exactly once in the mesh, else
 *   -1: a boundary edge, an irregular edge (a fin, a doubled triangle), and every edge of a triangle with two equal ids, which enters no
 *   edge (as in mvs_engine_mesh_boundaries).  *n_irregular (may be NULL) counts the irregular edges as mvs_engine_mesh_boundaries does.
 *
 * mvs_engine_mesh_face_quality: the candidate gates (a) to (d) of mvs_engine_mesh_face_views, by the same device function.
 *   quality[t][v] = 0 where v is no candidate for t, else max(1, 255 |area_v| / best_t) in int64 division, best_t = the largest |area|
 *   among t's candidates: the labelling's winner has 255.  nviews columns a row.
 *
 * mvs_engine_mesh_smooth_labels (needs no views; a graph problem): nviews_q is the row length of quality, 1 .. 64.  View l is
 *   ADMISSIBLE for t when quality[t][l] >= keep.  A_t(l) = the number of t's neighbours in nbr whose label is l; a label -1 agrees with
 *   nothing, and a triangle labelled -1 never moves.  Every iteration, from the labels at its start:
 *     PROPOSAL   among the labels of t's neighbours that are >= 0, differ from t's own and are admissible for t, the one with the
 *                largest (A_t(l), quality[t][l], -l); gain = A_t(proposal) - A_t(own).  Only a gain above 0 counts.
 *     MOVERS     t moves to its proposal when its gain is above 0 and it beats every neighbour whose gain is above 0: the larger
 *                (gain, quality of the proposal) wins, among equals the lexicographically smaller ascending triple of vertex ids; a
 *                full tie (two triangles on the same three vertices) moves neither.  The movers are an independent set, each strictly
 *                raises its own agreement while its neighbours stand still: the number of seams falls strictly every iteration.
 *   The loop ends after an iteration that moves nothing, or after `iterations`.  A SEAM is an adjacent pair of triangles, counted
 *   once, whose labels are both >= 0 and differ.  stats = (seams before, seams after, moves, iterations that moved something).  With
 *   iterations == 0 label_out == label_in.  label_in and label_out may be the same array.
 *
 * mvs_engine_mesh_seam_levels: labels are HONOURED as in mvs_engine_mesh_texture.  A SEAM EDGE is a pair in nbr whose two triangles
 *   both have honoured labels a != b (a the label of the side taken); it is taken once, from the side whose directed edge p -> q has
 *   p < q.  It is sampled at k = 0 .. samples with the integer weights n_p = samples - k, n_q = k.  In view v (a, then b), with
 *   (sx, sy, d) of p and q in v, TEXEL's chain on two vertices, fp64, left to right, without contraction: a_p = (double)n_p (double)d_p,
 *   a_q alike; den = a_p + a_q; xs = (a_p (double)sx_p + a_q (double)sx_q) / den, ys alike; x = xs / 256.0, y alike; TEXEL's grey
 *   conditions, clamp and bilinear c per channel; L = (int64)floor(c * 16.0 + 0.5).  A sample that is grey in either view is skipped.
 *   pairs[a][b] = (N, S_r, S_g, S_b): the samples of the seam edges between a and b, and S = sum(L_a - L_b); pairs[b][a] =
 *   (N, -S_r, -S_g, -S_b), the diagonal 0.  *n_seam_edges (may be NULL) = the seam edges.
 *   OFFSETS    per channel, on the host, fp64 without contraction: the g that minimise sum_pairs sum_samples (L_a + g_a - L_b - g_b)^2 +
 *              sum_v g_v^2.  n = nviews; for a = 0 .. n-1: A[a][a] = 1, s = 0; for b = 0 .. n-1, b != a, ascending:
 *              A[a][a] = A[a][a] + N_ab, s = s + S_ab, A[a][b] = -N_ab; rhs[a] = -s.  Elimination without pivoting:
 *                  for i = 0 .. n-1: for r = i+1 .. n-1: f = A[r][i] / A[i][i];
 *                      for c = i .. n-1: A[r][c] = A[r][c] - f * A[i][c];  rhs[r] = rhs[r] - f * rhs[i];
 *                  for i = n-1 .. 0: s = rhs[i]; for c = i+1 .. n-1: s = s - A[i][c] * g[c];  g[i] = s / A[i][i];
 *              g = fmin(fmax(g, -16 max_shift), 16 max_shift); offset[v][ch] = (int32)floor(g + 0.5), in 1/16 grey level.  A view
 *              without a seam gets 0.
 *
 * mvs_engine_mesh_texture_levelled: mvs_engine_mesh_texture with the byte
 *   clamp(floor(c + (double)offset[v][ch] / 16.0 + 0.5), 0.0, 255.0), v the triangle's label.  Grey texels stay 128.  Layout, size call,
 *   capacity and errors are that call's.  With offset NULL or all zeros the bytes equal mvs_engine_mesh_texture's.
 *
 * LIMITS: n_v, n_t in 0 .. 2^30.  Device memory per call: per triangle the 12 bytes of the input and 12 of nbr; the edge table, 16 bytes
 * a slot (key, count, owner), the smallest power of two >= 6 n_t slots and >= 1024; quality, n_t x nviews bytes; the smoothing 12 more a
 * triangle (label, proposal, score) and 8 bytes an iteration; the levels what mvs_engine_mesh_texture takes per triangle and vertex, and
 * nviews^2 x 32 bytes; the levelled atlas what mvs_engine_mesh_texture takes.
 * MVS_ERR_ARG, checked in this order before the handle is read: the struct(s) NULL (seams, then texturing); keep outside 1..255;
 * iterations outside 0..4096; max_shift outside 0..255; samples outside 1..16; res and width as in mvskit_texture.h; a negative count or
 * a count over the limit; verts NULL with n_v > 0; tris NULL with n_t > 0; then the call's own arrays in the order of its parameters,
 * each NULL with n_t > 0 (nviews_q outside 1..64 before quality; offset, pairs and stats NULL at any count; height, n_textured and cap_h
 * as in mvs_engine_mesh_texture); no engine.  MVS_ERR_STATE (face_quality, seam_levels, texture_levelled only): the views are not
 * set, or a pass is waiting for its commit.  Then MVS_ERR_ARG after a validating pass on the device: an id outside 0 .. n_v - 1, a
 * label outside -1 .. nviews - 1 (nviews_q - 1 in the smoothing).  MVS_ERR_HIP: an allocation or copy failed.
 * WHAT THESE CALLS DO NOT DO: pairwise energies other than Potts; graph cuts; per-vertex or Poisson levelling; chart packing; masks; a
 * variant sharded over GPUs. */
#ifndef MVSKIT_SEAMS_H
#define MVSKIT_SEAMS_H

#include "mvskit_texture.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mvs_mesh_seams {
    int32_t keep;       /* a view is admissible for a triangle from this quality on, 1..255 */
    int32_t iterations; /* of the smoothing at the most, 0..4096 */
    int32_t max_shift;  /* the largest offset of a view in grey levels, 0..255 */
    int32_t samples;    /* segments per seam edge, 1..16 */
} mvs_mesh_seams; /* 16 bytes */
void mvs_default_mesh_seams(mvs_mesh_seams* s); /* keep 192, iterations 64, max_shift 32, samples 4 */

int mvs_engine_mesh_adjacency(mvs_engine* e, int64_t n_v, int64_t n_t, const int32_t* tris, int32_t* nbr /* [n_t][3] */, int64_t* n_irregular /* or NULL */);
int mvs_engine_mesh_face_quality(mvs_engine* e, const mvs_mesh_texturing* x, int64_t n_v, const float* verts, int64_t n_t, const int32_t* tris,
                                 const uint64_t* visible /* [n_v] or NULL */, uint8_t* quality /* [n_t][nviews] */);
int mvs_engine_mesh_smooth_labels(mvs_engine* e, const mvs_mesh_seams* s, int64_t n_v, int64_t n_t, const int32_t* tris, int nviews_q,
                                  const uint8_t* quality /* [n_t][nviews_q] */, const int32_t* label_in /* [n_t] */, int32_t* label_out /* [n_t] */,
                                  int64_t* stats /* [4] */);
int mvs_engine_mesh_seam_levels(mvs_engine* e, const mvs_mesh_seams* s, const mvs_mesh_texturing* x, int64_t n_v, const float* verts, int64_t n_t,
                                const int32_t* tris, const int32_t* label /* [n_t] */, int32_t* offset /* [nviews][3] */,
                                int64_t* pairs /* [nviews][nviews][4] */, int64_t* n_seam_edges /* or NULL */);
int mvs_engine_mesh_texture_levelled(mvs_engine* e, const mvs_mesh_texturing* x, int64_t n_v, const float* verts, int64_t n_t, const int32_t* tris,
                                     const int32_t* label /* [n_t] */, const int32_t* offset /* [nviews][3] or NULL */, int64_t cap_h,
                                     uint8_t* rgb /* [cap_h][width][3] or NULL */, int32_t* uv /* [n_t][3][2] or NULL */, int64_t* height,
                                     int64_t* n_textured);

#ifdef __cplusplus
}
#endif
#endif /* MVSKIT_SEAMS_H */
