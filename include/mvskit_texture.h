/* mvskit_texture.h -- the textured-mesh calls of the MI355X PatchMatch-MVS engine: which view textures which triangle, and a texture
 * atlas with its texture coordinates, both on the device.  An extension of mvskit_engine.h, which it includes: the handle, the status
 * codes and mvs_last_error are that header's, and the calls are exported by the same libraries.  They have a header of their own
 * because tests/test_abi.py holds mvskit_engine.h to the prototypes and structs it has; this one is held against the binding's second
 * table (mvskit_amd/abi.py, TEXTURE_SIGNATURES) in the same way by tests/test_mesh_texture_abi.py.  A host that stops at the mesh
 * includes mvskit_engine.h alone and sees the interface it always saw.
 *
 * Textured mesh (no reference counterpart): the mesh leaves mvs_engine_mesh_colours with one colour per vertex; here every triangle gets
 * the texels of the view that sees it largest.  The pieces are the render's (mvskit_engine.h, "Mesh render"): its VERTEX rule gives the
 * snapped screen position (sx, sy), the depth d and the USABLE flag of every vertex per view, by the same device function;
 * mvs_engine_mesh_visibility gives the per-vertex visibility words; the RGBA8 pyramids are resident.  verts: n_v x 3 floats, tris:
 * n_t x 3 int32 vertex ids.  Both calls are stateless and only read the engine; they need views but no pool; all array pointers may be
 * host or device memory (hipMemcpyDefault; the struct, height and n_textured are host memory).  Masks play no part.  Every result is
 * integer arithmetic, or an fp64 chain without contraction from the device's own snapped vertices: the same bytes in any triangle order
 * (per triangle) and across two calls.  A refused call writes nothing.
 * Everything works at level L = m_level; W x H is a view's size there, the texels are those of mvs_engine_get_pyramid(v, L).
 *
 * mvs_engine_mesh_face_views: view v is a CANDIDATE for triangle t when
 *     (a) its three vertices are usable in v;
 *     (b) each lies in the bilinear window, in snapped units: 0 <= sx <= 256 (W - 1) - 1 and 0 <= sy <= 256 (H - 1) - 1;
 *     (c) area = (x1-x0)(y2-y0) - (y1-y0)(x2-x0) in int64 is not 0, and with front_only its sign equals f_v;
 *     (d) with visible != NULL, bit v is set in the words of all three vertices.
 *   f_v is the sign `area` has for a triangle whose FACE VECTOR (X1-X0) x (X2-X0) (mvs_engine_mesh_normals') points to the camera
 *   centre: f_v = -sign(det M) for P_L = [M | p], computed once per view on the host in fp64 from the float32 P_L.  For the usual camera
 *   (det M > 0, y down) f_v = -1: a triangle that faces the camera has a NEGATIVE area.  A view with det M == 0 has no orientation and
 *   is no candidate under front_only.
 *   The winner is the candidate with the largest |area| (the projected size in 1/65536 pixel^2), the lowest v among equals.
 *   label[t] = the winning v, or -1 when no view is a candidate; area[t] = the winner's |area|, or 0; n_faces[v] = the triangles
 *   labelled v.  area and n_faces may be NULL: not wanted.
 *
 * mvs_engine_mesh_texture: label is an input, the output of the call above or a caller's edit of it.  A label v >= 0 is HONOURED when
 *   the triangle's three vertices are usable in v and area != 0 there; gates (b) to (d) are the labelling call's business.  A triangle
 *   with label -1 or a label that is not honoured is UNTEXTURED.
 *     LAYOUT     B = res + 3, cpr = width / B.  The honoured triangles are numbered k = 0, 1, ... in row order (n_textured of them).
 *                Cell 0 is reserved, all 128 grey.  Cell q >= 1 holds triangle k = 2 (q - 1) in its lower half and k + 1 in its upper
 *                half; its origin is the texel ((q % cpr) B, (q / cpr) B).  n_cells = 1 + ceil(n_textured / 2),
 *                height = ceil(n_cells / cpr) B.  height > 32768 or width height > 2^30 is MVS_ERR_CAPACITY (with *height and
 *                *n_textured written).
 *     SIZE CALL  mvs_engine_export_ply's convention: with rgb == NULL or cap_h < height, *height and *n_textured are exact and nothing
 *                else is written (uv neither); MVS_ERR_CAPACITY when rgb != NULL.
 *     OWNERSHIP  texel (i, j) of a cell, relative to its origin: i + j <= res + 2 belongs to the lower triangle, whose corners lie on
 *                the centres of the texels (0, 0), (res, 0), (0, res) for vertices 0, 1, 2; i + j >= res + 3 to the upper one, whose
 *                corners lie on (res+2, res+2), (2, res+2), (res+2, 2).  The diagonals res+1 .. res+3 are the gutter a bilinear lookup
 *                along either hypotenuse can touch: they are filled by extrapolation, not left grey.  uv returns the corner texels as
 *                (column, row), cell origin added; an untextured triangle gets the centre texel (B / 2, B / 2) of cell 0 three
 *                times.  Texels of no honoured triangle are 128: cell 0, the right margin, the cells behind the last, the upper half
 *                of the last cell when n_textured is odd.
 *     TEXEL      (i, j) of a triangle labelled v with (sx_m, sy_m, d_m) of its vertices m = 0, 1, 2 in v.  Integer weights: lower half
 *                n1 = i, n2 = j; upper half n1 = res+2-i, n2 = res+2-j; n0 = res - n1 - n2 (negative in the gutter).  Then fp64, left
 *                to right, without contraction: a_m = (double)n_m (double)d_m; den = a0 + a1 + a2;
 *                xs = (a0 (double)sx0 + a1 (double)sx1 + a2 (double)sx2) / den, ys alike; x = xs / 256.0, y alike -- the
 *                perspective-correct position in the view, a homography of the planar triangle: the texel stands for the point
 *                (n0 X0 + n1 X1 + n2 X2) / res of the triangle in space, whose homogeneous image is sum n_m d_m (x_m, y_m, 1).  (The
 *                weights are n_m d_m, not n_m / d_m: the reciprocal is the render's direction, from a point of the screen back to
 *                the surface.)  If den is not finite or <= 0, or x or
 *                y is NaN, or the view is narrower or lower than 2 pixels, the texel is 128 grey.  Otherwise
 *                x = fmin(fmax(x, 0.0), (double)(W-1) - 1.0/256), y alike with H; ix = floor(x), fx = x - ix, iy and fy alike; per
 *                channel top = (1-fx) t00 + fx t10, bot = (1-fx) t01 + fx t11, c = (1-fy) top + fy bot with t00 the texel (ix, iy),
 *                t10 = (ix+1, iy), t01 = (ix, iy+1), t11 = (ix+1, iy+1); the byte is (uint8)floor(c + 0.5).
 * LIMITS: n_v, n_t in 0 .. 2^30.  Device memory per call: the render's per-vertex buffers (16 bytes a vertex and the 12 of the input; 8
 * more with visible); per triangle the 12 of the input and, for the labelling, 12 (label, area), for the texturing 52 (label, the nine
 * numbers, flag, scan, list) and 24 for uv; the atlas, 3 bytes a texel.
 * MVS_ERR_ARG, checked in this order before the handle is read: the struct NULL; res outside 1..256; width outside res + 3 .. 32768; a
 * negative count or a count over the limit; verts NULL with n_v > 0; tris NULL with n_t > 0; label NULL with n_t > 0;
 * (mvs_engine_mesh_texture: height or n_textured NULL; a negative cap_h;) no engine.  MVS_ERR_STATE: the views are not set, or a pass is
 * waiting for its commit.  Then MVS_ERR_ARG after a validating pass on the device: an id outside 0 .. n_v - 1, or (mvs_engine_mesh_texture)
 * a label outside -1 .. nviews - 1.  MVS_ERR_HIP: an allocation or copy failed.
 * WHAT THE TEXTURING DOES NOT DO: seam-aware labelling (an MRF over neighbouring triangles) (since f-14: mvskit_seams.h); colour
 * levelling across seams (since f-14: mvskit_seams.h); per-triangle size classes or chart packing (res is one number per call; the meshes made here are near-uniform); level-0 texels when
 * m_level > 0; masks; per-pixel occlusion inside a triangle (visibility is per vertex, as in the render); a variant sharded over GPUs. */
#ifndef MVSKIT_TEXTURE_H
#define MVSKIT_TEXTURE_H

#include "mvskit_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mvs_mesh_texturing {
    int32_t res;        /* texels along a triangle's leg in the atlas, 1..256 */
    int32_t width;      /* atlas width in texels, res + 3 .. 32768 */
    int32_t front_only; /* != 0: a view counts only for triangles that face it */
    int32_t pad;
} mvs_mesh_texturing; /* 16 bytes */
void mvs_default_mesh_texturing(mvs_mesh_texturing* x); /* res 8, width 4096, front_only 1 */

int mvs_engine_mesh_face_views(mvs_engine* e, const mvs_mesh_texturing* x, int64_t n_v, const float* verts, int64_t n_t, const int32_t* tris,
                               const uint64_t* visible /* [n_v] or NULL */, int32_t* label /* [n_t] */, int64_t* area /* [n_t] or NULL */,
                               int64_t* n_faces /* [nviews] or NULL */);
int mvs_engine_mesh_texture(mvs_engine* e, const mvs_mesh_texturing* x, int64_t n_v, const float* verts, int64_t n_t, const int32_t* tris,
                            const int32_t* label /* [n_t] */, int64_t cap_h, uint8_t* rgb /* [cap_h][width][3] or NULL */,
                            int32_t* uv /* [n_t][3][2] texel (column, row) of each corner, or NULL */, int64_t* height, int64_t* n_textured);

#ifdef __cplusplus
}
#endif
#endif /* MVSKIT_TEXTURE_H */
