// mvs_camera.cuh -- the camera of a view (image/camera.cpp) and what Optim and PatchManager derive from it alone: projection and
// unprojection, the unit of a point, its cell, the patch axes, the robust form of an INCC.  (half_bcast_f: mvs_wave.cuh.)
#pragma once
#include <limits.h>
#include "mvs_types.h"
#include "mvs_math.cuh"
#include "mvs_wave.cuh"

namespace mvsdev {

// ------------------------------------------------------------------ camera (image/camera.cpp)
// Camera::project, camera.cpp:310-326
DEV F3 project(const DView* vw, F4 X, int level) {
    const float* P = vw->P[level];
    float r0 = fma_(P[3], X.w, fma_(P[2], X.z, fma_(P[1], X.y, P[0] * X.x)));
    float r1 = fma_(P[7], X.w, fma_(P[6], X.z, fma_(P[5], X.y, P[4] * X.x)));
    float r2 = fma_(P[11], X.w, fma_(P[10], X.z, fma_(P[9], X.y, P[8] * X.x)));
    if (r2 <= 0.0f) return {-65535.0f, -65535.0f, -1.0f};
    const float lo = (float)(INT_MIN + 3.0f), hi = (float)(INT_MAX - 3.0f);
    const float inv = rcp_rn(r2);
    F3 ic{r0 * inv, r1 * inv, 1.0f};
    ic.x = fmaxf(lo, fminf(hi, ic.x));
    ic.y = fmaxf(lo, fminf(hi, ic.y));
    return ic;
}
// Camera::project on a projection matrix held in registers, without a branch (same values as project())
DEV F3 project_regs(const float (&P)[12], F4 X) {
    const float r0 = fma_(P[3], X.w, fma_(P[2], X.z, fma_(P[1], X.y, P[0] * X.x)));
    const float r1 = fma_(P[7], X.w, fma_(P[6], X.z, fma_(P[5], X.y, P[4] * X.x)));
    const float r2 = fma_(P[11], X.w, fma_(P[10], X.z, fma_(P[9], X.y, P[8] * X.x)));
    const float lo = (float)(INT_MIN + 3.0f), hi = (float)(INT_MAX - 3.0f);
    const float inv = rcp_rn(r2);  // r2 <= 0 is replaced below whatever this gave
    F3 ic{fmaxf(lo, fminf(hi, r0 * inv)), fmaxf(lo, fminf(hi, r1 * inv)), 1.0f};
    if (r2 <= 0.0f) ic = {-65535.0f, -65535.0f, -1.0f};
    return ic;
}
DEV void load_P(const DView* vw, int level, float (&P)[12]) {
#pragma unroll
    for (int k = 0; k < 12; ++k) P[k] = vw->P[level][k];
}
// Camera::unproject at m_level, camera.cpp:329-337
DEV F4 unproject(const DView* vw, F3 ic, int level) {
    const float* P = vw->P[level];
    const float* M = vw->Minv;
    F3 b{ic.x - P[3], ic.y - P[7], ic.z - P[11]};
    return {fma_(M[2], b.z, fma_(M[1], b.y, M[0] * b.x)), fma_(M[5], b.z, fma_(M[4], b.y, M[3] * b.x)),
            fma_(M[8], b.z, fma_(M[7], b.y, M[6] * b.x)), 1.0f};
}
// Optim::getUnit, optim.cpp:34-41 (2 * fz * 2^level is exact, so one fp32 division; see the oracle)
DEV float get_unit(const DParams& prm, const DView* vw, F4 coord) {
    const float fz = norm4(sub4(coord, ld4(vw->center)));
    const float ips = vw->ipscale;
    if (ips == 0.0f) return 1.0f;
    return div_rn(2.0f * fz * (float)(1 << prm.level), ips);
}
// the same for a caller that has loaded the view's centre and ipscale with its other constants
// (get_unit keeps its own lines and compute_weights spells the expression out: through this helper the code of the kernels that sample moves)
DEV float unit_at(const DParams& prm, F4 ctr, float ips, F4 coord) {
    float u = 1.0f;
    if (ips != 0.0f) u = div_rn(2.0f * norm4(sub4(coord, ctr)) * (float)(1 << prm.level), ips);
    return u;
}
// PatchManager::setGrids cell rule, patch_manager.cpp:241-250
DEV void cell_of(const DParams& prm, const DView* vw, F4 coord, int& ix, int& iy) {
    float P[12];
    load_P(vw, prm.level, P);
    const F3 ic = project_regs(P, coord);
    ix = ((int)floorf(ic.x + 0.5f)) / prm.csize;
    iy = ((int)floorf(ic.y + 0.5f)) / prm.csize;
}
// Optim::getPAxes, optim.cpp:67-84 (the view's constants are loaded once, up front).
// Every caller hands in a patch that is the same in all 16 lanes of a row (one patch per wave in the single evaluations, a proposal per
// row in the refinement steps, a patch per 16 / 32 / 64 lanes in Filter::filterExact).  The three projections of the reference view --
// of the patch's centre and of the centre moved along either axis -- are independent, so lanes 0, 1, 2 of every row take one each
// (the other lanes repeat the centre's), the two distances and their reciprocals come out of ONE norm / division sequence in lanes 1
// and 2, and the row reads them back with row broadcasts (DPP row_newbcast, no LDS): one projection, one square root and one division
// per step where each lane used to run three, two and two.  The point a lane projects is coord + a px + b py with (a, b) = (0, 0),
// (1, 0) or (0, 1): fma(b, py, fma(a, px, coord)) is coord, RN(coord + px) or RN(coord + py) exactly -- the reference's coord + pxaxis.
template <bool PAIR = false>
DEV void get_paxes(const DParams& prm, const DView* vw, F4 coord, F4 normal, F4& px, F4& py) {
    const F4 ctr = ld4(vw->center);
    const float ips = vw->ipscale;
    const F3 xax = ld3(vw->xaxis);
    float P[12];
    load_P(vw, prm.level, P);
    const float pscale = unit_at(prm, ctr, ips, coord);
    F3 n3{normal.x, normal.y, normal.z};
    F3 y3 = cross3(n3, xax);
    y3 = nrm3(y3);
    F3 x3 = cross3(y3, n3);
    px = {x3.x * pscale, x3.y * pscale, x3.z * pscale, 0.0f};
    py = {y3.x * pscale, y3.y * pscale, y3.z * pscale, 0.0f};
    const int j = lane_id() & (PAIR ? 7 : 15);
    const float a = j == 1 ? 1.0f : 0.0f, b = j == 2 ? 1.0f : 0.0f;
    const F4 X{fma_(b, py.x, fma_(a, px.x, coord.x)), fma_(b, py.y, fma_(a, px.y, coord.y)), fma_(b, py.z, fma_(a, px.z, coord.z)), coord.w};
    const F3 ic = project_regs(P, X);
    const F3 c0{half_bcast_f<0, PAIR>(ic.x), half_bcast_f<0, PAIR>(ic.y), half_bcast_f<0, PAIR>(ic.z)};
    const float inv = rcp_rn(norm3(sub3(ic, c0)));  // lane 1: 1 / xdis, lane 2: 1 / ydis (lane 0 and the rest: 1 / 0, never read)
    px = scl4(px, half_bcast_f<1, PAIR>(inv));
    py = scl4(py, half_bcast_f<2, PAIR>(inv));
}
DEV float robustincc(float incc) { return div_rn(incc, 1 + 3 * incc); }
DEV float unrobustincc(float r) { return div_rn(r, 1 - 3 * r); }

}  // namespace mvsdev
