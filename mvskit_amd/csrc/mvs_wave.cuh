// mvs_wave.cuh -- what the 64 lanes of a wave exchange without memory: lane reads (v_readlane / v_readfirstlane), ballots and the masks of
// a view list, the DPP butterflies (sum, minimum, pick-the-smallest), the row broadcasts and ds_bpermute.
#pragma once
#include <hip/hip_runtime.h>
#include "mvs_types.h"
#include "mvs_math.cuh"

namespace mvsdev {

DEV int lane_id() { return (int)(threadIdx.x & 63u); }
DEV int rli(int x, int l) { return __builtin_amdgcn_readlane(x, l); }
DEV float rlf(float x, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), l)); }
DEV int rfl(int x) { return __builtin_amdgcn_readfirstlane(x); }
DEV unsigned long long ballot(bool p) { return __ballot(p); }
DEV double rld(double x, int l) {
    const long long b = __double_as_longlong(x);
    const unsigned lo = (unsigned)rli((int)(b & 0xffffffffll), l), hi = (unsigned)rli((int)(b >> 32), l);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
DEV float rff(float x) { return __int_as_float(rfl(__float_as_int(x))); }
// one bit per entry of a view list: 32 bits serve the 16- and 32-view builds, the 64-view build needs all 64 lanes
#if MVS_LISTCAP > 32
typedef unsigned long long vmask_t;
DEV int vpop(vmask_t m) { return __popcll(m); }
#define MVS_VBITS 64
#else
typedef unsigned vmask_t;
DEV int vpop(vmask_t m) { return __popc(m); }
#define MVS_VBITS 32
#endif
DEV vmask_t vballot(bool p) { return (vmask_t)__ballot(p); }

// ------------------------------------------------------------------ wave butterflies
// sum over the 64 lanes, pairing order 1,2,4,8,16,32; every lane ends with the same bits.
template <int CTRL> DEV float dpp_f(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf, 0xf, false));
}
DEV float wave_sum(float x) {
    x = x + dpp_f<0xB1>(x);   // quad_perm [1,0,3,2]   : i ^ 1
    x = x + dpp_f<0x4E>(x);   // quad_perm [2,3,0,1]   : i ^ 2
    x = x + dpp_f<0x141>(x);  // row_half_mirror       : other quad of the 8 (== i ^ 4 once quads are uniform)
    x = x + dpp_f<0x140>(x);  // row_mirror            : other half of the row of 16 (== i ^ 8)
    // every row of 16 now holds its row sum r0..r3 in all of its lanes.  i ^ 16 pairs rows (0,1) and (2,3), i ^ 32 the
    // halves: (r0 + r1) + (r2 + r3).  row_bcast15 into rows 1 and 3 gives r1 + r0 and r3 + r2, row_bcast31 into rows 2,3
    // gives (r3 + r2) + (r1 + r0) in row 3 -- the same sums (fp addition commutes), 3 instructions, no LDS pipeline.
    // Only lane 63 is read, so the broadcasts may run on every row (rows without a source lane add 0: bound_ctrl), which
    // lets each step be a single v_add_f32_dpp.
    x = x + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x142, 0xf, 0xf, true));  // row_bcast:15
    x = x + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x143, 0xf, 0xf, true));  // row_bcast:31
    return rlf(x, 63);
}
// (bound_ctrl form of a DPP read: lanes without a source read 0)
template <int CTRL> DEV float dpp0_f(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf, 0xf, true));
}
DEV float wave_min(float x) {
    x = fminf(x, dpp_f<0xB1>(x));
    x = fminf(x, dpp_f<0x4E>(x));
    x = fminf(x, dpp_f<0x141>(x));
    x = fminf(x, dpp_f<0x140>(x));
    return fminf(fminf(rlf(x, 0), rlf(x, 16)), fminf(rlf(x, 32), rlf(x, 48)));
}
// Picks the smallest remaining: the lane of `active` (not empty) whose x is smallest, the lowest lane among equals, taken out of `active`;
// where every remaining x is a NaN, the first remaining lane.  (sort_images spells the step out: with the helper the sweep's machine code changes.)
DEV int wave_pick_min(float x, int lane, unsigned long long& active) {
    const bool act = (active >> lane) & 1ull;
    const float m = wave_min(act ? x : __int_as_float(0x7f800000));
    const unsigned long long eq = ballot(act && x == m);
    const int sel = eq ? __ffsll((long long)eq) - 1 : __ffsll((long long)active) - 1;
    active &= ~(1ull << sel);
    return sel;
}

// ------------------------------------------------------------------ row broadcasts (DPP row_newbcast, no LDS) and ds_bpermute
template <int LANE> DEV float row_bcast_f(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x150 + LANE, 0xf, 0xf, false));  // row_newbcast:LANE
}
// PAIR (the two-candidate refinement steps, refine_patch_pair): a row holds TWO patches, one per half of 8 lanes (vw may then differ between
// the halves); lanes 8 s + 0..2 take the three projections of half s and each half reads its own back -- the same row broadcasts, written
// into one half of the row at a time (DPP bank mask: banks 0-1 are lanes 0..7 of a row, banks 2-3 lanes 8..15).
template <int LANE, int BANKS> DEV float row_bcast_banks_f(float old, float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(x), 0x150 + LANE, 0xf, BANKS, false));
}
template <int LANE, bool PAIR> DEV float half_bcast_f(float x) {
    if constexpr (PAIR) return row_bcast_banks_f<8 + LANE, 0xC>(row_bcast_banks_f<LANE, 0x3>(x, x), x);
    else return row_bcast_f<LANE>(x);
}
DEV float bperm_f(int addr, float x) { return __int_as_float(__builtin_amdgcn_ds_bpermute(addr, __float_as_int(x))); }

}  // namespace mvsdev
