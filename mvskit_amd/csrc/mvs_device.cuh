// mvs_device.cuh -- the patch arithmetic of the PatchMatch-MVS engine for gfx950 (wave64): the device functions of a patch, by concern.
//
// Execution model: ONE 64-lane wavefront works on one patch / one destination cell.  Control flow is
// wave-uniform.  Three lane layouts coexist in registers:
//   * class lanes: lane 16 r + c holds samples c, c + 16, c + 32 of the 7x7 texture window (optim.cpp:835-842) its 16-lane
//     row works on -- a proposal in a refinement step, a view in a single evaluation; sums over a window are lane sums, a
//     DPP row tree (pairing 1, 2, 4, 8) and the window's 49th sample, taken by the lane that owns the sampling frame;
//   * view lanes: lane j holds element j of a per-view array (Patch::m_images[j], its ray, unit, INCC ...),
//     read back with v_readlane when a loop needs element j uniformly;
//   * frame lanes: lane 16*g + i holds the sampling frame of view i for proposal g (g < 4): the four
//     proposals of one refinement step share one pass of decode / getPAxes / projection arithmetic.
// Per-view scalars that need a square root or a division (msd, 1/msd, robust INCC) are gathered into view
// lanes first, so one vector instruction sequence serves all views of an evaluation.
// Arithmetic follows DESIGN.md "engine arithmetic": fp32, no implicit contraction (-ffp-contract=off), dot
// products as left-to-right fmaf chains, own polynomial sin/cos/asin/acos/atan -- the same operation order
// the CPU oracle's TREE64 mode uses, so results can be compared bit for bit.
#pragma once
#include "mvs_math.cuh"    // vectors, exact sqrt / rcp / div, the pm_* libm subset, the RNG
#include "mvs_wave.cuh"    // lane reads, ballots, DPP butterflies, row broadcasts
#include "mvs_camera.cuh"  // project / unproject, unit, cell, patch axes
#include "mvs_sample.cuh"  // frames, WaveCtx, class-lane sampling, the four proposals of a step
#include "mvs_eval.cuh"    // the single evaluation, the Gram tiles
#include "mvs_cand.cuh"    // Cand, INCC / NCC, view lists, preProcess, postProcess, records
#include "mvs_refine.cuh"  // refine_patch, refine_patch_pair, refine_patch_simplex
