// mvs_sweep.cuh (part of the unit mvs_patch.hip) -- Propagate::run on the device: the job lists, the sweep (sweep_cell in a grid of resident waves) with its retry
// tier, the choice of a launch's kernel variant, and the commit of what a pass staged; kernels first, their launchers behind them.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstddef>
#include <type_traits>
#include "mvs_patch_common.cuh"
#include "mvs_check.cuh"
#include "mvs_kernels.h"

using namespace mvsdev;

// m_pgrids entry `pos` (an offset into the index): the fields the sweep reads of its own and its source cells
DEV int pgrid_id(const DParams& prm, csr_off_t pos) {
    return prm.csr_id32[pos];
}
DEV float pgrid_ncc(const DParams& prm, csr_off_t pos) {
    return prm.csr_key[pos].ncc;
}
DEV int pgrid_ref(const DParams& prm, csr_off_t pos) {
    return prm.csr_key[pos].ref;
}
// =================================================================== K4: the sweep
// One wavefront at a time per destination cell of the pass colour.  Propagate::propagatePmImage (propagate.cpp:72-124)
// turned inside out: the cell gathers from the cell above/below and the cell beside it, in the order the
// raster sweep would reach them, and runs Propagate::propagatePatch (propagate.cpp:126-218) on its own list.
DEV bool rank_before(float na, int a, float nb, int b) { return (na != nb) ? (na > nb) : (a < b); }
// job -> (swept view, destination cell): one job per (view, row, half column) of the pass colour
DEV void job_cell(const DParams& prm, const SweepArgs& a, int64_t job, int& v, int& cx, int& cy) {
    int s = 0;
    while (s + 1 < a.nsweep_views && job >= a.job_base[s + 1]) ++s;
    v = a.sweep_views[s];
    const int gw = (prm.views + v)->gw, halfw = (gw + 1) / 2;
    const int local = (int)(job - a.job_base[s]);
    cy = local / halfw;
    cx = 2 * (local % halfw) + ((a.colour + cy) & 1);
}
// The entries of a job's source lists that start trials in sweep_cell -- 0 for a job without a destination cell (the ghost job at
// cx == gw of an odd-width grid, a job outside the grid) --: of the first min(csr_cnt, MVS_CAPMAX) entries of the cell above/below
// and the cell beside, those whose reference view is the swept view; with view propagation, those of the cell's own list whose
// reference view is another.  *dest = the destination cell's index entry (-1 without a cell).  A lane per job (k_job_list, k_job_work).
DEV int job_trial_sources(const DParams& prm, const SweepArgs& a, int64_t job, int* dest) {
    int v, cx, cy;
    job_cell(prm, a, job, v, cx, cy);
    const DView* vw = prm.views + v;
    const int gw = vw->gw, gh = vw->gh;
    *dest = -1;
    if (cx >= gw || cy >= gh) return 0;
    *dest = vw->cell_base + cy * gw + cx;
    const int sxs[3] = {cx, cx - a.inc, cx}, sys[3] = {cy - a.inc, cy, cy};
    const int nsrc = prm.view_propagation ? 3 : 2;
    int n = 0;
    for (int k = 0; k < nsrc; ++k) {
        if (sxs[k] < 0 || gw <= sxs[k] || sys[k] < 0 || gh <= sys[k]) continue;
        const int g = vw->cell_base + sys[k] * gw + sxs[k];
        const csr_off_t sb = prm.csr_start[g];
        const int sn = min(prm.csr_cnt[g], MVS_CAPMAX);
        for (int j = 0; j < sn; ++j) n += ((pgrid_ref(prm, sb + j) == v) != (k == 2)) ? 1 : 0;
    }
    return n;
}
// Work proxy of a job, for cutting the job sequence into ranges of equal WORK (multi-GPU: every rank holds the same index,
// computes the same proxy and finds the same cuts).  A job runs max_propag trials per source entry whose reference view is
// the swept view (propagate.cpp:102-108); a trial into a cell that still has room runs the whole pipeline (preProcess,
// refinePatch's 25 evaluations, postProcess, check), a trial into a full cell one evaluation and, mostly, the pre-filter
// (propagate.cpp:166-173); about four trials in five that run the pipeline add a patch to the cell.
// mode 1: source entries alone; mode 2: 32 per expected pipeline trial + 2 per expected pre-filter trial.
__global__ void k_job_work(DParams prm, SweepArgs a, int mode, int shift, int32_t* __restrict__ work) {
    const int64_t job = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (job >= a.njobs) return;
    int dest;
    const int n = job_trial_sources(prm, a, job, &dest);
    int w = 0;
    if (dest >= 0) {
        if (mode == 1) w = n;
        else {
            const int trials = n * prm.max_propag;
            const int room = max(prm.cap - prm.csr_cnt[dest], 0);
            const int full = min(trials, (room * 5 + 3) / 4);
            w = 32 * full + 2 * (trials - full);
        }
    }
    work[job] = (w + (1 << shift) - 1) >> shift;
}
// cuts[r] = first job whose inclusive work prefix exceeds total * r / n (r = 1 .. n-1): exactly one job qualifies per r
__global__ void k_job_cuts(const int32_t* __restrict__ scan, int64_t njobs, int n, int32_t* __restrict__ cuts) {
    const int64_t job = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (job >= njobs) return;
    const long long total = scan[njobs], p0 = scan[job], p1 = scan[job + 1];
    if (p0 == p1) return;
    for (int r = 1; r < n; ++r) {
        const long long target = total * r / n;
        if (p0 <= target && target < p1) cuts[r] = (int32_t)job;
    }
}

#ifndef MVS_XCD_CHUNK
#define MVS_XCD_CHUNK 128
#endif
// The sweep's job lists (sweep_resident).  The launch's job range [job_lo, job_hi) is cut into chunks of MVS_XCD_CHUNK consecutive
// jobs, chunk c belongs to queue c % 8; the flags of the jobs are laid out QUEUE-MAJOR -- queue q owns the slots [q seg, (q + 1) seg),
// seg = its chunks rounded up over the queues, times MVS_XCD_CHUNK; a slot beyond job_hi has no job -- so that ONE exclusive scan of
// the flags gives every listed job its place in a list that holds queue 0's jobs, then queue 1's, ..., each in ascending job order.
DEV int64_t list_slot_job(const SweepArgs& a, int64_t slot, int seg) {
    const int64_t q = slot / seg, r = slot % seg;
    return a.job_lo + ((r / MVS_XCD_CHUNK) * MVS_SWEEP_QUEUES + q) * MVS_XCD_CHUNK + r % MVS_XCD_CHUNK;
}
// A thread per job of [0, njobs) clears its job_nstage (a job that is not listed stages nothing: other shards' jobs, jobs without a
// trial); a thread per slot flags the slot's job if sweep_cell would run a trial for it (job_trial_sources).
__global__ void k_job_list(DParams prm, SweepArgs a, int seg, int32_t* __restrict__ flags) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < a.njobs) a.job_nstage[t] = 0;
    if (t >= (int64_t)MVS_SWEEP_QUEUES * seg) return;
    const int64_t job = list_slot_job(a, t, seg);
    int dest = -1;
    const int n = job < a.job_hi ? job_trial_sources(prm, a, job, &dest) : 0;
    flags[t] = n > 0 ? 1 : 0;
#ifdef MVS_JOBLIST_COUNTS
    // diagnostic build: how many jobs the test of the former take passed (a destination cell and ANY entry in a source list), and how
    // many are listed, into the stage words of counter slot 0 (the host prints them per launch)
    bool any = false;
    if (dest >= 0) {
        int v, cx, cy;
        job_cell(prm, a, job, v, cx, cy);
        const DView* vw = prm.views + v;
        const int sxs[3] = {cx, cx - a.inc, cx}, sys[3] = {cy - a.inc, cy, cy};
        for (int k = 0; k < (prm.view_propagation ? 3 : 2); ++k)
            if (0 <= sxs[k] && sxs[k] < vw->gw && 0 <= sys[k] && sys[k] < vw->gh) any |= prm.csr_cnt[vw->cell_base + sys[k] * vw->gw + sxs[k]] > 0;
    }
    const unsigned long long m_any = __ballot(any), m_listed = __ballot(n > 0);
    if ((threadIdx.x & 63) == 0) {
        if (m_any) atomicAdd(&a.counters->stage[0], (unsigned long long)__popcll(m_any));
        if (m_listed) atomicAdd(&a.counters->stage[1], (unsigned long long)__popcll(m_listed));
    }
#endif
}
// list[scan[slot]] = the job of every flagged slot (scan = the exclusive scan of the flags); bounds[q] = where queue q's jobs begin,
// bounds[8] = the number of jobs listed
__global__ void k_job_scatter(SweepArgs a, int seg, const int32_t* __restrict__ scan, int32_t* __restrict__ list, int32_t* __restrict__ bounds) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nslots = (int64_t)MVS_SWEEP_QUEUES * seg;
    if (t >= nslots) return;
    const int32_t pos = scan[t];
    if (t % seg == 0) bounds[t / seg] = pos;
    if (t == nslots - 1) bounds[MVS_SWEEP_QUEUES] = scan[nslots];
    if (scan[t + 1] != pos) list[pos] = (int32_t)list_slot_job(a, t, seg);
}

// BIG = false: the sweep proper (k_sweep).  BIG = true: the second tier (k_sweep_retry) -- the few destination cells in which an
// Optim::check met a neighbourhood larger than the wave's LDS id set run again, from the start, with a global-memory table for such
// checks (mvs_check.cuh).  A cell of the first launch that meets such a check gives up: nothing it staged counts (job_nstage = 0)
// and its counters are dropped.  The cells of a colour pass are independent of each other and a cell's run is deterministic (RNG
// keyed by iteration, view, cell, source slot, trial), so the second run repeats the first up to the point where it gave up -- the
// pool patches the first run evicted until then are exactly the first evictions of the second: their kill flags may stand.
#ifdef MVS_STAGE_TIMING
#define ST_NOW() ((unsigned long long)__builtin_amdgcn_s_memtime())
#define ST_ADD(k, t0) { const unsigned long long t1_ = ST_NOW(); st_acc[k] += t1_ - (t0); (t0) = t1_; }
#else
#define ST_ADD(k, t0)
#endif
// The work counts of a wave, summed over its cells (wave-uniform: scalar registers) and added into one counter slot before it exits
struct SweepAcc {
    unsigned cand, pref, patch, f0, f1, ins, rep;
    unsigned long long evals, view_evals;
    unsigned pair[6];  // DCounters::pair
    unsigned skip;     // DCounters::repeats[0]
#ifdef MVS_STAGE_TIMING
    unsigned long long stage[16];
#endif
};
DEV SweepAcc sweep_acc_zero() {
    SweepAcc acc;
    acc.cand = acc.pref = acc.patch = acc.f0 = acc.f1 = acc.ins = acc.rep = 0u;
    acc.evals = acc.view_evals = 0ull;
    for (int k = 0; k < 6; ++k) acc.pair[k] = 0u;
    acc.skip = 0u;
#ifdef MVS_STAGE_TIMING
    for (int k = 0; k < 16; ++k) acc.stage[k] = 0ull;
#endif
    return acc;
}
DEV void sweep_acc_flush(const SweepArgs& a, const SweepAcc& acc, unsigned slot) {  // one lane
    DCounters* C = a.counters + slot;  // partial sums, added up by the host: the waves of a launch on ONE cache line queue up
    if (acc.cand) atomicAdd(&C->candidates, (unsigned long long)acc.cand);
    if (acc.pref) atomicAdd(&C->prefiltered, (unsigned long long)acc.pref);
    if (acc.patch) atomicAdd(&C->patches, (unsigned long long)acc.patch);
    if (acc.f0) atomicAdd(&C->fail0, (unsigned long long)acc.f0);
    if (acc.f1) atomicAdd(&C->fail1, (unsigned long long)acc.f1);
    if (acc.ins) atomicAdd(&C->inserted, (unsigned long long)acc.ins);
    if (acc.rep) atomicAdd(&C->replaced, (unsigned long long)acc.rep);
    if (acc.evals) atomicAdd(&C->evals, acc.evals);
    if (acc.view_evals) atomicAdd(&C->view_evals, acc.view_evals);
    for (int k = 0; k < 6; ++k) if (acc.pair[k]) atomicAdd(&C->pair[k], (unsigned long long)acc.pair[k]);
    if (acc.skip) atomicAdd(&C->repeats[0], (unsigned long long)acc.skip);
#ifdef MVS_STAGE_TIMING
    for (int k = 0; k < 12; ++k) if (acc.stage[k]) atomicAdd(&C->stage[k], acc.stage[k]);
    atomicMax(&C->stage[12], acc.stage[12]); atomicMax(&C->stage[13], acc.stage[13]);
    atomicAdd(&C->stage[14], acc.stage[14]); atomicAdd(&C->stage[15], acc.stage[15]);  // inside postProcess: setRefImage's pair sums and choice
#endif
}
// The ONE argument of every sweep kernel, and how the sweep reads it.  DParams and SweepArgs are ~230 dwords against 104 scalar
// registers: taken by value and read as plain kernel arguments, every field is fetched once at kernel entry and lives across the
// whole cell loop -- 336 scalars spilled into vector lanes, 779 v_readlane_b32 to bring them back, most of them in the stages around
// the refinement (profiles/r26_codeobj_stage_args.txt).  The sweep instead reads the fields where it uses them, from the
// kernel-argument segment itself (constant address space: a uniform read is a scalar load, which takes no vector issue slot), through
// a pointer that stage_args makes opaque at a stage boundary: a load cannot be hoisted above the empty asm that defines the
// pointer it reads through, so a field's live range ends with the stage that read it.  The shared device functions still take
// `const DParams&`; inlined, their reads resolve to the constant address space behind the reference.
struct SweepKArgs {
    DParams prm;
    SweepArgs a;
    int32_t nretry;     // k_sweep_retry, k_sweep_retry_simplex: the cells handed to the second tier
    int32_t max_evals;  // the CONVERGED refiner (k_sweep_simplex, k_sweep_retry_simplex)
    float xtol;
};
// the kernel-argument segment IS this struct: one argument, at offset 0, in its C++ layout
static_assert(std::is_standard_layout<SweepKArgs>::value && std::is_trivially_copyable<SweepKArgs>::value, "SweepKArgs is read from the kernel-argument segment as it lies in memory");
static_assert(offsetof(SweepKArgs, prm) == 0 && offsetof(SweepKArgs, a) == sizeof(DParams) && sizeof(DParams) % 8 == 0, "DParams, then SweepArgs");
static_assert(sizeof(SweepKArgs) <= 4096, "a kernel-argument segment holds at most 4 KiB");
typedef const __attribute__((address_space(4))) SweepKArgs* SweepKPtr;
DEV SweepKPtr sweep_kargs() { return (SweepKPtr)__builtin_amdgcn_kernarg_segment_ptr(); }
// the arguments for ONE stage: what is read through the result is loaded after this point and is dead when the stage is
DEV const SweepKArgs& stage_args(SweepKPtr p) {
    asm volatile("" : "+s"(p));
    return *(const SweepKArgs*)p;
}
// ... and without a boundary: the stages of a trial up to and including the refinement read through the kernel's own pointer.  Their
// loads stay where the fields are used all the same (nothing proves the segment dereferenceable, so nothing is hoisted), and with a
// boundary around each of them the pair step loop reloads 9 spilled scalars instead of 2.  With no boundary anywhere the kernel spills
// 22 VGPRs where the parent spilled 20; with the boundaries of sweep_cell, sweep_resident and the retry loops 15
// (profiles/r26_codeobj_stage_args.txt: the three granularities side by side).
DEV const SweepKArgs& kernel_args(SweepKPtr p) { return *(const SweepKArgs*)p; }
// One destination cell: `job` has a cell and a source entry that starts a trial (it is listed: k_job_list), job_nstage[job] is 0.  The wave comes here cell after cell
// (the LDS of the previous cell is dead: the caller puts a barrier in between): everything a cell keeps is set up here, and what it
// counted goes into `acc` when it is done -- nothing of a cell that gives up.
// SIMPLEX = true: the refinement is refine_patch_simplex with max_evals / xtol (k_sweep_simplex, k_sweep_retry_simplex: the CONVERGED
// refiner of mvs_engine_set_refiner); the default kernels keep the halving search and never read the two fields.
template <bool BIG, bool SIMPLEX = false, class WC>
DEV void sweep_cell(const SweepKPtr kp, WC& wc, SweepAcc* acc, const int64_t job, int* s_scratch, int* s_pend, float* s_texs, int* big_table) {
#ifdef MVS_STAGE_TIMING
    unsigned long long st_acc[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const unsigned long long st_begin = ST_NOW();
    unsigned long long st_t = st_begin;
    for (int k = 0; k < 8; ++k) wc.st_acc[k] = 0;
#endif
    // ---- stage: the cell's prologue.  What the cell keeps of the arguments: its place (v, cx, cy, the grid), inc, the number of sources.
    int v, cx, cy, gw, gh, cell, inc, nsrc;
    const DView* vw;
    float icx, icy;
    // live list of this cell as view-lane arrays: lane k holds entry k (sorted: ncc desc, id asc)
    int L_id = -1;
    float L_ncc = 0.0f;
    int L_n = 0;
    {
        const SweepKArgs& K = stage_args(kp);
        const DParams& prm = K.prm;
        job_cell(prm, K.a, job, v, cx, cy);
        vw = prm.views + v;
        gw = vw->gw; gh = vw->gh;
        cell = cy * gw + cx;
        inc = K.a.inc;
        const int g = vw->cell_base + cell;
        const csr_off_t fb = prm.csr_start[g];
        L_n = min(prm.csr_cnt[g], MVS_CAPMAX);
        if (wc.lane < L_n) { L_id = pgrid_id(prm, fb + wc.lane); L_ncc = pgrid_ncc(prm, fb + wc.lane); }
        icx = (float)(prm.csize * (2 * cx + 1) - 1) / 2.0f; icy = (float)(prm.csize * (2 * cy + 1) - 1) / 2.0f;
        // sources: the cell above/below, the cell beside (propagate.cpp:104-108), and -- view propagation, the branch the
        // reference keeps commented out (propagate.cpp:110-120) -- this cell's own list: a patch of another reference view
        // that is listed here proposes itself with view v as the reference
        nsrc = prm.view_propagation ? 3 : 2;
    }
    wc.evals = 0; wc.view_evals = 0;
    const int sxs[2] = {cx, cx - inc}, sys[2] = {cy - inc, cy};
    unsigned n_cand = 0, n_pref = 0, n_patch = 0, n_f0 = 0, n_f1 = 0, n_ins = 0, n_rep = 0;
    int ns = 0;  // staged records of this job
    bool gave_up = false;
    // Two consecutive trials of the cell are refined TOGETHER where the second is certain to find room (refine_patch_pair): a candidate that
    // has passed preProcess waits in s_pend for the next one that does.  Everything after the refinement -- postProcess, Optim::check, the
    // staging slot, the live list -- then runs candidate by candidate in trial order, as if each had been refined in its turn.  When the
    // sources are through (the pass sidx == nsrc below) a candidate still waiting is finished alone.
    bool pend = false, pend_failed = false;  // a candidate waits; a trial that would have joined it failed generate / preProcess
    uint32_t pend_k3 = 0u;
    int pend_sz = 0;
    unsigned n_pair = 0, n_elig = 0, n_last = 0, n_noroom = 0, n_lost = 0, n_long = 0;  // DCounters::pair
    unsigned n_skip = 0;                                                                // DCounters::repeats[0]
    for (int sidx = 0; sidx <= nsrc; ++sidx) {
        const bool flush = sidx == nsrc;
        const int scx = sidx < 2 ? sxs[sidx] : cx, scy = sidx < 2 ? sys[sidx] : cy;
        if (!flush && (scx < 0 || gw <= scx || scy < 0 || gh <= scy)) continue;
        const int as_view = sidx == 2 ? v : -1;
        // the entries of the source list, a lane each, in ONE round trip (the walk used to read entry after entry: a dependent load
        // per entry, six in seven of them only to find another reference view); then the sources in list order
        int E_id = 0;
        bool E_take = false;
        if (!flush) {  // ---- stage: a source list
            const DParams& prm = kernel_args(kp).prm;
            const int g = vw->cell_base + scy * gw + scx;
            const csr_off_t sb = prm.csr_start[g];
            const int sn = min(prm.csr_cnt[g], MVS_CAPMAX);  // a trimmed list: at most MAX_NUM_OF_PATCHES <= 32 entries
            if (wc.lane < sn) { E_id = pgrid_id(prm, sb + wc.lane); E_take = (pgrid_ref(prm, sb + wc.lane) == v) != (sidx == 2); }
        }
        unsigned todo = flush ? (pend ? 1u : 0u) : (unsigned)ballot(E_take);
        while (todo) {
            const int n = __ffs((int)todo) - 1;
            todo &= todo - 1u;
            const DPatch* sp;
            int srcslot, ntrial;
            {
                const DParams& prm = kernel_args(kp).prm;
                sp = prm.pool + rli(E_id, n);
                srcslot = sidx * prm.cap + n;
                // ---- Propagate::propagatePatch, propagate.cpp:153-213
                ntrial = flush ? 1 : prm.max_propag;
            }
            for (int it = 0; it < ntrial; ++it) {
                ST_ADD(7, st_t)
                const int np = L_n;
                const uint32_t k1 = (uint32_t)v, k2 = (uint32_t)cell;  // (k0, the iteration, is read where a stage draws)
                uint32_t k3 = (uint32_t)(srcslot * 16 + it);
                Cand c;
                float keep_w = 0.0f;  // computeWeights of refinePatch, for the m_ncc postProcess takes from its first evaluation
                int worst = -1;
                int nfin = 1;         // candidates to finish now: this one, or the waiting one and this one
                if (!flush) {
                    float worst_ncc = 0.0f;
                    F3 ic;
                    bool full;  // the trial goes into a full cell
                    {   // ---- stage: the trial's image point
                        const SweepKArgs& K = kernel_args(kp);
                        const DParams& prm = K.prm;
                        full = np >= prm.cap;
                        if (!full) {
                            const uint32_t k0 = (uint32_t)K.a.iter;
                            const float ra = rng_uniform(prm.seed, k0, k1, k2, k3, 0) * (float)prm.csize;
                            const float rb = rng_uniform(prm.seed, k0, k1, k2, k3, 1) * (float)prm.csize;
                            ic = {icx + ra, icy + rb, 1.0f};
                        } else {
                            worst = rli(L_id, prm.cap - 1);
                            worst_ncc = rlf(L_ncc, prm.cap - 1);
                            const DPatch* wp = worst >= MVS_NEWBASE ? K.a.staging + (worst - MVS_NEWBASE) : prm.pool + worst;
                            ic = project(vw, ld4(wp->coord), prm.level);
                        }
                    }
                    // A trial into a FULL cell draws nothing before the refinement: what follows, up to and including preProcess, is a function
                    // of the source record, the worst patch and the index.  If it ends there it has staged nothing, the live list is what it
                    // was, and the `rest` trials of this source entry still to come would compute the same and end the same way: their counts
                    // (the evaluations included) are added here and they are not run.  (Nothing waits in such a cell: `pend` is false.)
                    const unsigned rest = full ? (unsigned)(ntrial - 1 - it) : 0u;
                    const unsigned ev0 = wc.evals, vev0 = wc.view_evals;
                    auto skip_rest = [&]() {
                        n_skip += rest;
                        wc.evals += rest * (wc.evals - ev0); wc.view_evals += rest * (wc.view_evals - vev0);
                        it += (int)rest;
                    };
                    {   // ---- stage: generate
                        Cand src;  // loaded per trial: its registers are free again during the refinement
                        load_cand(sp, wc, src);
                        const bool gen_ok = generate_patch(kernel_args(kp).prm, wc, s_scratch, src, ic, c, as_view, full);
                        ST_ADD(1, st_t)
                        if (!gen_ok) { pend_failed |= pend; skip_rest(); continue; }
                    }
                    ++n_cand;
                    if (full && c.ncc < worst_ncc) { ++n_pref; n_cand += rest; n_pref += rest; skip_rest(); continue; }
                    ++n_patch;
                    const int pre_r = pre_process(kernel_args(kp).prm, wc, s_scratch, c);  // ---- stage: preProcess
                    ST_ADD(2, st_t)
                    if (pre_r == -1) { ++n_f0; pend_failed |= pend; n_cand += rest; n_patch += rest; n_f0 += rest; skip_rest(); continue; }
                    const DParams& prm = kernel_args(kp).prm;
                    if (!pend && np + 1 < prm.cap) {
                        // Room for this trial AND the next: the next one, whatever becomes of this one, still takes the np < cap branch above and
                        // reads nothing of the live list before Optim::check -- it may be generated first and refined together with this one.
                        pend_store(s_pend, wc, c, 0.0f);
                        pend = true; pend_failed = false; pend_k3 = k3; pend_sz = min(prm.tau, c.nimg);
                        continue;
                    }
                    if (pend) nfin = 2;
                    else ++n_noroom;  // no guaranteed room for a partner
                } else {
                    pend_load(s_pend, wc, c, keep_w);  // nothing came to join the waiting candidate
                    k3 = pend_k3;
                    if (pend_failed) ++n_lost; else ++n_last;
                }
                bool paired = false;
                if (nfin == 2) {  // ---- stage: the refinement of a pair
                    // the waiting candidate is the earlier trial: it is finished first, this one takes its place in the stash meanwhile
                    const SweepKArgs& K = kernel_args(kp);
                    const DParams& prm = K.prm;
                    const bool fits = pend_sz <= 8 && min(prm.tau, c.nimg) <= 8;
                    if (!fits) n_long += 2;
                    else n_elig += 2;
                    if constexpr (!SIMPLEX) {
                        if (fits && K.a.pair) {
                            refine_patch_pair(prm, wc, s_pend, c, (uint32_t)K.a.iter, k1, k2, pend_k3, k3, keep_w);
                            paired = true;
                            n_pair += 2;
                        }
                    }
                    Cand first;
                    float first_w;
                    pend_load(s_pend, wc, first, first_w);
                    pend_store(s_pend, wc, c, keep_w);
                    c = first; keep_w = first_w;
                    const uint32_t t = k3; k3 = pend_k3; pend_k3 = t;
                }
                pend = false;
                for (int fi = 0; fi < nfin; ++fi) {
                    if (fi == 1) { pend_load(s_pend, wc, c, keep_w); k3 = pend_k3; }
                    if (!paired) {  // ---- stage: the refinement of one candidate
                        const SweepKArgs& K = kernel_args(kp);
                        if constexpr (SIMPLEX) (void)refine_patch_simplex(K.prm, wc, c, K.max_evals, K.xtol, &keep_w);
                        else refine_patch(K.prm, wc, c, (uint32_t)K.a.iter, k1, k2, k3, &keep_w);
                    }
                    ST_ADD(3, st_t)
                    int post_r;
                    {   // ---- stage: postProcess
                        const DParams& prm = stage_args(kp).prm;
                        const int tstride = prm.wsz;  // odd for 7x7 / 5x5 windows: the lane-per-pair reads of setRefImage fall in distinct banks
                        post_r = post_process(prm, wc, s_scratch, s_texs, tstride, c, keep_w, true);
                    }
                    ST_ADD(4, st_t)
                    if (post_r == -1) { ++n_f1; continue; }
                    {   // ---- stage: Optim::check, optim.cpp:292
                        const SweepKArgs& K = stage_args(kp);
                        const DParams& prm = K.prm;
                        if (prm.depth >= 2 && prm.enable_check) {
                            __syncthreads();
                            if (wc.lane < MVS_CAPMAX) s_scratch[wc.lane] = L_id;  // publish the live list of this cell
                            __syncthreads();
#ifdef MVS_STAGE_TIMING
                            const CheckCtx cx{K.a.staging, v, cell, L_n, s_scratch, st_acc};
#else
                            const CheckCtx cx{K.a.staging, v, cell, L_n, s_scratch, nullptr};
#endif
                            const int chk_r = check_patch<BIG>(prm, wc, cx, c, s_texs, K.a.error_flag, big_table);
                            ST_ADD(5, st_t)
                            if (!BIG && chk_r < 0) { gave_up = true; break; }  // the neighbourhood does not fit LDS: this cell goes to k_sweep_retry
                            if (chk_r) { ++n_f1; continue; }
                        }
                    }
                    // ---- stage: staging and insert
                    const SweepKArgs& K = stage_args(kp);
                    const DParams& prm = K.prm;
                    const SweepArgs& a = K.a;
                    // staging slot for the accepted patch
                    unsigned long long slot64 = 0;
                    if (wc.lane == 0) slot64 = atomicAdd(a.stage_counter, 1ull);
                    const int64_t slot = ((int64_t)rfl((int)(slot64 >> 32)) << 32) | (uint32_t)rfl((int)(slot64 & 0xffffffffull));
                    if (slot >= a.staging_cap || ns >= a.maxstage) {
                        if (wc.lane == 0) atomicOr(a.error_flag, 1);
                        continue;
                    }
                    if (L_n == prm.cap) {  // removePatch(worst), propagate.cpp:198-201 (the list is as long as when the trial began: np)
                        if (wc.lane == 0) {
                            if (worst >= MVS_NEWBASE) a.staging[worst - MVS_NEWBASE].flags &= ~1;
                            else a.kill[worst] = 1;
                        }
                        --L_n;
                        ++n_rep;
                    } else ++n_ins;
                    store_cand(a.staging + slot, wc, c, 1 | (v << 8), cell);
                    if (wc.lane == 0) a.job_stage[job * a.maxstage + ns] = (int32_t)slot;
                    ++ns;
                    // PatchManager::addPatch into this cell's own list if the patch lands here
                    const bool lands = ballot(wc.lane < c.nimg && c.img == v && c.gy * gw + c.gx == cell) != 0ull;
                    if (lands) {
                        const int nid = MVS_NEWBASE + (int)slot;
                        const int pos = __popcll(ballot(wc.lane < L_n && rank_before(L_ncc, L_id, c.ncc, nid)));
                        const int up_id = __shfl_up(L_id, 1);
                        const float up_ncc = __shfl_up(L_ncc, 1);
                        if (wc.lane > pos) { L_id = up_id; L_ncc = up_ncc; }
                        if (wc.lane == pos) { L_id = nid; L_ncc = c.ncc; }
                        ++L_n;
                    }
                    ST_ADD(6, st_t)
                }
                if (gave_up) break;
            }
            if (gave_up) break;
        }
        if (gave_up) break;
    }
    const SweepArgs& a = stage_args(kp).a;  // ---- stage: the cell's end
    if (!BIG && gave_up) {
        if (wc.lane == 0) { a.job_nstage[job] = 0; a.retry_jobs[atomicAdd(a.nretry, 1)] = (int32_t)job; }
        return;
    }
    if (wc.lane == 0) a.job_nstage[job] = ns;
    {  // wave-uniform sums: scalar registers, the caller's SweepAcc being a local
        acc->cand += n_cand; acc->pref += n_pref; acc->patch += n_patch; acc->f0 += n_f0; acc->f1 += n_f1; acc->ins += n_ins; acc->rep += n_rep;
        acc->evals += wc.evals; acc->view_evals += wc.view_evals;
        acc->pair[0] += n_pair; acc->pair[5] += n_elig;
        acc->pair[1] += n_last; acc->pair[2] += n_noroom; acc->pair[3] += n_lost; acc->pair[4] += n_long;
        acc->skip += n_skip;
#ifdef MVS_STAGE_TIMING
        st_acc[0] = ST_NOW() - st_begin;
        for (int k = 0; k < 12; ++k) acc->stage[k] += st_acc[k];
        acc->stage[12] = max(acc->stage[12], st_acc[12]); acc->stage[13] = max(acc->stage[13], st_acc[13]);
        acc->stage[14] += wc.st_acc[3]; acc->stage[15] += wc.st_acc[4];
#endif
    }
}

// The sweep's launch form: a grid of RESIDENT waves (as many 64-thread blocks as the device holds at MVS_SWEEP_WAVES per SIMD, or
// fewer) that pull work until none is left.  The launch's job range [job_lo, job_hi) is cut into chunks of MVS_XCD_CHUNK consecutive
// jobs (a stretch of one grid row); chunk c is in queue c % 8.  Blocks are dealt round-robin over the 8 XCDs (block b runs on XCD
// b % 8), and a wave serves queue blockIdx.x & 7 first: a stretch of cells goes to one XCD and consecutive stretches to consecutive
// XCDs, so a destination and its source cells share an L2 and every XCD gets the same mix of cheap and expensive regions.  (One
// contiguous band of cells per XCD left XCDs idle for a quarter of the launch: the bands -- one and a half views each -- differ in
// work; measured 770 -> 603 ms per iteration.)
// A queue is a LIST of the jobs of its chunks that will run a trial, in ascending job order (k_job_list / k_job_scatter, built while
// the index is hot; list_bounds[q] .. list_bounds[q + 1] of job_list): a wave never meets a ghost job, a cell without a source, or a
// cell whose source lists hold only patches of other reference views -- two jobs in three where the pool is dense -- and a launch
// in which no cell has a source reads eight empty bounds and exits.  A wave takes the next job of its queue with one atomicAdd WITH
// return on the queue's cursor (a cache line each, zero before the launch) -- in the middle of its work, like the staging-slot
// counter, never as its last instruction -- and when its queue is drained it takes from the others, in the order q + 1, q + 2, ...;
// when all eight are drained it adds its work counts into its counter slot and exits.  No grid barrier, no co-residency assumption:
// a block that starts late finds less work, a grid of one wave drains everything.
// A take is ONE job: the waves of an XCD must work on NEIGHBOURING cells at any one time, as the blocks of a one-block-per-cell
// launch do -- neighbours sample the same texels and read the same lists, and L1 / L2 serve them.  A wave that keeps a whole
// chunk to itself spreads the 384 waves of an XCD over 384 chunks: sweep 333 ms per step against 281 for one block per cell;
// takes of 64 / 16 / 4 / 1 jobs (of unlisted jobs, a lane per job testing for a source): 309 / 285 / 273.5 / 270.4 ms
// (profiles/r09_resident_ab.txt).  The cursor's atomic is one per listed job: a round trip in ~430 us of work per cell.
// WC: the wave context of the instantiation -- plain WaveCtx, or a WaveCtxT for a full window and / or the narrow samplers (mvs_sample.cuh)
template <bool SIMPLEX, class WC>
DEV void sweep_resident(const SweepKPtr kp, int* s_scratch, int* s_pend, float* s_texs) {
    WC wc;
    static_cast<WaveCtx&>(wc) = make_wave_ctx(stage_args(kp).prm);
    SweepAcc acc = sweep_acc_zero();
    for (unsigned step = 0; step < MVS_SWEEP_QUEUES; ++step) {
        const unsigned q = (blockIdx.x + step) & (MVS_SWEEP_QUEUES - 1u);
        int32_t qbegin;
        unsigned ntake;
        {
            const SweepArgs& a = stage_args(kp).a;
            qbegin = a.list_bounds[q];
            ntake = (unsigned)(a.list_bounds[q + 1] - qbegin);
        }
        if (ntake == 0u) continue;
        for (;;) {
            const SweepArgs& a = stage_args(kp).a;  // a take: the queue's cursor and the list
            unsigned k = 0;
            if (wc.lane == 0) k = atomicAdd(a.cursors + q * MVS_SWEEP_CURSOR_STRIDE, 1u);
            k = (unsigned)rfl((int)k);
            if (k >= ntake) break;  // drained: on to the next queue
            const int64_t job = a.job_list[qbegin + (int32_t)k];
            __syncthreads();  // the LDS scratch, frames, pivots and kept textures of the previous cell are dead
            sweep_cell<false, SIMPLEX>(kp, wc, &acc, job, s_scratch, s_pend, s_texs, nullptr);
        }
    }
    if (wc.lane == 0) sweep_acc_flush(stage_args(kp).a, acc, blockIdx.x & (MVS_COUNTER_SLOTS - 1));
}
// the second tier: block b runs the cells retry_jobs[b], retry_jobs[b + gridDim.x], ... with big_tables slot b
template <bool SIMPLEX>
DEV void sweep_retry_cell(const SweepKPtr kp, const int64_t job, int* s_scratch, int* s_pend, float* s_texs, int* big_table) {
    WaveCtx wc = make_wave_ctx(stage_args(kp).prm);
    SweepAcc acc = sweep_acc_zero();
    sweep_cell<true, SIMPLEX>(kp, wc, &acc, job, s_scratch, s_pend, s_texs, big_table);
    if (wc.lane == 0) sweep_acc_flush(stage_args(kp).a, acc, (unsigned)(job & (MVS_COUNTER_SLOTS - 1)));
}
// The kernels: the block's LDS, then sweep_resident or the retry loop on what varies (refiner, wave context); mvsk_sweep's table chooses
// among the first four.  (The LDS is declared, and the retry loop written, in the kernel itself: with either in a shared device function
// the kernels compile to other code -- profiles/r24_codeobj_kernel_split.txt.)
#define SWEEP_LDS                                                                                                                  \
    __shared__ int s_scratch[192];                                                                                                 \
    __shared__ __attribute__((aligned(16))) int s_pend[MVS_PEND_INTS]; /* a waiting candidate, the working block of a pair (mvs_refine.cuh) */ \
    extern __shared__ float s_texs[];
// (The argument is never named: the kernels read it in place, through sweep_kargs().)
__global__ __launch_bounds__(64, MVS_SWEEP_WAVES) void k_sweep(SweepKArgs) { SWEEP_LDS sweep_resident<false, WaveCtx>(sweep_kargs(), s_scratch, s_pend, s_texs); }
// for a launch whose window fills every slot of every lane (cls_full_window: the default 7x7)
__global__ __launch_bounds__(64, MVS_SWEEP_WAVES) void k_sweep_full(SweepKArgs) { SWEEP_LDS sweep_resident<false, WaveCtxT<true, false>>(sweep_kargs(), s_scratch, s_pend, s_texs); }
// ... with the narrow samplers (32-bit texel offsets from DParams::pyr32) where the pyramid block is below 4 GiB; k_sweep_full itself,
// with a 64-bit address per lane, serves the larger ones
__global__ __launch_bounds__(64, MVS_SWEEP_WAVES) void k_sweep_full_ofs(SweepKArgs) { SWEEP_LDS sweep_resident<false, WaveCtxT<true, true>>(sweep_kargs(), s_scratch, s_pend, s_texs); }
__global__ __launch_bounds__(64, MVS_SWEEP_WAVES) void k_sweep_simplex(SweepKArgs) { SWEEP_LDS sweep_resident<true, WaveCtx>(sweep_kargs(), s_scratch, s_pend, s_texs); }
__global__ __launch_bounds__(64, 1) void k_sweep_retry(SweepKArgs) {
    SWEEP_LDS
    const SweepKPtr kp = sweep_kargs();
    int* big_table = stage_args(kp).a.big_tables + (size_t)blockIdx.x * MVS_FILTER2_HASH_CAP;
    for (int k = blockIdx.x; k < stage_args(kp).nretry; k += gridDim.x) {
        __syncthreads();
        sweep_retry_cell<false>(kp, (int64_t)stage_args(kp).a.retry_jobs[k], s_scratch, s_pend, s_texs, big_table);
    }
}
__global__ __launch_bounds__(64, 1) void k_sweep_retry_simplex(SweepKArgs) {
    SWEEP_LDS
    const SweepKPtr kp = sweep_kargs();
    int* big_table = stage_args(kp).a.big_tables + (size_t)blockIdx.x * MVS_FILTER2_HASH_CAP;
    for (int k = blockIdx.x; k < stage_args(kp).nretry; k += gridDim.x) {
        __syncthreads();
        sweep_retry_cell<true>(kp, (int64_t)stage_args(kp).a.retry_jobs[k], s_scratch, s_pend, s_texs, big_table);
    }
}

// =================================================================== commit
// alive staged records per job -> cnt[job]
__global__ void k_commit_count(SweepArgs a, int32_t* __restrict__ cnt) {
    const int64_t job = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (job >= a.njobs) return;
    const int ns = a.job_nstage[job];
    int c = 0;
    for (int k = 0; k < ns; ++k) c += a.staging[a.job_stage[job * a.maxstage + k]].flags & 1;
    cnt[job] = c;
}
// copy alive staged records to dst[base[job] + r] in creation order: global order (view, cell, sequence)
__global__ void k_commit_copy(SweepArgs a, const int32_t* __restrict__ base, DPatch* __restrict__ dst, int64_t dst_cap, int32_t* __restrict__ per_view,
                              int keep_key) {
    const int64_t job = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (job >= a.njobs) return;
    const int ns = a.job_nstage[job];
    int r = 0;
    for (int k = 0; k < ns; ++k) {
        const DPatch* sp = a.staging + a.job_stage[job * a.maxstage + k];
        if (!(sp->flags & 1)) continue;
        const int64_t o = (int64_t)base[job] + r++;
        if (o >= dst_cap) { atomicOr(a.error_flag, 2); return; }
        const uint4* s4 = reinterpret_cast<const uint4*>(sp);
        uint4* d4 = reinterpret_cast<uint4*>(dst + o);
        for (int w = 0; w < (int)MVS_REC_U4; ++w) d4[w] = s4[w];
        if (per_view) atomicAdd(&per_view[(sp->flags >> 8) & 0xff], 1);
        if (!keep_key) { dst[o].flags = 1; dst[o].id = 0; }
    }
}

// =================================================================== host-callable launchers
size_t mvsk_sweep_lds_bytes(const DParams& prm) {
    const size_t texs = texs_gram_lds_bytes(prm);                                         // setRefImage's textures behind the frames
    const size_t chk = (size_t)MVS_CHECK_LDS_FLOATS * sizeof(float);                      // Optim::check hash set + rows
    const size_t need = texs > chk ? texs : chk;
    return need > (size_t)MVS_FRAME_LDS_BYTES ? need : (size_t)MVS_FRAME_LDS_BYTES;  // the frames + pivots of a refinement step
}
// What a sweep or refine-probe launch on these parameters may use.  The three A/B and test switches are read here, on every launch, and
// the result depends on none of them:
//   MVS_SWEEP_FULLWINDOW=0  keeps a full window (cls_full_window: the default 7x7) on the generic kernel
//   MVS_SAMPLER_WIDE=1      keeps the 64-bit per-lane addresses that a pyramid block of 4 GiB or more needs (DParams::pyr32 is null there)
//   MVS_SWEEP_PAIR=0        makes every trial refine alone
KernelVariant mvsk_kernel_variant(const DParams& prm) {
    const auto env_int = [](const char* name, int unset) { const char* p = getenv(name); return p ? atoi(p) : unset; };
    KernelVariant v;
    v.launched = false;
    v.full_window = cls_full_window(prm.wsz) && env_int("MVS_SWEEP_FULLWINDOW", 1) != 0;
    v.narrow = prm.pyr32 && env_int("MVS_SAMPLER_WIDE", 0) == 0;
    v.pair = env_int("MVS_SWEEP_PAIR", 1) != 0;
    return v;
}
// The sweep's kernels, the most particular first: a launch goes to the first row of its refiner that asks for nothing the launch lacks
// (mvsk_kernel_variant), and what mvsk_sweep reports is that row.  A new instantiation is a wrapper above and a row here.
// A launch's argument block is built here, per launch, and passed by value: the runtime copies it into the launch's own kernel-argument
// segment, so two launches in flight -- of one engine or of two -- never share a parameter.
static SweepKArgs sweep_kargs_of(const DParams& prm, const SweepArgs& a, int nretry, const RefineSel& rs) {
    SweepKArgs k;
    k.prm = prm; k.a = a; k.nretry = nretry; k.max_evals = rs.max_evals; k.xtol = rs.xtol;
    return k;
}
typedef void (*SweepLaunch)(unsigned nblocks, size_t lds, hipStream_t st, const DParams& prm, const SweepArgs& a, const RefineSel& rs);
#define SWEEP_ROW(simplex, full_window, narrow, ...) \
    {simplex, full_window, narrow, [](unsigned nblocks, size_t lds, hipStream_t st, const DParams& prm, const SweepArgs& a, const RefineSel& rs) { \
         hipLaunchKernelGGL(__VA_ARGS__); }}
static const struct { bool simplex, full_window, narrow; SweepLaunch launch; } sweep_table[] = {
    SWEEP_ROW(true, false, false, k_sweep_simplex, dim3(nblocks), dim3(64), lds, st, sweep_kargs_of(prm, a, 0, rs)),
    SWEEP_ROW(false, true, true, k_sweep_full_ofs, dim3(nblocks), dim3(64), lds, st, sweep_kargs_of(prm, a, 0, rs)),
    SWEEP_ROW(false, true, false, k_sweep_full, dim3(nblocks), dim3(64), lds, st, sweep_kargs_of(prm, a, 0, rs)),
    SWEEP_ROW(false, false, false, k_sweep, dim3(nblocks), dim3(64), lds, st, sweep_kargs_of(prm, a, 0, rs)),
};
KernelVariant mvsk_sweep(const DParams& prm, const SweepArgs& a, const RefineSel& rs, hipStream_t st) {
    KernelVariant v = mvsk_kernel_variant(prm);
    const int64_t nloc = a.job_hi - a.job_lo;
    if (nloc <= 0) return v;
    // development knob: MVS_SWEEP_LDS_PAD=<bytes> raises the block's LDS allocation, i.e. lowers the waves per SIMD
    static const size_t pad = getenv("MVS_SWEEP_LDS_PAD") ? (size_t)atol(getenv("MVS_SWEEP_LDS_PAD")) : 0;
    const size_t lds = mvsk_sweep_lds_bytes(prm) + pad;
    // the resident grid: the waves the device holds at the launch bound (4 SIMDs per CU) and no more blocks than there are jobs.  (Where the LDS allocation lets fewer waves in, the rest start late and find less work: nothing depends on residency.)
    int dev = 0, cus = 0;
    (void)hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) { (void)hipGetLastError(); cus = 256; }
    int64_t nblocks = (int64_t)cus * 4 * MVS_SWEEP_WAVES;
    nblocks = std::min(nblocks, nloc);  // (how many of them are listed only the device knows)
    // development knob, read on every launch: MVS_SWEEP_GRID=<n> caps the number of resident blocks (the result does not depend on it)
    if (const char* g = getenv("MVS_SWEEP_GRID")) {
        const long cap = atol(g);
        if (cap > 0) nblocks = std::min<int64_t>(nblocks, cap);
    }
    SweepArgs b = a;
    b.pair = v.pair ? 1 : 0;
    for (const auto& row : sweep_table) {
        if (row.simplex != (rs.simplex != 0) || (row.full_window && !v.full_window) || (row.narrow && !v.narrow)) continue;
        row.launch((unsigned)nblocks, lds, st, prm, b, rs);
        v.launched = true; v.full_window = row.full_window; v.narrow = row.narrow;
        break;
    }
    return v;
}
void mvsk_job_work(const DParams& prm, const SweepArgs& a, int mode, int shift, int32_t* work, hipStream_t st) {
    if (a.njobs > 0) hipLaunchKernelGGL(k_job_work, dim3(nblk(a.njobs, 256)), dim3(256), 0, st, prm, a, mode, shift, work);
}
int mvsk_job_list_seg(const SweepArgs& a) {
    const int64_t nchunks = (std::max<int64_t>(a.job_hi - a.job_lo, 0) + MVS_XCD_CHUNK - 1) / MVS_XCD_CHUNK;
    return (int)((nchunks + MVS_SWEEP_QUEUES - 1) / MVS_SWEEP_QUEUES) * MVS_XCD_CHUNK;
}
void mvsk_job_list(const DParams& prm, const SweepArgs& a, int32_t* flags, int32_t* scan, int32_t* scan_tmp, int32_t* list, int32_t* bounds, hipStream_t st) {
    const int seg = mvsk_job_list_seg(a);
    const int64_t nslots = (int64_t)MVS_SWEEP_QUEUES * seg, nthreads = std::max(nslots, a.njobs);
    if (nthreads <= 0) return;
    hipLaunchKernelGGL(k_job_list, dim3(nblk(nthreads, 256)), dim3(256), 0, st, prm, a, seg, flags);
    if (nslots <= 0) return;
    mvsk_exclusive_scan(flags, scan, nslots, scan_tmp, st);
    hipLaunchKernelGGL(k_job_scatter, dim3(nblk(nslots, 256)), dim3(256), 0, st, a, seg, scan, list, bounds);
}
void mvsk_job_cuts(const int32_t* scan, int64_t njobs, int n, int32_t* cuts, hipStream_t st) {
    if (njobs > 0) hipLaunchKernelGGL(k_job_cuts, dim3(nblk(njobs, 256)), dim3(256), 0, st, scan, njobs, n, cuts);
}
void mvsk_sweep_retry(const DParams& prm, const SweepArgs& a, int nretry, const RefineSel& rs, hipStream_t st) {
    if (nretry <= 0) return;
    const dim3 grid((unsigned)std::min(nretry, MVS_BIG_SLOTS));
    SweepArgs b = a;
    b.pair = mvsk_kernel_variant(prm).pair ? 1 : 0;
    if (rs.simplex) hipLaunchKernelGGL(k_sweep_retry_simplex, grid, dim3(64), mvsk_sweep_lds_bytes(prm), st, sweep_kargs_of(prm, b, nretry, rs));
    else hipLaunchKernelGGL(k_sweep_retry, grid, dim3(64), mvsk_sweep_lds_bytes(prm), st, sweep_kargs_of(prm, b, nretry, rs));
}
void mvsk_commit_count(const SweepArgs& a, int32_t* cnt, hipStream_t st) { hipLaunchKernelGGL(k_commit_count, dim3(nblk(a.njobs, 256)), dim3(256), 0, st, a, cnt); }
void mvsk_commit_copy(const SweepArgs& a, const int32_t* base, DPatch* dst, int64_t dst_cap, int32_t* per_view, int keep_key, hipStream_t st) {
    hipLaunchKernelGGL(k_commit_copy, dim3(nblk(a.njobs, 256)), dim3(256), 0, st, a, base, dst, dst_cap, per_view, keep_key);
}
