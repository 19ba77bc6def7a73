// mvs_engine_pass.cpp -- the hot path of the C ABI in include/mvskit_engine.h: the cell indexes and the pool's counts, the per-pass
// schedule (index build -> sweep -> commit) on one HIP stream with its HIP-event timing, the commit paths and Propagate::run.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "mvs_engine_impl.h"

using namespace mvseng;

namespace mvseng {

int build_list(mvs_engine* e, bool vgrid, bool trim, bool unordered) {
    hipStream_t st = e->stream;
    const int64_t nc = e->total_cells;
    DParams p = current_params(e);
    DevBuf<int32_t>& cnt = vgrid ? e->vcnt : e->cnt;
    DevBuf<csr_off_t>& start = vgrid ? e->vstart : e->start;
    DevBuf<int32_t>& cursor = vgrid ? e->vcursor : e->cursor;
    DevBuf<unsigned long long>& ids = e->ids;
    DevBuf<int32_t>& id32 = vgrid ? e->vid32 : e->id32;
    DevBuf<int32_t>& cnt_alive = vgrid ? e->vcnt_alive : e->cnt_alive;
    HIPCHK(hipMemsetAsync(cnt.p, 0, (size_t)(nc + 1) * sizeof(int32_t), st));
    mvsk_index_count(p, vgrid ? nullptr : cnt.p, vgrid ? cnt.p : nullptr, nullptr, st);
    const bool direct = unordered && !trim;
    DevBuf<csr_off_t>& raw = e->start_raw;  // the offsets before the trim (ordered lists): the scan writes them where the sort wants them
    csr_off_t* const first_scan = direct ? start.p : raw.p;
    mvsk_exclusive_scan_off(cnt.p, first_scan, nc, reinterpret_cast<csr_off_t*>(e->scan_tmp.p), st);
    csr_off_t tot64 = 0;  // the number of memberships = the scan's last element (a per-wave atomicAdd to one counter cost the count a third of its time)
    if (int r = read_back(e, first_scan + nc, &tot64)) return r;
    const int64_t tot = (int64_t)tot64;
    if (!unordered) { if (int r = ids.ensure(tot + 16)) return r; }
    if (!vgrid && !unordered) { if (int r = e->key.ensure(tot + 16)) return r; }
    if (int r = id32.ensure(tot + 16)) return r;
    p = current_params(e);
    HIPCHK(hipMemsetAsync(cursor.p, 0, (size_t)(nc + 1) * sizeof(int32_t), st));
    if (direct) {
        mvsk_index_fill_direct(p, vgrid ? 1 : 0, start.p, cursor.p, id32.p, st);
        cnt.swap(cnt_alive);  // every entry is alive: the counts ARE the alive counts (two buffers of one size; the next build clears its own)
        e->lists_dense[vgrid ? 1 : 0] = true;
        return MVS_OK;
    }
    // sorted lists [and the trim]: keys -> per-cell sort -> [trim] -> each list's alive entries to the front of its range -> the lists
    // packed end to end (a second scan, over the alive counts), so that every index the engine builds is dense
    if (int r = e->id32_raw.ensure(tot + 16)) return r;
    mvsk_index_fill(p, vgrid ? 1 : 0, raw.p, cursor.p, ids.p, st);
    mvsk_index_sort_trim(p, raw.p, ids.p, trim ? 1 : 0, e->misc.p + misc::trim_parts, st);
    mvsk_index_finalize(p, vgrid ? 1 : 0, raw.p, ids.p, e->id32_raw.p, cnt_alive.p, st);
    mvsk_exclusive_scan_off(cnt_alive.p, start.p, nc, reinterpret_cast<csr_off_t*>(e->scan_tmp.p), st);
    mvsk_index_pack(p, raw.p, start.p, cnt_alive.p, ids.p, e->id32_raw.p, vgrid ? nullptr : e->key.p, id32.p, st);
    e->lists_dense[vgrid ? 1 : 0] = true;
    return MVS_OK;
}
int build_depth(mvs_engine* e) {
    const DParams p = current_params(e);
    HIPCHK(hipMemsetAsync(e->dpgrid.p, 0xff, (size_t)e->total_cells * sizeof(unsigned long long), e->stream));
    mvsk_depth_maps(p, e->dpgrid.p, nullptr, e->stream);
    return MVS_OK;
}
int build_index(mvs_engine* e, unsigned long long* trimmed_out) {
    hipStream_t st = e->stream;
    const DParams p = current_params(e);
    HIPCHK(hipMemsetAsync(e->misc.p + misc::fill_evals, 0, 2 * sizeof(unsigned long long), st));
    HIPCHK(hipMemsetAsync(e->misc.p + misc::trim_parts, 0, misc::trim_nparts * sizeof(unsigned long long), st));
    // PatchManager::sortPatches re-scores every patch whose m_ncc < 0 each time it meets it
    // (patch_manager.cpp:411-415); a wave that finds m_ncc >= 0 exits at once.
    mvsk_fill_ncc(p, e->misc.p + misc::fill_evals, st);
    e->ncc_dirty = false;
    if (int r = build_list(e, false, true)) return r;
    // m_vpgrids: no reader depends on the order inside its lists (findNeighbors' set, filterSmallGroups' unions): written without keys and sort
    if (want_vgrid(e)) if (int r = build_list(e, true, false, true)) return r;
    if (int r = build_depth(e)) return r;
    if (trimmed_out) {
        unsigned long long part[misc::trim_nparts];
        HIPCHK(hipMemcpyAsync(part, e->misc.p + misc::trim_parts, sizeof part, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        *trimmed_out = 0;
        for (unsigned long long v : part) *trimmed_out += v;
    }
    HIPCHK(hipGetLastError());
    return MVS_OK;
}

int count_pool(mvs_engine* e, Count what, int64_t* total) {
    hipStream_t st = e->stream;
    *total = 0;
    if (e->pool_n == 0) return MVS_OK;
    if (what == Count::alive) mvsk_alive_count(e->pool.p, e->pool_n, e->kill_cnt.p, st);
    else mvsk_kill_count(e->kill.p, e->pool_n, e->kill_cnt.p, st);
    mvsk_exclusive_scan(e->kill_cnt.p, e->kill_base.p, e->pool_n, reinterpret_cast<int32_t*>(e->scan_tmp.p), st);
    int32_t n = 0;
    HIPCHK(hipMemcpyAsync(&n, e->kill_base.p + e->pool_n, sizeof n, hipMemcpyDeviceToHost, st));
    if (what == Count::apply_kills) mvsk_apply_kill_flags(e->pool.p, e->kill.p, e->pool_n, st);
    HIPCHK(hipStreamSynchronize(st));
    *total = n;
    return MVS_OK;
}

int ensure_counts(mvs_engine* e) {
    if (e->counted) return MVS_OK;
    hipStream_t st = e->stream;
    const int64_t nj = e->sa.njobs;
    e->n_new = 0; e->n_kill = 0;
    e->h_per_view.assign(e->cfg.nviews, 0);
    if (nj > 0) {
        mvsk_commit_count(e->sa, e->job_cnt.p, st);
        mvsk_exclusive_scan(e->job_cnt.p, e->job_base_scan.p, nj, reinterpret_cast<int32_t*>(e->scan_tmp.p), st);
        std::vector<int32_t> bounds(e->sa.nsweep_views + 1);
        for (int s = 0; s < e->sa.nsweep_views; ++s)
            HIPCHK(hipMemcpyAsync(&bounds[s], e->job_base_scan.p + e->sa.job_base[s], sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(&bounds[e->sa.nsweep_views], e->job_base_scan.p + nj, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        e->n_new = bounds[e->sa.nsweep_views];
        for (int s = 0; s < e->sa.nsweep_views; ++s) e->h_per_view[e->sa.sweep_views[s]] = bounds[s + 1] - bounds[s];
    }
    if (int r = count_pool(e, Count::kills, &e->n_kill)) return r;
    e->counted = true;
    return MVS_OK;
}

int compact_pool(mvs_engine* e) {
    int64_t alive = 0;
    if (int r = count_pool(e, Count::alive, &alive)) return r;
    if (alive == e->pool_n) return MVS_OK;
    mvsk_alive_gather(e->pool.p, e->pool_n, e->kill_base.p, e->pool_alt.p, e->pool_alt.cap, e->stream);
    e->pool.swap(e->pool_alt);
    e->pool_n = alive;
    return MVS_OK;
}

void discard_pass(mvs_engine* e) {
    if (e->kill.p && e->pool_n > 0) (void)hipMemsetAsync(e->kill.p, 0, (size_t)e->pool_n, e->stream);
    (void)hipStreamSynchronize(e->stream);
    e->staged = false; e->counted = false;
}

}  // namespace mvseng

namespace {

// a += b over the ten counters (b: another mvs_counters, or one of the sweep's DCounters partial sums)
template <typename C> void add_counters(mvs_counters& a, const C& b) {
    a.candidates += b.candidates; a.prefiltered += b.prefiltered; a.patches += b.patches; a.fail0 += b.fail0; a.fail1 += b.fail1;
    a.inserted += b.inserted; a.replaced += b.replaced; a.evals += b.evals; a.view_evals += b.view_evals; a.trimmed += b.trimmed;
}

}  // namespace

extern "C" {

// A pass that failed (staging or Optim::check capacity in this rank's shard, a HIP error) leaves its status in the engine:
// with a communicator attached the next mvs_engine_exchange hands it to every rank, so that all of them give the pass up
// together instead of waiting in a collective for a rank that has already returned.
static int pass_impl(mvs_engine* e, int iter, int pass, mvs_counters* out);
int mvs_engine_pass(mvs_engine* e, int iter, int pass, mvs_counters* out) {
    const int r = pass_impl(e, iter, pass, out);
    if (e) { e->pass_status = r; e->pass_error = r ? g_err : std::string(); }
    return r;
}
static int pass_impl(mvs_engine* e, int iter, int pass, mvs_counters* out) {
    if (!e || !e->have_views) { g_err = "mvs_engine_pass: views not set"; return MVS_ERR_STATE; }
    if (e->staged) { g_err = "mvs_engine_pass: the previous pass was not committed"; return MVS_ERR_STATE; }
    HIPCHK(hipSetDevice(e->cfg.device));
    hipStream_t st = e->stream;
    HIPCHK(hipEventRecord(e->ev[0], st));
    unsigned long long trimmed = 0;
    {
        Range rg("mvs:index");
        if (int r = build_index(e, &trimmed)) return r;
    }
    // jobs: one per (swept view, row, half column) of the pass colour
    SweepArgs& a = e->sa;
    memset(&a, 0, sizeof a);
    a.iter = iter; a.inc = (iter % 2 == 0) ? 1 : -1; a.colour = pass & 1;
    int64_t nj = 0;
    const bool ranged = e->cfg.shard_count > 1;  // shard by job range over all views, else by whole views
    for (int v = ranged ? 0 : e->cfg.view_begin; v < e->cfg.nviews; v += ranged ? 1 : e->cfg.view_stride) {
        a.sweep_views[a.nsweep_views] = v;
        a.job_base[a.nsweep_views] = (int32_t)nj;
        ++a.nsweep_views;
        nj += (int64_t)((e->hviews[v].gw + 1) / 2) * e->hviews[v].gh;
    }
    a.njobs = nj;
    a.job_lo = 0; a.job_hi = nj;
    if (ranged) {
        // Contiguous ranges of equal WORK, not of equal job count: every rank holds the same index, so every rank computes the
        // same per-job work proxy (k_job_work), the same prefix sums and the same cuts; rank order stays commit order.  Equal
        // counts gave each of 8 ranks a band of one and a half views, and such bands differ in work by tens of per cent.
        // MVS_SPLIT_PROXY=0|1|2 (development): 0 = equal job counts, 1 = source entries, 2 = expected trials by kind (default).
        const int split_mode = getenv("MVS_SPLIT_PROXY") ? atoi(getenv("MVS_SPLIT_PROXY")) : 2;
        const int N = e->cfg.shard_count, R = e->cfg.shard_index;
        std::vector<int32_t> cuts(N + 1, -1);
        int64_t total_work = 0;
        if (split_mode > 0 && nj > 0) {
            const DParams p0 = current_params(e);
            int shift = 0;  // the scan is 32-bit: scale the proxy down if its worst case would not fit
            // (every job's work is rounded UP after the shift, so the 32-bit prefix sum may exceed the shifted bound by up to nj)
            while ((((int64_t)3 * e->prm.cap * e->prm.max_propag * 32 * nj) >> shift) + nj >= (int64_t)INT32_MAX) ++shift;
            mvsk_job_work(p0, a, split_mode, shift, e->job_cnt.p, st);
            mvsk_exclusive_scan(e->job_cnt.p, e->job_base_scan.p, nj, reinterpret_cast<int32_t*>(e->scan_tmp.p), st);
            if (int r = e->tmp_i.ensure(N + 1)) return r;
            HIPCHK(hipMemsetAsync(e->tmp_i.p, 0xff, (size_t)(N + 1) * sizeof(int32_t), st));
            mvsk_job_cuts(e->job_base_scan.p, nj, N, e->tmp_i.p, st);
            int32_t tw = 0;
            HIPCHK(hipMemcpyAsync(cuts.data(), e->tmp_i.p, (size_t)(N + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(&tw, e->job_base_scan.p + nj, sizeof tw, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            total_work = tw;
        }
        cuts[0] = 0; cuts[N] = (int32_t)nj;
        for (int r = 1; r < N; ++r) {
            if (total_work <= 0 || cuts[r] < 0) cuts[r] = (int32_t)(nj * r / N);  // no work anywhere: equal counts
            cuts[r] = std::max(cuts[r], cuts[r - 1]);
        }
        a.job_lo = cuts[R];
        a.job_hi = cuts[R + 1];
    }
    a.staging = e->staging.p; a.staging_cap = e->staging.cap;
    a.stage_counter = e->misc.p + misc::stage_counter;
    a.job_stage = e->job_stage.p; a.job_nstage = e->job_nstage.p;
    a.maxstage = (e->prm.view_propagation ? 3 : 2) * e->prm.cap * e->prm.max_propag;
    a.kill = e->kill.p;
    a.counters = e->counters.p;
    a.error_flag = e->error_flag.p;
    if (want_vgrid(e)) {  // Optim::check runs in this pass: its second tier needs its global-memory tables and the list of cells
        if (int r = e->big_tables.ensure((int64_t)256 * 16384)) return r;
        if (int r = e->retry_jobs.ensure(std::max<int64_t>(nj, 16))) return r;
    }
    a.big_tables = e->big_tables.p; a.retry_jobs = e->retry_jobs.p; a.nretry = reinterpret_cast<int32_t*>(e->misc.p + misc::sweep_retry);
    HIPCHK(hipMemsetAsync(e->misc.p + misc::sweep_retry, 0, sizeof(unsigned long long), st));
    HIPCHK(hipMemsetAsync(e->misc.p + misc::stage_counter, 0, sizeof(unsigned long long), st));
    a.cursors = reinterpret_cast<uint32_t*>(e->misc.p + misc::sweep_cursors);
    HIPCHK(hipMemsetAsync(e->misc.p + misc::sweep_cursors, 0, (misc::sweep_cursor_words + misc::sweep_list_bound_words) * sizeof(unsigned long long), st));
    HIPCHK(hipMemsetAsync(e->counters.p, 0, MVS_COUNTER_SLOTS * sizeof(DCounters), st));
    HIPCHK(hipMemsetAsync(e->error_flag.p, 0, sizeof(int32_t), st));
    const DParams p = current_params(e);
    const RefineSel rs = refine_sel(e);
    // The jobs of this launch that will run a trial, per queue, while the index is hot (part of index_ms); every job's job_nstage is
    // cleared on the way.  The waves read the list bounds on the device: the host learns them with the counters, after the sweep.
    if (int r = e->job_list.ensure(std::max<int64_t>(nj, 16))) return r;
    if (e->job_cnt.ensure(nj + misc::job_list_pad) || e->job_base_scan.ensure(nj + misc::job_list_pad)) return MVS_ERR_HIP;
    int32_t* list_bounds = reinterpret_cast<int32_t*>(e->misc.p + misc::sweep_list_bounds);
    a.job_list = e->job_list.p; a.list_bounds = list_bounds;
    mvsk_job_list(p, a, e->job_cnt.p, e->job_base_scan.p, reinterpret_cast<int32_t*>(e->scan_tmp.p), e->job_list.p, list_bounds, st);
    HIPCHK(hipEventRecord(e->ev[1], st));
    Range rg_sweep(pass & 1 ? "mvs:sweep colour 1" : "mvs:sweep colour 0");
    const KernelVariant sweep_kernel = mvsk_sweep(p, a, rs, st);
    if (sweep_kernel.launched) { e->sweep_kernels[sweep_kernel.full_window ? 1 : 0] += 1; e->sampler_launches[sweep_kernel.narrow ? 1 : 0] += 1; }
    e->pass_retried = 0;
    if (want_vgrid(e)) {  // cells whose Optim::check outgrew the wave's LDS run again on the second tier (normally none)
        int32_t nretry = 0;
        if (int r = read_back(e, a.nretry, &nretry)) return r;
        e->pass_retried = nretry;
        if (nretry > 0) { mvsk_sweep_retry(p, a, nretry, rs, st); e->retried_cells += nretry; }
    }
    HIPCHK(hipEventRecord(e->ev[2], st));
    std::vector<DCounters> hcs(MVS_COUNTER_SLOTS);
    int32_t herr = 0;
    unsigned long long fill[2] = {0, 0};  // evaluations spent on seeds whose m_ncc was < 0 (sortPatches)
    HIPCHK(hipMemcpyAsync(fill, e->misc.p + misc::fill_evals, sizeof fill, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(hcs.data(), e->counters.p, hcs.size() * sizeof(DCounters), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&herr, e->error_flag.p, sizeof herr, hipMemcpyDeviceToHost, st));
    int32_t hbounds[MVS_SWEEP_QUEUES + 1];
    HIPCHK(hipMemcpyAsync(hbounds, list_bounds, sizeof hbounds, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    mvs_counters sum{};
    for (const DCounters& c : hcs) {
        add_counters(sum, c);
        for (int k = 0; k < 6; ++k) e->sweep_pairs[k] += (int64_t)c.pair[k];
        for (int k = 0; k < 2; ++k) e->sweep_repeats[k] += (int64_t)c.repeats[k];
    }
    sum.evals += fill[0]; sum.view_evals += fill[1]; sum.trimmed = (int64_t)trimmed;
    float ms = 0.0f;
    (void)hipEventElapsedTime(&ms, e->ev[0], e->ev[1]); e->timing.index_ms = ms;
    (void)hipEventElapsedTime(&ms, e->ev[1], e->ev[2]); e->timing.sweep_ms = ms;
    e->timing.commit_ms = 0.0f; e->timing.sweep_launches = 1; e->timing.exchange_ms = 0.0f; e->timing.exchange_bytes = 0;
    e->timing.check_retried_cells = e->pass_retried;
    e->timing.sweep_jobs_listed = hbounds[MVS_SWEEP_QUEUES];
    e->staged = true; e->counted = false;
    if (out) *out = sum;
#ifdef MVS_JOBLIST_COUNTS  // diagnostic build (k_job_list): what the former per-take test would have let through, beside what is listed
    fprintf(stderr, "[job list] iter %d colour %d: jobs %lld, with any source entry %llu, listed %llu\n", iter, pass & 1, (long long)(a.job_hi - a.job_lo),
            hcs[0].stage[0], hcs[0].stage[1]);
#endif
#ifdef MVS_STAGE_TIMING
    {
        unsigned long long stage[16] = {0};
        for (const DCounters& c : hcs)
            for (int k = 0; k < 16; ++k) stage[k] = (k == 12 || k == 13) ? std::max(stage[k], c.stage[k]) : stage[k] + c.stage[k];
        static const char* nm[8] = {"wave", "generate", "pre", "refine", "post", "check", "stage", "prologue"};
        fprintf(stderr, "[stage cycles]");
        for (int k = 0; k < 8; ++k) fprintf(stderr, " %s %.1f%%", nm[k], 100.0 * (double)stage[k] / (double)(stage[0] ? stage[0] : 1));
        static const char* nm2[4] = {"gain", "search", "sort", "quad"};
        for (int k = 0; k < 4; ++k) fprintf(stderr, " %s %.1f%%", nm2[k], 100.0 * (double)stage[8 + k] / (double)(stage[0] ? stage[0] : 1));
        fprintf(stderr, " setRefImage pairs %.1f%% choice %.1f%%", 100.0 * (double)stage[14] / (double)(stage[0] ? stage[0] : 1), 100.0 * (double)stage[15] / (double)(stage[0] ? stage[0] : 1));
        fprintf(stderr, "  (wave cycles %.3e; max visited %llu, max neighbours %llu)\n", (double)stage[0], stage[12], stage[13]);
    }
#endif
    // Fault injection: MVS_FAULT_PASS=<shard>:<iter>:<pass> makes that one pass of that shard report a
    // capacity failure after its sweep, once -- how the tests drive a rank-local failure through the collective status word.
#ifdef MVS_FAULT_INJECTION  // test builds only (libmvskit_engine_faultinj.so, mvskit_amd/build.py): the product library never reads the variable
    if (const char* f = getenv("MVS_FAULT_PASS")) {
        int fr = -1, fi = -1, fp = -1;
        if (!e->fault_fired && sscanf(f, "%d:%d:%d", &fr, &fi, &fp) == 3 && fr == (e->cfg.shard_count > 1 ? e->cfg.shard_index : 0) && fi == iter && fp == pass) {
            e->fault_fired = true;
            g_err = "mvs_engine_pass: capacity failure injected by MVS_FAULT_PASS";
            return MVS_ERR_CAPACITY;
        }
    }
#endif
    if (herr & 3) { g_err = "mvs_engine_pass: staging capacity exceeded (raise mvs_config.max_patches)"; return MVS_ERR_CAPACITY; }
    if (herr & 4) {
        g_err = "mvs_engine_pass: Optim::check met more than 14336 patches around one patch, or more than 4064 neighbours (engine limit)";
        return MVS_ERR_CAPACITY;
    }
    return MVS_OK;
}

int mvs_engine_export_counts(mvs_engine* e, int64_t* n_new, int64_t* n_kill, int32_t* per_view_new) {
    if (!e || !e->staged) { g_err = "mvs_engine_export_counts: no pass to export"; return MVS_ERR_STATE; }
    HIPCHK(hipSetDevice(e->cfg.device));
    if (int r = ensure_counts(e)) return r;
    if (n_new) *n_new = e->n_new;
    if (n_kill) *n_kill = e->n_kill;
    if (per_view_new) for (int v = 0; v < e->cfg.nviews; ++v) per_view_new[v] = e->h_per_view[v];
    return MVS_OK;
}

int mvs_engine_export_device(mvs_engine* e, void* d_new, int64_t cap_new, void* d_kill, int64_t cap_kill) {
    if (!e || !e->staged) { g_err = "mvs_engine_export_device: no pass to export"; return MVS_ERR_STATE; }
    HIPCHK(hipSetDevice(e->cfg.device));
    if (int r = ensure_counts(e)) return r;
    if (e->n_new > cap_new || e->n_kill > cap_kill) { g_err = "mvs_engine_export_device: buffers too small"; return MVS_ERR_CAPACITY; }
    if (e->n_new > 0) mvsk_commit_copy(e->sa, e->job_base_scan.p, (DPatch*)d_new, cap_new, nullptr, 1, e->stream);
    if (e->n_kill > 0) mvsk_kill_export(e->kill.p, e->pool_n, e->kill_base.p, (int32_t*)d_kill, cap_kill, e->stream);
    HIPCHK(hipStreamSynchronize(e->stream));
    return MVS_OK;
}

int mvs_engine_commit_device(mvs_engine* e, const void* d_new, int64_t n_new, const void* d_kill, int64_t n_kill) {
    if (!e || !e->have_views) return MVS_ERR_STATE;
    HIPCHK(hipSetDevice(e->cfg.device));
    hipStream_t st = e->stream;
    if (e->pool_n + n_new > e->pool.cap) { g_err = "mvs_engine_commit_device: patch pool capacity exceeded (raise mvs_config.max_patches)"; return MVS_ERR_CAPACITY; }
    return commit_pool(e, [&](int64_t* added) -> int {  // the caller's kill ids and records
        mvsk_apply_kill_ids(e->pool.p, (const int32_t*)d_kill, n_kill, e->pool_n, st);
        mvsk_append_records(e->pool.p, e->pool_n, (const DPatch*)d_new, n_new, st);
        if (e->pool_n > 0) HIPCHK(hipMemsetAsync(e->kill.p, 0, (size_t)e->pool_n, st));
        *added = n_new;
        return MVS_OK;
    });
}

int mvs_engine_commit_local(mvs_engine* e) {
    if (!e || !e->staged) { g_err = "mvs_engine_commit_local: no pass to commit"; return MVS_ERR_STATE; }
    HIPCHK(hipSetDevice(e->cfg.device));
    hipStream_t st = e->stream;
    Range rg("mvs:commit");
    return commit_pool(e, [&](int64_t* added) -> int {  // this engine's kill flags and staged records
        if (int r = ensure_counts(e)) return r;
        if (e->pool_n + e->n_new > e->pool.cap) { g_err = "mvs_engine_commit_local: patch pool capacity exceeded (raise mvs_config.max_patches)"; return MVS_ERR_CAPACITY; }
        if (e->n_new > 0) mvsk_commit_copy(e->sa, e->job_base_scan.p, e->pool.p + e->pool_n, e->pool.cap - e->pool_n, nullptr, 0, st);
        mvsk_apply_kill_flags(e->pool.p, e->kill.p, e->pool_n, st);
        *added = e->n_new;
        return MVS_OK;
    });
}

int mvs_engine_propagate(mvs_engine* e, int iter, mvs_counters* out) {  // Propagate::run, propagate.cpp:28-64
    mvs_counters total;
    memset(&total, 0, sizeof total);
    mvs_timing tt{};
    for (int pass = 0; pass < 2; ++pass) {
        mvs_counters c;
        memset(&c, 0, sizeof c);
        const int rp = mvs_engine_pass(e, iter, pass, &c);
        if (e && e->comm) {  // the exchange is reached whatever the pass returned: it is where the ranks agree on a failure
            if (int r = mvs_engine_exchange(e)) return r;
        } else {
            if (rp) { if (e && e->staged) { const std::string keep = g_err; discard_pass(e); g_err = keep; } return rp; }
            if (int r = mvs_engine_commit_local(e)) return r;
        }
        add_counters(total, c);
        tt.index_ms += e->timing.index_ms; tt.sweep_ms += e->timing.sweep_ms; tt.commit_ms += e->timing.commit_ms; tt.sweep_launches += 1;
        tt.exchange_ms += e->timing.exchange_ms; tt.exchange_bytes += e->timing.exchange_bytes; tt.check_retried_cells += e->timing.check_retried_cells;
        tt.sweep_jobs_listed += e->timing.sweep_jobs_listed;
    }
    e->timing = tt;
    if (out) *out = total;
    return MVS_OK;
}

}  // extern "C"
