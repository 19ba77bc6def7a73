// mvs_engine_filter.cpp -- Filter::run of the C ABI in include/mvskit_engine.h: its four stages, the rebuilds between them and, over
// the ranks of a multi-GPU job, the agreement that stands in front of every collective of the call.
//
// A failure on ONE rank inside the collective Filter::run (an allocation that does not fit there, a HIP error) must not leave the
// others waiting in the next broadcast.  Every step of the call goes through FilterRun: after a local failure the rank does no more
// work of its own and only keeps the appointments -- an agreement (one int64 per rank, all-gathered) stands in front of EVERY
// collective of the call, so the next collective any rank reaches is an agreement, in which all ranks see the first failed rank's
// status, give the call up together and return that status (the scheme of mvs_engine_exchange's status word).
#include <climits>
#include <cstdio>
#include <cstdlib>

#include "mvs_engine_impl.h"

using namespace mvseng;

namespace {

// Filter::setDepthMapsVGridsVPGridsAddPatchV, filter.cpp:628-655
// setDepthMapsVGridsVPGridsAddPatchV between the stages of Filter::run.  The depth maps and m_vimages come from the pool; the two
// grid indexes are built only for a stage that walks them: filterOutside (computeGain) reads m_pgrids, filterExact neither,
// filterNeighbor and filterSmallGroups both -- and after the last stage the pool is compacted, which invalidates them anyway.
// Filter::run over the ranks of a multi-GPU job: every stage is a per-patch kernel on a snapshot, so rank r runs it on the patches
// [pool_n r / N, pool_n (r + 1) / N) and the ranks then hand each other what the stage wrote -- its kill bytes, and the records
// themselves where it rewrote lists (filterExact: m_images; setVImagesVGrids: m_vimages) -- as in-place broadcasts of the ranges
// (an all-gather-v without staging; ranges are contiguous and every rank computes the same bounds).  What works on the whole pool
// at once stays replicated: the grid indexes, the depth maps, filterSmallGroups' union-find.  One rank: the whole pool, no exchange.
void filter_range(const mvs_engine* e, int64_t& first, int64_t& last) {
    first = 0; last = e->pool_n;
    if (e->comm && e->comm_world > 1) {
        first = e->pool_n * e->comm_rank / e->comm_world;
        last = e->pool_n * (e->comm_rank + 1) / e->comm_world;
    }
}
struct FilterRun {
    mvs_engine* e;
    int local = MVS_OK;   // first failure on this rank
    std::string err;
    int agreed = MVS_OK;  // != MVS_OK: the ranks have agreed to give the call up with this status
    bool multi() const { return e->comm && e->comm_world > 1; }
    bool live() const { return local == MVS_OK && agreed == MVS_OK; }
    void note(int r) { if (r != MVS_OK && local == MVS_OK) { local = r; err = g_err; } }
};
// runs a step (an expression returning an mvs_status) unless a failure is pending
#define FR(expr) do { if (fr.live()) fr.note(expr); } while (0)
int hip_status(hipError_t e, const char* what) {
    if (e == hipSuccess) return MVS_OK;
    g_err = std::string(what) + ": " + hipGetErrorString(e);
    return MVS_ERR_HIP;
}
#define FRHIP(expr) FR(hip_status((expr), #expr))
#ifdef MVS_FAULT_INJECTION
// test builds only (libmvskit_engine_faultinj.so): MVS_FAULT_FILTER=<rank>:<point> makes that rank fail at that point of Filter::run
void filter_fault_point(FilterRun& fr, int point) {
    const char* f = getenv("MVS_FAULT_FILTER");
    int r = -1, p = -1;
    if (f && fr.live() && sscanf(f, "%d:%d", &r, &p) == 2 && r == fr.e->comm_rank && p == point) {
        g_err = "mvs_engine_filter: failure injected by MVS_FAULT_FILTER";
        fr.note(MVS_ERR_CAPACITY);
    }
}
#else
inline void filter_fault_point(FilterRun&, int) {}
#endif
// the agreement: returns MVS_OK when every rank is fine, else the status all ranks give the call up with
int filter_agree(FilterRun& fr) {
    mvs_engine* e = fr.e;
    if (fr.agreed != MVS_OK) return fr.agreed;
    if (!fr.multi()) {
        if (fr.local != MVS_OK) { fr.agreed = fr.local; g_err = fr.err; }
        return fr.agreed;
    }
    // comm_counts was sized before the first collective of the call; without it not even a status can be sent
    const int64_t mine = fr.local;
    std::vector<int64_t> all((size_t)e->comm_world, 0);
    hipStream_t st = e->stream;
    if (hipMemcpyAsync(e->comm_counts.p, &mine, sizeof mine, hipMemcpyHostToDevice, st) != hipSuccess ||
        rccl().AllGather(e->comm_counts.p, e->comm_counts.p + 1, 1, ncclInt64, e->comm, st) != ncclSuccess ||
        hipMemcpyAsync(all.data(), e->comm_counts.p + 1, all.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) {
        g_err = "mvs_engine_filter: the status all-gather itself failed (the communicator is unusable; the job must be torn down)";
        fr.agreed = MVS_ERR_HIP;
        return fr.agreed;
    }
    for (int r = 0; r < e->comm_world; ++r) {
        if (all[r] == MVS_OK) continue;
        fr.agreed = (int)all[r];
        if (r == e->comm_rank) g_err = fr.err.empty() ? std::string("mvs_engine_filter: this rank failed") : fr.err;
        else g_err = "mvs_engine_filter: rank " + std::to_string(r) + " reported status " + std::to_string((int)all[r]) + "; all ranks give the call up";
        break;
    }
    return fr.agreed;
}
// in-place broadcasts of every rank's share of the kill bytes and / or records; returns != 0 when the call is given up
int filter_exchange(FilterRun& fr, bool kills, bool records) {
    mvs_engine* e = fr.e;
    if (!fr.multi()) return filter_agree(fr);
    if (int a = filter_agree(fr)) return a;
    if (e->pool_n == 0) return MVS_OK;
    const int N = e->comm_world;
    const ncclResult_t first_err = broadcast_blocks(e, [&](int r, auto&& send) {
        const int64_t lo = e->pool_n * r / N, hi = e->pool_n * (r + 1) / N;
        if (kills) send(e->kill.p + lo, hi - lo, ncclUint8);
        if (records) send(e->pool.p + lo, (hi - lo) * (int64_t)sizeof(DPatch), ncclUint8);
        e->fstats_exchange_bytes += (r == e->comm_rank) ? 0 : (kills ? (hi - lo) : 0) + (records ? (hi - lo) * (int64_t)sizeof(DPatch) : 0);
    });
    if (first_err != ncclSuccess) {  // the transport itself: nothing can be agreed on any more
        g_err = std::string("Filter::run exchange: ") + rccl().GetErrorString(first_err);
        fr.note(MVS_ERR_HIP); fr.agreed = MVS_ERR_HIP;
        return fr.agreed;
    }
    return MVS_OK;
}
// Filter::filterSmallGroups with the reference's own labelling (filter.cpp:432-524; mvs_config.literal_groups): a breadth-first search
// in patch order over the DIRECTED relation "q is listed in the 3x3 cells around p in p's reference view and isNeighbor(p, q)" -- the
// first unlabelled patch claims everything it reaches.  On the GPU: (1) the sets joined by edges that run BOTH ways (union-find;
// inside such a set everything reaches everything, so the search claims a set whole or not at all, and the first unlabelled patch
// is always the smallest index of its set = its root); (2) the edges that are left between different sets, as (root, root) pairs --
// a few thousand; (3) on the host, the search over that condensed graph, sets in the order of their roots; (4) the size of its
// literal group written over every set's size, and the removal as usual.
int literal_small_groups(mvs_engine* e, int threshold) {
    hipStream_t st = e->stream;
    const DParams p = current_params(e);
    const int cap = 8 << 20;  // (root, root) pairs
    if (int r = e->group_edges.ensure(2 * (int64_t)cap)) return r;
    int32_t* nedges = reinterpret_cast<int32_t*>(e->misc.p + misc::group_edges);
    HIPCHK(hipMemsetAsync(nedges, 0, sizeof(unsigned long long), st));
    mvsk_groups_literal_edges(p, e->uf_parent.p, e->uf_size.p, e->group_edges.p, nedges, cap, st);
    int32_t ne = 0;
    if (int r = read_back(e, nedges, &ne)) return r;
    HIPCHK(hipGetLastError());
    if (ne > cap) { g_err = "Filter::filterSmallGroups (literal labelling): more than 8 M one-way edges between sets"; return MVS_ERR_CAPACITY; }
    if (ne > 0) {
        std::vector<int32_t> pairs(2 * (size_t)ne);
        HIPCHK(hipMemcpy(pairs.data(), e->group_edges.p, pairs.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        // the sets that have such an edge, in the order of their roots
        std::vector<int32_t> nodes(pairs);
        std::sort(nodes.begin(), nodes.end());
        nodes.erase(std::unique(nodes.begin(), nodes.end()), nodes.end());
        const size_t nn = nodes.size();
        auto idx = [&](int32_t root) { return (size_t)(std::lower_bound(nodes.begin(), nodes.end(), root) - nodes.begin()); };
        std::vector<int32_t> sizes(nn);
        if (int r = e->tmp_i.ensure((int64_t)2 * nn + 16)) return r;
        HIPCHK(hipMemcpy(e->tmp_i.p, nodes.data(), nn * sizeof(int32_t), hipMemcpyHostToDevice));
        mvsk_gather_i32(e->uf_size.p, e->tmp_i.p, e->tmp_i.p + nn, (int64_t)nn, st);
        HIPCHK(hipMemcpyAsync(sizes.data(), e->tmp_i.p + nn, nn * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        std::vector<std::vector<uint32_t>> adj(nn);
        for (int32_t k = 0; k < ne; ++k) adj[idx(pairs[2 * k])].push_back((uint32_t)idx(pairs[2 * k + 1]));
        std::vector<int32_t> label(nn, -1), gsize;
        std::vector<uint32_t> queue;
        for (size_t r0 = 0; r0 < nn; ++r0) {  // ascending roots = ascending first patches
            if (label[r0] != -1) continue;
            const int32_t gid = (int32_t)gsize.size();
            int64_t total = 0;
            queue.assign(1, (uint32_t)r0);
            label[r0] = gid;
            for (size_t qh = 0; qh < queue.size(); ++qh) {
                const uint32_t u = queue[qh];
                total += sizes[u];
                for (uint32_t v : adj[u]) if (label[v] == -1) { label[v] = gid; queue.push_back(v); }
            }
            gsize.push_back((int32_t)std::min<int64_t>(total, INT32_MAX));
        }
        std::vector<int32_t> newsize(nn);
        for (size_t u = 0; u < nn; ++u) newsize[u] = gsize[label[u]];
        HIPCHK(hipMemcpy(e->tmp_i.p + nn, newsize.data(), nn * sizeof(int32_t), hipMemcpyHostToDevice));
        mvsk_scatter_i32(e->uf_size.p, e->tmp_i.p, e->tmp_i.p + nn, (int64_t)nn, st);
    }
    mvsk_groups_kill(p, e->uf_parent.p, e->uf_size.p, threshold, e->kill.p, st);
    return MVS_OK;
}
// `incr` (after a stage's removals, marked by apply_kills): 1 = the depth maps are brought up to date in the marked cells only,
// 2 = and so is m_vimages -- allowed when the stage removed patches and left the lists of the others alone.
int rebuild_head(mvs_engine* e, int additive, bool need_pgrid, int incr) {
    if (need_pgrid) { if (int r = build_list(e, false, false, true)) return r; }
    if (incr && e->dirty_marked) mvsk_depth_maps(current_params(e), e->dpgrid.p, e->dirty.p, e->stream);
    else { incr = 0; if (int r = build_depth(e)) return r; }
    e->dirty_marked = false;
    int64_t first, last;
    filter_range(e, first, last);
    mvsk_filter_vimages(current_params(e), additive, first, last, incr == 2 && additive ? e->dirty.p : nullptr, e->stream);
    return MVS_OK;
}
int rebuild_tail(mvs_engine* e, bool need_vpgrid) {
    if (need_vpgrid) { if (int r = build_list(e, true, false, true)) return r; }
    HIPCHK(hipGetLastError());
    return MVS_OK;
}
// Filter::run never moves a patch, so what its stages read of the patches they MEET -- position, normal, depth scale, score, and (in
// filterOutside, before filterExact picks reference views anew) the reference view -- is packed once per call: 32 bytes + 1 per patch
// instead of a 96-byte record (192 in the 64-view build) that straddles cache lines.  filterNeighbor met ~40 KB of records per patch and ran at
// the HBM rate (5.7 TB/s, profiles/r04_pmc_traffic_per_kernel_filter_run.csv).  A pool with a record whose coord.w / normal.w are not
// 1 / 0 (only a caller's own seeds can be), or no memory for the copy: the stages read the records, as they did.
int pack_geometry(mvs_engine* e) {
    e->geo_valid = false;
    if (e->pool_n <= 0) return MVS_OK;
#ifdef MVS_FAULT_INJECTION  // test builds only: MVS_FAULT_NOPACK=1 keeps Filter::run on the records, so a test can compare the two paths
    if (const char* f = getenv("MVS_FAULT_NOPACK")) { if (atoi(f)) return MVS_OK; }
#endif
    if (e->geo.ensure(2 * e->pool_n) != MVS_OK || e->geo_ref.ensure(e->pool_n) != MVS_OK) { (void)hipGetLastError(); return MVS_OK; }
    hipStream_t st = e->stream;
    int32_t* bad = reinterpret_cast<int32_t*>(e->misc.p + misc::geo_bad);
    HIPCHK(hipMemsetAsync(bad, 0, sizeof(unsigned long long), st));
    mvsk_geo_pack(e->pool.p, e->pool_n, e->geo.p, e->geo_ref.p, bad, st);
    int32_t hbad = 1;
    if (int r = read_back(e, bad, &hbad)) return r;
    HIPCHK(hipGetLastError());
    e->geo_valid = hbad == 0;
    return MVS_OK;
}
// returns != 0 when the call is given up (all ranks alike)
int filter_rebuild(FilterRun& fr, int additive, bool need_pgrid, bool need_vpgrid, int incr = 0) {
    FR(rebuild_head(fr.e, additive, need_pgrid, incr));
    filter_fault_point(fr, 2);
    if (int a = filter_exchange(fr, false, true)) return a;  // m_vimages of the other ranks' patches
    FR(rebuild_tail(fr.e, need_vpgrid));
    return MVS_OK;
}
// counts and applies the kill flags a filter stage has set
// `mark` (inside Filter::run, the depth maps being those of the pool as it stands): the cells that name a patch about to be
// removed are emptied and marked, for filter_rebuild's incremental passes
int apply_kills(mvs_engine* e, int64_t* removed, bool mark = false) {
    hipStream_t st = e->stream;
    *removed = 0;
    e->dirty_marked = false;
    if (e->pool_n == 0) return MVS_OK;
    if (mark) {
        const int64_t words = (e->total_cells + 31) / 32;
        if (int r = e->dirty.ensure(words + 1)) return r;
        HIPCHK(hipMemsetAsync(e->dirty.p, 0, (size_t)words * sizeof(uint32_t), st));
        mvsk_depth_mark_dirty(current_params(e), e->kill.p, e->dpgrid.p, e->dirty.p, st);
        e->dirty_marked = true;
    }
    return count_pool(e, Count::apply_kills, removed);
}

}  // namespace

extern "C" {

int mvs_engine_filter(mvs_engine* e, int64_t* removed4) {  // Filter::run, filter.cpp:25-49
    if (!e || !e->have_views) { g_err = "mvs_engine_filter: views not set"; return MVS_ERR_STATE; }
    if (e->staged) { g_err = "mvs_engine_filter: a pass is waiting for its commit"; return MVS_ERR_STATE; }
    HIPCHK(hipSetDevice(e->cfg.device));
    hipStream_t st = e->stream;
    int64_t rem[4] = {0, 0, 0, 0};
    Range rg("mvs:Filter::run");
    FilterRun fr{e};
    // the one thing without which a rank cannot even report a failure: the word(s) of the agreement
    if (fr.multi()) { if (int r = e->comm_counts.ensure(MVS_XCHG_WORDS * (1 + (int64_t)e->comm_world))) return r; }
    FRHIP(hipEventRecord(e->ev[0], st));
    FRHIP(hipMemsetAsync(e->error_flag.p, 0, sizeof(int32_t), st));
    if (e->pool_n > 0) FRHIP(hipMemsetAsync(e->kill.p, 0, (size_t)e->pool_n, st));
    e->fstats = mvs_filter_stats{};
    FRHIP(hipMemsetAsync(e->fstat_buf.p, 0, fstat::words * sizeof(unsigned long long), st));  // sized by set_views
    FR(mvs_engine_num_patches(e, &e->fstats.patches_in));
    e->fstats_exchange_bytes = 0;
    int64_t first = 0, last = 0;  // this rank's share of the pool (everything on one GPU)
    int32_t herr = 0;
    // every `break` below: the ranks have agreed to give the call up (or, on one GPU, a step failed)
    do {
        if (filter_rebuild(fr, 0, true, false)) break;
        FR(pack_geometry(e));
        FRHIP(hipEventRecord(e->fev[0], st));
        filter_range(e, first, last);
        if (fr.live()) mvsk_filter_outside(current_params(e), e->kill.p, first, last, st);          // filterOutside
        FRHIP(hipEventRecord(e->fev[1], st));
        filter_fault_point(fr, 0);
        if (filter_exchange(fr, true, false)) break;
        FR(apply_kills(e, &rem[0], true));
        // a stage that removed nothing leaves the depth maps, hence m_vimages (additive pass) and both grids, as they are
        if (rem[0] > 0) { if (filter_rebuild(fr, 1, false, false, 2)) break; }
        e->fstats.exact_patches = e->fstats.patches_in - rem[0];
        FRHIP(hipEventRecord(e->fev[2], st));
        filter_range(e, first, last);
#ifdef MVS_STAGE_TIMING
        FRHIP(hipMemsetAsync(e->counters.p, 0, sizeof(DCounters), st));
        if (fr.live()) {
            mvsk_filter_exact(current_params(e), e->kill.p, e->fstat_buf.p + fstat::exact_evals, e->counters.p->stage, first, last, st);
            DCounters hc;
            (void)hipMemcpyAsync(&hc, e->counters.p, sizeof hc, hipMemcpyDeviceToHost, st);
            (void)hipStreamSynchronize(st);
            static const char* nm[8] = {"wave", "frames", "sampling", "pair sums", "choice", "load", "visibility", "lists"};
            fprintf(stderr, "[filterExact cycles]");
            for (int k = 0; k < 8; ++k) fprintf(stderr, " %s %.1f%%", nm[k], 100.0 * (double)hc.stage[k] / (double)(hc.stage[0] ? hc.stage[0] : 1));
            fprintf(stderr, " (wave cycles %.3e)\n", (double)hc.stage[0]);
        }
#else
        if (fr.live()) mvsk_filter_exact(current_params(e), e->kill.p, e->fstat_buf.p + fstat::exact_evals, nullptr, first, last, st);  // filterExact
#endif
        FRHIP(hipEventRecord(e->fev[3], st));
        {
            std::vector<unsigned long long> ev(fstat::words - fstat::exact_evals, 0ull);
            FRHIP(hipMemcpyAsync(ev.data(), e->fstat_buf.p + fstat::exact_evals, ev.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
            FRHIP(hipStreamSynchronize(st));
            unsigned long long ev2[2] = {0, 0};
            for (size_t k = 0; k < ev.size(); ++k) ev2[k & 1] += ev[k];
            e->fstats.exact_view_evals = (int64_t)ev2[1];
        }
        filter_fault_point(fr, 1);
        if (filter_exchange(fr, true, true)) break;  // kill bytes + the rewritten m_images
        FR(apply_kills(e, &rem[1], true));
        if (filter_rebuild(fr, 1, true, true, 1)) break;  // filterExact rewrote m_images: every patch's m_vimages is tested anew
        e->fstats.neighbor_patches = e->fstats.exact_patches - rem[1];
        {                                                                              // filterNeighbor(1)
            FR(e->uf_parent.ensure(e->pool.cap));                                      // reused as the retry list
            FRHIP(hipMemsetAsync(e->misc.p + misc::neighbor_retry, 0, sizeof(unsigned long long), st));
            int32_t* nretry = reinterpret_cast<int32_t*>(e->misc.p + misc::neighbor_retry);
            FRHIP(hipEventRecord(e->fev[4], st));
            if (fr.live() && (!e->lists_dense[0] || !e->lists_dense[1])) { g_err = "Filter::filterNeighbor: the grid indexes must come from a rebuild without the trim"; fr.note(MVS_ERR_ARG); }
            filter_range(e, first, last);
            int32_t nr = 0;
            if (fr.live()) mvsk_filter_neighbor(current_params(e), e->kill.p, e->uf_parent.p, nretry, e->error_flag.p, e->fstat_buf.p + fstat::neighbor_parts, first, last, st);
            FR(read_back(e, nretry, &nr));
            FRHIP(hipGetLastError());
            e->fstats.neighbor_retried = nr;
            if (fr.live()) mvsk_filter_neighbor_retry(current_params(e), e->kill.p, e->uf_parent.p, nr, e->error_flag.p, e->fstat_buf.p + fstat::neighbor_parts, st);
            FRHIP(hipGetLastError());  // a refused launch (LDS request) must not pass for "nothing to filter"
            FRHIP(hipEventRecord(e->fev[5], st));
#ifdef MVS_STAGE_TIMING
            if (fr.live()) {
                unsigned long long hc[16] = {0};
                (void)hipMemcpyAsync(hc, e->fstat_buf.p + fstat::neighbor_cycles, sizeof hc, hipMemcpyDeviceToHost, st);
                (void)hipStreamSynchronize(st);
                const double w = (double)(hc[0] ? hc[0] : 1);
                fprintf(stderr, "[filterNeighbor cycles] load + grids %.1f%% set build %.1f%% gather + predicate %.1f%% filterQuad %.1f%% (wave cycles %.3e)\n",
                        100.0 * hc[1] / w, 100.0 * hc[9] / w, 100.0 * hc[10] / w, 100.0 * hc[11] / w, (double)hc[0]);
            }
#endif
        }
        filter_fault_point(fr, 3);
        if (filter_exchange(fr, true, false)) break;
        FR(apply_kills(e, &rem[2], true));
        // filterNeighbor removes a handful of patches (46 of 6 M in a second call at 1080p): m_pgrids is not rebuilt for them -- its one
        // reader left, filterSmallGroups, skips a listed patch that is dead (k_groups_edges) -- while m_vpgrids is, because the removals
        // can ADD memberships (a patch becomes visible where its occluder went)
        if (rem[2] > 0) { if (filter_rebuild(fr, 1, false, true, 2)) break; }
        {                                                                              // filterSmallGroups (replicated: every rank on the whole pool)
            int64_t alive = 0;
            FR(mvs_engine_num_patches(e, &alive));
            FR(e->uf_parent.ensure(e->pool.cap));
            FR(e->uf_size.ensure(e->pool.cap));
            const int threshold = (int)std::max<int64_t>(20, alive / 10000);
            FRHIP(hipEventRecord(e->fev[6], st));
            if (fr.live()) {
                if (!e->cfg.literal_groups) mvsk_groups(current_params(e), e->uf_parent.p, e->uf_size.p, threshold, e->kill.p, st);
                else fr.note(literal_small_groups(e, threshold));
            }
            FRHIP(hipEventRecord(e->fev[7], st));
            FR(apply_kills(e, &rem[3], true));
        }
        if (rem[3] > 0) { if (filter_rebuild(fr, 1, false, false, 2)) break; }
        FR(compact_pool(e));
        FRHIP(hipMemcpyAsync(&herr, e->error_flag.p, sizeof herr, hipMemcpyDeviceToHost, st));
        FRHIP(hipEventRecord(e->ev[1], st));
        FRHIP(hipStreamSynchronize(st));
        FRHIP(hipGetLastError());
        if (fr.live() && (herr & 4)) {  // this rank's share met the engine's limit: every rank returns that status
            g_err = "mvs_engine_filter: more than 14336 patches around one patch, or more than 4064 neighbours (engine limit)";
            fr.note(MVS_ERR_CAPACITY);
        }
    } while (0);
    const int status = filter_agree(fr);  // the closing agreement (one GPU: this rank's own status)
    e->geo_valid = false;  // compact_pool renumbers the patches
    if (status != MVS_OK) {
        // given up: what the unfinished stage marked is forgotten.  The stages that completed stand (on every rank alike); a stage that
        // was under way may have rewritten the lists of this rank's share only -- after an error the caller re-uploads or stops.
        const std::string keep = g_err;
        if (e->kill.p && e->pool_n > 0) (void)hipMemsetAsync(e->kill.p, 0, (size_t)e->pool_n, st);
        (void)hipStreamSynchronize(st);
        (void)hipGetLastError();
        e->dirty_marked = false;
        g_err = keep;
        return status;
    }
    float ms = 0.0f;
    (void)hipEventElapsedTime(&ms, e->ev[0], e->ev[1]);
    e->timing = mvs_timing{};
    e->timing.index_ms = ms;  // whole Filter::run
    {
        mvs_filter_stats& f = e->fstats;
        f.total_ms = ms;
        (void)hipEventElapsedTime(&f.outside_ms, e->fev[0], e->fev[1]);
        (void)hipEventElapsedTime(&f.exact_ms, e->fev[2], e->fev[3]);
        (void)hipEventElapsedTime(&f.neighbor_ms, e->fev[4], e->fev[5]);
        (void)hipEventElapsedTime(&f.groups_ms, e->fev[6], e->fev[7]);
        f.rebuild_ms = f.total_ms - f.outside_ms - f.exact_ms - f.neighbor_ms - f.groups_ms;  // rebuilds + the scans between the stages
        std::vector<unsigned long long> part(fstat::neighbor_cycles - fstat::neighbor_parts);
        HIPCHK(hipMemcpy(part.data(), e->fstat_buf.p + fstat::neighbor_parts, part.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        unsigned long long sum4[4] = {0, 0, 0, 0};
        for (size_t k = 0; k < part.size(); ++k) sum4[k & 3] += part[k];
        f.neighbor_tasks = (int64_t)sum4[0]; f.neighbor_entries = (int64_t)sum4[1]; f.neighbor_visited = (int64_t)sum4[2]; f.neighbor_accepted = (int64_t)sum4[3];
    }
    e->fstats.exchange_bytes = e->fstats_exchange_bytes;
    if (removed4) for (int k = 0; k < 4; ++k) removed4[k] = rem[k];
    return MVS_OK;
}

int mvs_engine_filter_stats(mvs_engine* e, mvs_filter_stats* out) {
    if (!e || !out) return MVS_ERR_ARG;
    *out = e->fstats;
    return MVS_OK;
}

}  // extern "C"
