// mvs_engine_impl.h -- what the host units of the C ABI (mvs_engine*.cpp) share, and nothing else: the error string and HIPCHK, the
// owning device buffer, the slot tables of the scratch words, the tracing ranges, the RCCL entry points, struct mvs_engine and the
// helpers that more than one unit calls.  The non-template helpers have external linkage in namespace mvseng, so that nothing here can
// collide with what a host application links; what one unit alone uses stays in that unit's anonymous namespace.  Internal: no device
// compilation reads this file.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>  // types only: librccl is opened at run time (see Rccl below)

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "mvskit_engine.h"
#include "mvs_kernels.h"
#include "mvs_types.h"

namespace mvseng {
extern thread_local std::string g_err;  // mvs_last_error (defined in mvs_engine.cpp)
}

#define HIPCHK(expr)                                                                                       \
    do {                                                                                                   \
        hipError_t _e = (expr);                                                                            \
        if (_e != hipSuccess) {                                                                            \
            mvseng::g_err = std::string(#expr) + ": " + hipGetErrorString(_e);                             \
            return MVS_ERR_HIP;                                                                            \
        }                                                                                                  \
    } while (0)

#define MVS_XCHG_WORDS 5  // what a rank tells the others before anything is moved: {new records, evicted ids, status, pool headroom, kill-id capacity}

namespace mvseng {

// Device memory owned by the engine: freed by the destructor, with whatever device is current (the engine's: every entry point
// sets it first).  Not copyable; a move (the view pyramids' vectors) or a swap of the storage is.
template <typename T> struct DevBuf {
    T* p = nullptr;
    int64_t cap = 0;
    bool headroom = false;  // the cell indexes only: a buffer that has to grow a second time takes half as much again
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap), headroom(o.headroom) { o.p = nullptr; o.cap = 0; }
    ~DevBuf() { release(); }
    void swap(DevBuf& o) { std::swap(p, o.p); std::swap(cap, o.cap); }  // the storage only: `headroom` belongs to the member
    int ensure(int64_t n) {
        if (n <= cap) return MVS_OK;
        // (headroom) The cell indexes of a pool that grows from iteration to iteration: freeing and allocating 10 GB costs ~100 ms, and an
        // exact fit did it at every index build of a 48 x 4K run.  (A caller that knows how large its pool will get sizes the indexes
        // up front: mvs_engine_reserve.)  Every other buffer gets exactly what it asks for.
        const int64_t exact = std::max<int64_t>(n, 16);
        int64_t want = (p && headroom) ? exact + exact / 2 : exact;
        // The contents are never needed across a growth.  The new buffer is allocated before the old one is freed where both fit; if
        // they do not fit side by side, the old one is freed first, and a failure then leaves the buffer empty (cap 0).
        T* q = nullptr;
        hipError_t e = hipMalloc((void**)&q, (size_t)want * sizeof(T));
        if (e != hipSuccess && want > exact) { (void)hipGetLastError(); want = exact; e = hipMalloc((void**)&q, (size_t)want * sizeof(T)); }  // no room for the headroom
        if (e != hipSuccess && p) {
            (void)hipGetLastError();
            (void)hipFree(p); p = nullptr; cap = 0;
            e = hipMalloc((void**)&q, (size_t)want * sizeof(T));
        }
        if (e != hipSuccess) { (void)hipGetLastError(); g_err = std::string("hipMalloc: ") + hipGetErrorString(e); return MVS_ERR_HIP; }
        if (p) (void)hipFree(p);
        p = q; cap = want;
        return MVS_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

// The scratch words of mvs_engine::misc (unsigned long long; a count that a kernel keeps as int32 uses the low half of its word)
namespace misc {
constexpr int stage_counter = 0;   // the sweep's staging counter (SweepArgs::stage_counter)
constexpr int fill_evals = 1;      // [2] mvsk_fill_ncc: evaluations and view evaluations spent on seeds whose m_ncc was < 0
constexpr int neighbor_retry = 4;  // filterNeighbor: the number of patches for its retry launch
constexpr int sweep_retry = 5;     // the sweep: the number of cells for Optim::check's second tier (SweepArgs::nretry)
constexpr int geo_bad = 6;         // pack_geometry: a record that cannot be packed
constexpr int group_edges = 7;     // the literal filterSmallGroups: the number of one-way edges between sets
constexpr int trim_parts = 8;      // [trim_nparts] the MAX_NUM_OF_PATCHES trim's count as partial sums
constexpr int trim_nparts = 256;   // (k_index_sort_trim: one per block index mod 256)
// the sweep's queue cursors (SweepArgs::cursors, uint32 each): eight 128-byte lines, the first on a line boundary of the buffer
constexpr int sweep_cursors = (trim_parts + trim_nparts + 15) / 16 * 16;
constexpr int sweep_cursor_words = MVS_SWEEP_QUEUES * MVS_SWEEP_CURSOR_STRIDE * (int)sizeof(uint32_t) / (int)sizeof(unsigned long long);
// behind them, cleared with them: the bounds of the sweep's job lists (SweepArgs::list_bounds, int32 each; the last = jobs listed)
constexpr int sweep_list_bounds = sweep_cursors + sweep_cursor_words;
constexpr int sweep_list_bound_words = (MVS_SWEEP_QUEUES + 1 + 1) / 2;
constexpr int words = sweep_list_bounds + sweep_list_bound_words;
// the scratch of mvsk_job_list holds a flag per job of the launch's range, rounded up to whole chunks in every queue
constexpr int64_t job_list_pad = 1024 + 2;
}  // namespace misc
// The words of mvs_engine::fstat_buf (Filter::run's statistics).  k_filter_neighbor fixes the first two ranges itself.
namespace fstat {
constexpr int neighbor_parts = 0;      // [1024][4] partial sums of filterNeighbor's work counts
constexpr int neighbor_cycles = 4096;  // [16] filterNeighbor's stage cycles (-DMVS_STAGE_TIMING)
constexpr int exact_evals = 4112;      // [1024][2] partial sums of filterExact's evaluations and view evaluations
constexpr int words = exact_evals + 2048;
}  // namespace fstat

// RCCL, opened at run time (mvs_engine_comm.cpp).  A process that has loaded torch already holds torch's own librccl: that copy is
// reused (one RCCL per process); otherwise the ROCm installation's is opened.  Nothing here is needed on one GPU.
struct Rccl {
    void* h = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*CommCount)(const ncclComm_t, int*) = nullptr;     // optional (mvs_engine_comm_info)
    ncclResult_t (*CommUserRank)(const ncclComm_t, int*) = nullptr;  // optional
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Broadcast)(const void*, void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    bool ok = false;
};
Rccl& rccl();

// roctx ranges (tracing) around upload / index build / colour-pass sweep / exchange / commit /
// Filter::run stages; libroctx64 is opened at run time (mvs_engine.cpp) and the ranges cost nothing when no profiler listens.
struct Roctx {
    int (*push)(const char*) = nullptr;
    int (*pop)() = nullptr;
};
Roctx& roctx();
struct Range {
    bool on;
    explicit Range(const char* name) : on(roctx().push != nullptr) { if (on) roctx().push(name); }
    ~Range() { if (on) roctx().pop(); }
    Range(const Range&) = delete;
    Range& operator=(const Range&) = delete;
};

}  // namespace mvseng

using mvseng::DevBuf;  // the handle's struct is the C ABI's own name: it stays at global scope
struct mvs_engine {
    mvs_config cfg{};
    mvs_refiner refiner{MVS_REFINE_HALVING, 500, 1e-4f};  // mvs_engine_set_refiner
    DParams prm{};
    hipStream_t stream = nullptr;
    bool have_views = false;
    std::vector<DView> hviews;
    DevBuf<DView> dviews;
    DevBuf<uint8_t> pyr;                     // the pyramid levels of all views in one block (DView::img / img_off)
    bool pyr_narrow = false;                 // ... which 32-bit byte offsets can address (DParams::pyr32)
    std::vector<DevBuf<uint8_t>> mask_bufs;  // and masks (DView::mask) of the views
    int total_cells = 0;
    // pool
    DevBuf<DPatch> pool, pool_alt;  // pool_alt: target of the stable compaction done at every commit
    DevBuf<uint8_t> kill;
    int64_t pool_n = 0;
    bool ncc_dirty = false;
    // index
    DevBuf<int32_t> cnt, cursor, vcnt, vcursor;
    DevBuf<csr_off_t> start, vstart;       // list offsets (64-bit)
    DevBuf<csr_off_t> start_raw;           // m_pgrids offsets of a build with the trim, before the lists are packed end to end
    DevBuf<int32_t> id32_raw;              // ... and its ids, each list compacted to the front of its own range
    DevBuf<int64_t> scan_tmp;              // block sums of the scans (used as int32 or as csr_off_t)
    DevBuf<unsigned long long> ids;        // the (descending ncc, id) sort keys of an index build: transient, one buffer serves both grids
    DevBuf<ListKey> key;                   // (m_ncc, reference view) per m_pgrids entry
    DevBuf<int32_t> id32, vid32;           // the ids alone
    DevBuf<int32_t> uf_parent, uf_size;  // Filter::filterSmallGroups union-find
    DevBuf<int32_t> group_edges;         // its literal labelling: (root, root) pairs of the one-way edges between sets
    DevBuf<int32_t> cnt_alive, vcnt_alive;
    DevBuf<unsigned long long> dpgrid, best;
    DevBuf<uint32_t> dirty;      // Filter::run: one bit per depth-map cell whose nearest patch the last stage removed
    bool dirty_marked = false;
    DevBuf<float4> geo;            // Filter::run: the packed geometry of the pool (DParams::geo), 2 words per patch
    DevBuf<uint8_t> geo_ref;       //              and the reference views
    bool geo_valid = false;        // between pack_geometry and the end of that Filter::run
    bool lists_dense[2] = {false, false};  // m_pgrids / m_vpgrids index built without the trim: the lists of neighbouring cells lie end to end
    // sweep / staging
    DevBuf<DPatch> staging;
    DevBuf<int32_t> job_stage, job_nstage, job_cnt, job_base_scan, kill_cnt, kill_base;
    DevBuf<unsigned long long> misc;  // scratch words: namespace misc
    DevBuf<DCounters> counters;
    DevBuf<int32_t> error_flag;
    DevBuf<int32_t> big_tables, retry_jobs;  // Optim::check's second tier (k_sweep_retry): 256 id sets of 16384 ints, the cells to run again
    DevBuf<int32_t> job_list;                // the jobs of a launch that run a trial, per queue (SweepArgs::job_list); its flags and their scan
                                             // lie in job_cnt and job_base_scan, which the commit fills only after the sweep
    int64_t sweep_pairs[6] = {0, 0, 0, 0, 0, 0};  // DCounters::pair, summed over the passes since the engine was created (mvs_engine_sweep_pairs)
    int64_t sweep_repeats[2] = {0, 0};            // DCounters::repeats, likewise (mvs_engine_sweep_repeats)
    int64_t sweep_kernels[2] = {0, 0};            // sweep launches by kernel: generic, full-window (mvs_engine_sweep_kernels)
    int64_t sampler_launches[4] = {0, 0, 0, 0};   // sweep launches, then refine probes, by the form of their samplers: wide, narrow (mvs_engine_sampler_launches)
    int64_t retried_cells = 0;               // destination cells that went to the second tier since the engine was created
    int64_t pass_retried = 0;                // ... in the last pass
    SweepArgs sa{};
    bool staged = false;      // a pass has run and was not committed yet
    bool counted = false;     // commit_count + scans done for the staged pass
    int64_t n_new = 0, n_kill = 0;
    std::vector<int32_t> h_per_view;
    // probes / downloads
    DevBuf<DPatch> tmp_rec_in, tmp_rec_out;
    DevBuf<float> tmp_f_in, tmp_f_out;
    DevBuf<int32_t> tmp_i;
    DevBuf<uint8_t> tmp_bytes;
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    mvs_timing timing{};
    mvs_filter_stats fstats{};
    int64_t fstats_exchange_bytes = 0;  // bytes this rank received in the last Filter::run's exchanges
    DevBuf<unsigned long long> fstat_buf;  // Filter::run's statistics: namespace fstat
    hipEvent_t fev[10] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    // multi-GPU (mvs_engine_comm_*): one RCCL communicator over the engines of the job
    ncclComm_t comm = nullptr;
    bool comm_owned = false;
    int comm_rank = 0, comm_world = 1;
    DevBuf<int64_t> comm_counts;   // [MVS_XCHG_WORDS] mine + [MVS_XCHG_WORDS * world] gathered
    DevBuf<int32_t> comm_kill_ids; // all ranks' kill ids
    int pass_status = MVS_OK;      // what the last mvs_engine_pass returned: the exchange carries it to the other ranks
    std::string pass_error;
    bool fault_fired = false;      // MVS_FAULT_PASS (fault injection, see pass_impl) fires once per engine
};

namespace mvseng {

// ---- mvs_engine.cpp
RefineSel refine_sel(const mvs_engine* e);
DParams current_params(mvs_engine* e);
bool want_vgrid(const mvs_engine* e);
// The state an entry point asks of its handle, each level with those before it, checked in this order: a handle, views, no pass waiting
// for its commit.  An entry point that has checks of its own between two of them asks twice.
enum Need { NEED_ENGINE, NEED_VIEWS, NEED_IDLE };
int need_state(const mvs_engine* e, Need need, const char* who);
// flags[0, n) -> base[0, n], their exclusive scan, and *count = base[n], the number of set flags, read back: the stream is idle on return
// (scan: n / 256 + 4096 ints of scratch)
int scan_total(mvs_engine* e, const int32_t* flags, int32_t* base, int32_t* scan, int64_t n, int64_t* count);

// ---- mvs_engine_pass.cpp
// One cell index (m_pgrids or m_vpgrids): count -> scan -> fill -> per-cell sort (ncc desc, id asc) [-> trim to
// MAX_NUM_OF_PATCHES] -> compaction to alive entries, written out as id (and ListKey) streams.
// `unordered` (the rebuilds inside Filter::run, never with the trim): the entries of a list in no particular order, see k_index_fill_direct
int build_list(mvs_engine* e, bool vgrid, bool trim, bool unordered = false);
int build_depth(mvs_engine* e);  // m_dpgrids from the alive pool
// Index build of a propagation pass: seed scores, m_pgrids lists with the MAX_NUM_OF_PATCHES trim, m_vpgrids lists
// (needed by Optim::check), depth maps.
int build_index(mvs_engine* e, unsigned long long* trimmed_out);
// What count_pool counts: the alive records, the kill flags, or the kill flags that are then applied (mvsk_apply_kill_flags, queued
// in front of the wait so that the device does not idle between the read-back and the apply)
enum class Count { alive, kills, apply_kills };
// Count, exclusive scan, total over the pool's slots: kill_cnt[i] = 1 where slot i holds an alive record (Count::alive) or carries a
// kill flag (the other two), kill_base = the exclusive scan of kill_cnt, and *total = kill_base[pool_n], read back after a
// synchronisation.  Until the next call kill_base[i] is the number of counted slots before slot i: mvsk_kill_export reads it after
// a count of the kill flags, the gathers of mvs_engine_download_patches and mvs_engine_export_ply after one of the alive records.
int count_pool(mvs_engine* e, Count what, int64_t* total);
int ensure_counts(mvs_engine* e);  // commit_count + scans for the staged pass
// Stable compaction of the pool: dead records (evicted, trimmed) are dropped, the relative order of the
// survivors -- the only thing ids are used for -- is kept.  Runs at every commit, on every rank alike.
int compact_pool(mvs_engine* e);
// forgets a staged pass (after an error): its records are dropped, the eviction flags it set are cleared, the pool is as it
// was when the pass began (minus the patches the MAX_NUM_OF_PATCHES trim removed, which every rank removes alike)
void discard_pass(mvs_engine* e);

// One scalar of device memory read back on the engine's stream: the stream is idle on return.  For the places that do exactly this
// and queue nothing between the copy and the wait (count_pool, which does, writes the two calls out).
template <typename T> int read_back(mvs_engine* e, const T* dev, T* host) {
    HIPCHK(hipMemcpyAsync(host, dev, sizeof(T), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return MVS_OK;
}

// The tail of every commit (mvs_engine_commit_device, mvs_engine_commit_local, and mvs_engine_exchange for the union of the ranks):
// apply(&n_new) evicts the pass's patches, leaves the kill bytes clear and puts the n_new new records behind the pool; the pool then
// takes them in and is compacted.  The whole is timed as commit_ms.
template <typename Apply> int commit_pool(mvs_engine* e, Apply&& apply) {
    hipStream_t st = e->stream;
    HIPCHK(hipEventRecord(e->ev[2], st));
    int64_t n_new = 0;
    if (int r = apply(&n_new)) return r;
    e->pool_n += n_new;
    if (int r = compact_pool(e)) return r;
    HIPCHK(hipEventRecord(e->ev[3], st));
    HIPCHK(hipStreamSynchronize(st));
    float ms = 0.0f;
    (void)hipEventElapsedTime(&ms, e->ev[2], e->ev[3]);
    e->timing.commit_ms = ms;
    e->staged = false; e->counted = false;
    return MVS_OK;
}

// An all-gather-v without staging: every rank's blocks broadcast in place from that rank, all in one group.  blocks(r, send) calls
// send(ptr, count, type) for each block of rank r; empty blocks are skipped.  An error inside the group still closes it (a group left
// open would swallow every later call of this thread); the first error is returned.
template <typename Blocks> ncclResult_t broadcast_blocks(mvs_engine* e, Blocks&& blocks) {
    const Rccl& R = rccl();
    ncclResult_t first = R.GroupStart();
    for (int r = 0; r < e->comm_world && first == ncclSuccess; ++r)
        blocks(r, [&](void* p, int64_t n, ncclDataType_t type) {
            if (n > 0 && first == ncclSuccess) first = R.Broadcast(p, p, (size_t)n, type, r, e->comm, e->stream);
        });
    const ncclResult_t end = R.GroupEnd();
    return first == ncclSuccess ? end : first;
}

// ---- mvs_engine_output.cpp
// The buffers of a call that starts from the dense maps (the maps calls themselves, and the mesh calls of mvs_engine_mesh.cpp)
struct MapsBufs {
    MapsArgs args{};
    int64_t total_pix = 0, max_pix = 0;
    DevBuf<int32_t> ids;             // [total_pix] the pool index behind every pixel of every view, -1 = invalid
    DevBuf<float> pts;               // [3 total_pix] its point
    DevBuf<unsigned long long> agree;  // the views stream through these: [max_pix] each
    DevBuf<int32_t> flag, base, scan;
    DevBuf<float> maps;              // [5 max_pix] depth, normal, conf of the view under way
    DevBuf<uint8_t> flag8;           // [total_pix] fused_points: the emitted pixels, between its counting and its gathering pass
    DevBuf<mvs_fused_point> recs;    // fused_points: the records of one view
};
int maps_args(const mvs_maps_config* c, const char* who);  // the checks of a mvs_maps_config that need no handle
int maps_state(const mvs_engine* e, const mvs_maps_config* c, const char* who);
int64_t maps_npix(const mvs_engine* e, int v);
int render_all(mvs_engine* e, const mvs_maps_config* c, MapsBufs& b);     // steps 1 and 2 for every view: b.ids and b.pts
int render_usable(mvs_engine* e, const mvs_maps_config* c, MapsBufs& b);  // and their usability, a byte per pixel of all views: b.flag8

}  // namespace mvseng
