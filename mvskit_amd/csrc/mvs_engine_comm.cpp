// mvs_engine_comm.cpp -- multi-GPU through the C ABI in include/mvskit_engine.h: the RCCL loader, the communicator calls and the
// per-pass exchange.  A pass that failed (staging or Optim::check capacity in this rank's shard, a HIP error) leaves its status in the
// engine (mvs_engine_pass): the exchange hands it to every rank, so that all of them give the pass up together instead of waiting in
// a collective for a rank that has already returned.
#include <dlfcn.h>

#include <climits>
#include <cstdlib>
#include <cstring>

#include "mvs_engine_impl.h"

using namespace mvseng;

#define NCCLCHK(expr)                                                                                      \
    do {                                                                                                   \
        ncclResult_t _r = (expr);                                                                          \
        if (_r != ncclSuccess) {                                                                           \
            g_err = std::string(#expr) + ": " + rccl().GetErrorString(_r);                                 \
            return MVS_ERR_HIP;                                                                            \
        }                                                                                                  \
    } while (0)

namespace mvseng {

Rccl& rccl() {
    static Rccl r;
    static bool tried = false;
    if (tried) return r;
    tried = true;
    // MVS_CCL_LIBRARY: another library with the same eight entry points (a site's own RCCL build; the shared-memory
    // loopback of tests/loopback_ccl, which lets several ranks share the one GPU of a test box)
    if (const char* over = getenv("MVS_CCL_LIBRARY")) {
        if (*over) { r.h = dlopen(over, RTLD_NOW | RTLD_LOCAL); if (!r.h) return r; }
    }
    const char* names[] = {"librccl.so", "librccl.so.1"};
    for (const char* n : names) if (!r.h) r.h = dlopen(n, RTLD_NOW | RTLD_NOLOAD);
    const char* paths[] = {"/opt/rocm/lib/librccl.so.1", "librccl.so.1", "librccl.so"};
    for (const char* n : paths) if (!r.h) r.h = dlopen(n, RTLD_NOW | RTLD_LOCAL);
    if (!r.h) return r;
#define MVS_SYM(field, name) r.field = reinterpret_cast<decltype(r.field)>(dlsym(r.h, name))
    MVS_SYM(GetUniqueId, "ncclGetUniqueId"); MVS_SYM(CommInitRank, "ncclCommInitRank"); MVS_SYM(CommDestroy, "ncclCommDestroy");
    MVS_SYM(AllGather, "ncclAllGather"); MVS_SYM(Broadcast, "ncclBroadcast"); MVS_SYM(GroupStart, "ncclGroupStart");
    MVS_SYM(GroupEnd, "ncclGroupEnd"); MVS_SYM(GetErrorString, "ncclGetErrorString");
    MVS_SYM(CommCount, "ncclCommCount"); MVS_SYM(CommUserRank, "ncclCommUserRank");
#undef MVS_SYM
    r.ok = r.GetUniqueId && r.CommInitRank && r.CommDestroy && r.AllGather && r.Broadcast && r.GroupStart && r.GroupEnd && r.GetErrorString;
    return r;
}

}  // namespace mvseng

extern "C" {

// ---- multi-GPU: RCCL communicator + the per-pass exchange (include/mvskit_engine.h, "multi-GPU through the C ABI")
int mvs_comm_unique_id(void* id_out) {
    if (!id_out) return MVS_ERR_ARG;
    static_assert(sizeof(ncclUniqueId) == MVS_COMM_ID_BYTES, "ncclUniqueId is 128 bytes");
    if (!rccl().ok) { g_err = "mvs_comm_unique_id: librccl could not be opened"; return MVS_ERR_STATE; }
    ncclUniqueId id;
    NCCLCHK(rccl().GetUniqueId(&id));
    memcpy(id_out, &id, sizeof id);
    return MVS_OK;
}
static int comm_check(mvs_engine* e, int rank, int world, const char* who) {
    if (!e || world < 1 || rank < 0 || rank >= world) { g_err = std::string(who) + ": bad rank / world"; return MVS_ERR_ARG; }
    if (e->comm) { g_err = std::string(who) + ": a communicator is already attached"; return MVS_ERR_STATE; }
    const int sc = e->cfg.shard_count > 1 ? e->cfg.shard_count : 1, si = e->cfg.shard_count > 1 ? e->cfg.shard_index : 0;
    if (sc != world || si != rank || e->cfg.view_begin != 0 || e->cfg.view_stride != 1) {
        g_err = std::string(who) + ": the engine must be created with shard_index = rank and shard_count = world (contiguous job ranges: rank order is the commit order)";
        return MVS_ERR_ARG;
    }
    if (!rccl().ok) { g_err = std::string(who) + ": librccl could not be opened"; return MVS_ERR_STATE; }
    return MVS_OK;
}
int mvs_engine_comm_init(mvs_engine* e, const void* id, int rank, int world) {
    if (!id) return MVS_ERR_ARG;
    if (int r = comm_check(e, rank, world, "mvs_engine_comm_init")) return r;
    HIPCHK(hipSetDevice(e->cfg.device));
    ncclUniqueId uid;
    memcpy(&uid, id, sizeof uid);
    ncclComm_t c = nullptr;
    NCCLCHK(rccl().CommInitRank(&c, world, uid, rank));
    e->comm = c; e->comm_owned = true; e->comm_rank = rank; e->comm_world = world;
    return MVS_OK;
}
int mvs_engine_comm_attach(mvs_engine* e, void* nccl_comm, int rank, int world) {
    if (!nccl_comm) return MVS_ERR_ARG;
    if (int r = comm_check(e, rank, world, "mvs_engine_comm_attach")) return r;
    e->comm = (ncclComm_t)nccl_comm; e->comm_owned = false; e->comm_rank = rank; e->comm_world = world;
    return MVS_OK;
}
int mvs_engine_comm_release(mvs_engine* e) {
    if (!e) return MVS_ERR_ARG;
    if (e->comm && e->comm_owned && rccl().ok) {
        (void)hipSetDevice(e->cfg.device);
        (void)hipStreamSynchronize(e->stream);
        (void)rccl().CommDestroy(e->comm);
    }
    e->comm = nullptr; e->comm_owned = false; e->comm_rank = 0; e->comm_world = 1;
    return MVS_OK;
}

int mvs_engine_comm_info(mvs_engine* e, int* rank, int* world, int* comm_count, int* comm_rank) {
    if (!e) return MVS_ERR_ARG;
    if (rank) *rank = e->comm_rank;
    if (world) *world = e->comm ? e->comm_world : 0;  // 0: no communicator attached
    int cc = -1, cr = -1;  // what the communicator itself says (ncclCommCount / ncclCommUserRank), -1 where it cannot be asked
    if (e->comm && rccl().ok) {
        if (rccl().CommCount && rccl().CommCount(e->comm, &cc) != ncclSuccess) cc = -1;
        if (rccl().CommUserRank && rccl().CommUserRank(e->comm, &cr) != ncclSuccess) cr = -1;
    }
    if (comm_count) *comm_count = cc;
    if (comm_rank) *comm_rank = cr;
    return MVS_OK;
}

int mvs_engine_exchange(mvs_engine* e) {
    if (!e) { g_err = "mvs_engine_exchange: null engine"; return MVS_ERR_ARG; }
    if (!e->comm) { g_err = "mvs_engine_exchange: no communicator (mvs_engine_comm_init / _attach)"; return MVS_ERR_STATE; }
    if (!e->staged && e->pass_status == MVS_OK) { g_err = "mvs_engine_exchange: no pass to exchange"; return MVS_ERR_STATE; }
    HIPCHK(hipSetDevice(e->cfg.device));
    hipStream_t st = e->stream;
    const Rccl& R = rccl();
    const int world = e->comm_world, rank = e->comm_rank;
    Range rg("mvs:exchange");
    // (0) everything that can fail on this rank alone happens BEFORE the first collective and ends up in a status word
    int local = e->pass_status;
    std::string local_err = e->pass_error;
    auto fail_local = [&](int r) { if (local == MVS_OK) { local = r; local_err = g_err; } };
    if (hipEventRecord(e->ev[4], st) != hipSuccess) { g_err = "mvs_engine_exchange: hipEventRecord failed"; fail_local(MVS_ERR_HIP); }
    if (local == MVS_OK) { if (int r = ensure_counts(e)) fail_local(r); }
    if (int r = e->comm_counts.ensure(MVS_XCHG_WORDS * (1 + (int64_t)world))) fail_local(r);
    // the evicted ids of all ranks (a rank evicts pool patches from its own cells only, but a patch sits in the cells of several
    // views, so the union may name an id twice): one allocation of pool-capacity ids, the limit agreed as the minimum over the ranks
    if (int r = e->comm_kill_ids.ensure(std::max<int64_t>(e->pool.cap, 1024))) fail_local(r);
    // The ONE way out before the first collective: no device word to put the status in (a 40-byte allocation failed).  This rank
    // can then tell nobody anything; the other ranks wait in their all-gather until the launcher tears the job down (bench.py's
    // spawn_ranks and torch.distributed.run both end the job when a rank exits non-zero) -- INTEGRATION.md, "failures".
    if (!e->comm_counts.p) { g_err = "mvs_engine_exchange: no device memory for the status word; the job must be torn down by its launcher"; return MVS_ERR_HIP; }
    if (local != MVS_OK) { e->n_new = 0; e->n_kill = 0; }
    // (1) one all-gather of MVS_XCHG_WORDS int64 per rank.  A failure of the host-to-device copy of this rank's words does not skip
    // the collective: the status word is then written by a kernel-free fallback (hipMemsetD32Async of the status alone), so the
    // others still see a failure and nobody waits; a failure of the all-gather or of its read-back is a failure of the transport
    // itself -- past that nothing can be agreed on.
    int64_t mine[MVS_XCHG_WORDS] = {e->n_new, e->n_kill, (int64_t)local, e->pool.cap - e->pool_n, e->comm_kill_ids.cap};
    std::vector<int64_t> all(MVS_XCHG_WORDS * (size_t)world);
    if (hipMemcpyAsync(e->comm_counts.p, mine, sizeof mine, hipMemcpyHostToDevice, st) != hipSuccess) {
        (void)hipGetLastError();
        g_err = "mvs_engine_exchange: host-to-device copy of the count words failed"; fail_local(MVS_ERR_HIP);
        // {0, 0, MVS_ERR_HIP, 0, 0}: zero the words, then the status as an int64 -- low word MVS_ERR_HIP, high word all ones
        (void)hipMemsetAsync(e->comm_counts.p, 0, sizeof mine, st);
        int32_t* status = reinterpret_cast<int32_t*>(e->comm_counts.p + 2);
        (void)hipMemsetD32Async((hipDeviceptr_t)status, (int)MVS_ERR_HIP, 1, st);
        (void)hipMemsetD32Async((hipDeviceptr_t)(status + 1), -1, 1, st);
    }
    NCCLCHK(R.AllGather(e->comm_counts.p, e->comm_counts.p + MVS_XCHG_WORDS, MVS_XCHG_WORDS, ncclInt64, e->comm, st));
    HIPCHK(hipMemcpyAsync(all.data(), e->comm_counts.p + MVS_XCHG_WORDS, all.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    std::vector<int64_t> off_new(world + 1, 0), off_kill(world + 1, 0);
    int64_t headroom = INT64_MAX, kill_cap = INT64_MAX;
    int bad_rank = -1, bad_status = MVS_OK;
    for (int r = 0; r < world; ++r) {
        const int64_t* w = &all[MVS_XCHG_WORDS * (size_t)r];
        off_new[r + 1] = off_new[r] + w[0]; off_kill[r + 1] = off_kill[r] + w[1];
        if (w[2] != MVS_OK && bad_rank < 0) { bad_rank = r; bad_status = (int)w[2]; }
        headroom = std::min(headroom, w[3]); kill_cap = std::min(kill_cap, w[4]);
    }
    const int64_t tot_new = off_new[world], tot_kill = off_kill[world];
    // every rank sees the same words and takes the same way out: the pass is given up everywhere, nobody waits
    if (bad_rank >= 0) {
        discard_pass(e);
        e->pass_status = MVS_OK;
        if (bad_rank == rank) g_err = local_err.empty() ? std::string("mvs_engine_exchange: this rank's pass failed") : local_err;
        else g_err = "mvs_engine_exchange: rank " + std::to_string(bad_rank) + " reported status " + std::to_string(bad_status) + " for this pass; all ranks give it up";
        return bad_status;
    }
    if (all[MVS_XCHG_WORDS * (size_t)rank] != e->n_new || all[MVS_XCHG_WORDS * (size_t)rank + 1] != e->n_kill) {
        g_err = "mvs_engine_exchange: count all-gather returned other values for this rank"; return MVS_ERR_STATE;
    }
    if (tot_new > headroom || tot_kill > kill_cap) {  // decided on the minimum over the ranks: all fail alike, whatever their own capacity
        discard_pass(e);
        g_err = "mvs_engine_exchange: patch pool capacity exceeded on at least one rank (raise mvs_config.max_patches)";
        return MVS_ERR_CAPACITY;
    }
    // (2) this rank's block goes straight to its final place behind the pool, (3) every block is broadcast in place.
    // Job ranges are contiguous and ascending in rank, so the concatenation in rank order is the global
    // (view, cell, creation) order of the 1-GPU commit.
    DPatch* tail = e->pool.p + e->pool_n;
    if (e->n_new > 0) mvsk_commit_copy(e->sa, e->job_base_scan.p, tail + off_new[rank], e->n_new, nullptr, 0, st);
    if (e->n_kill > 0) mvsk_kill_export(e->kill.p, e->pool_n, e->kill_base.p, e->comm_kill_ids.p + off_kill[rank], e->n_kill, st);
    const ncclResult_t bc = broadcast_blocks(e, [&](int r, auto&& send) {
        send(tail + off_new[r], all[MVS_XCHG_WORDS * (size_t)r] * (int64_t)sizeof(DPatch), ncclUint8);
        send(e->comm_kill_ids.p + off_kill[r], all[MVS_XCHG_WORDS * (size_t)r + 1], ncclInt32);
    });
    if (bc != ncclSuccess) { g_err = std::string("mvs_engine_exchange: record / kill-id broadcast: ") + R.GetErrorString(bc); return MVS_ERR_HIP; }
    HIPCHK(hipEventRecord(e->ev[5], st));
    {
        Range rc("mvs:commit");
        // the union of the ranks' kill ids and records (the same on every rank)
        if (int r = commit_pool(e, [&](int64_t* added) -> int {
                mvsk_apply_kill_ids(e->pool.p, e->comm_kill_ids.p, tot_kill, e->pool_n, st);
                if (e->pool_n > 0) HIPCHK(hipMemsetAsync(e->kill.p, 0, (size_t)e->pool_n, st));
                *added = tot_new;
                return MVS_OK;
            }))
            return r;
    }
    HIPCHK(hipGetLastError());
    float ms = 0.0f;
    (void)hipEventElapsedTime(&ms, e->ev[4], e->ev[5]); e->timing.exchange_ms = ms;
    e->timing.exchange_bytes = (tot_new - e->n_new) * (int64_t)sizeof(DPatch) + (tot_kill - e->n_kill) * 4 + 8 * MVS_XCHG_WORDS * (int64_t)(world - 1);
    return MVS_OK;
}

}  // extern "C"
