// comm_host.inc — the multi-GPU exchange behind the C-ABI (SURVEY §8e).  Included by lynse_hip.hip.
//
// Replaces the reference's TCP scatter / gather between a coordinator and its shard nodes — fan-out of the query batch
// (src/cluster.rs:101-123, :173-217), the 12 B / candidate result blocks every shard returns (src/rpc.rs:1156-1177) and the
// coordinator's merge (src/cluster.rs:327-393) — with ONE process per GPU, every rank scanning its row shard for the whole
// batch, ONE ncclAllGather over xGMI of the fixed-size per-rank result block [rows u64 | dists f32 | counts u32] and a
// device k-way merge in the canonical (distance in metric order, global row) order, all on the shard's own HIP stream.
//
// RCCL is bound at RUN time (dlopen): the library has no link-time dependency on it, single-GPU users never load it, and
// a host process that already carries an RCCL (PyTorch bundles one) hands its path in so that the process keeps ONE copy.
// The bootstrap (handing rank 0's unique id to the other ranks) is the launcher's business: torch.distributed, MPI, a
// file — 128 opaque bytes.

#include <dlfcn.h>
#include <rccl/rccl.h>  // types and prototypes only (decltype below); nothing of it is linked

namespace {

struct RcclApi {
    void* lib = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclAllGather) AllGather = nullptr;
    decltype(&ncclAllReduce) AllReduce = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    std::string path;
};

RcclApi g_rccl;
std::mutex g_rccl_mu;

int rccl_load_locked(const char* path) {
    if (g_rccl.lib) return LYNSE_OK;
    std::vector<std::string> candidates;
    if (path && *path) candidates.push_back(path);
    if (const char* e = env_str("LYNSE_HIP_RCCL_PATH")) candidates.push_back(e);
    for (const char* n : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) candidates.push_back(n);
    std::string tried;
    for (const std::string& c : candidates) {
        void* lib = dlopen(c.c_str(), RTLD_NOW | RTLD_LOCAL);
        if (!lib) { tried += (tried.empty() ? "" : ", ") + c; continue; }
        RcclApi a;
        a.lib = lib;
        a.GetUniqueId = reinterpret_cast<decltype(a.GetUniqueId)>(dlsym(lib, "ncclGetUniqueId"));
        a.CommInitRank = reinterpret_cast<decltype(a.CommInitRank)>(dlsym(lib, "ncclCommInitRank"));
        a.CommDestroy = reinterpret_cast<decltype(a.CommDestroy)>(dlsym(lib, "ncclCommDestroy"));
        a.AllGather = reinterpret_cast<decltype(a.AllGather)>(dlsym(lib, "ncclAllGather"));
        a.AllReduce = reinterpret_cast<decltype(a.AllReduce)>(dlsym(lib, "ncclAllReduce"));
        a.GetErrorString = reinterpret_cast<decltype(a.GetErrorString)>(dlsym(lib, "ncclGetErrorString"));
        if (!a.GetUniqueId || !a.CommInitRank || !a.CommDestroy || !a.AllGather || !a.AllReduce || !a.GetErrorString) {
            dlclose(lib);
            tried += (tried.empty() ? "" : ", ") + c + " (symbols missing)";
            continue;
        }
        a.path = c;
        g_rccl = a;
        return LYNSE_OK;
    }
    return set_error(LYNSE_ERR_DEVICE, "RCCL could not be loaded (tried: " + tried + ")");
}

}  // namespace

#define LY_NCCL(expr)                                                                                              \
    do {                                                                                                           \
        ncclResult_t _r = (expr);                                                                                  \
        if (_r != ncclSuccess)                                                                                     \
            return set_error(LYNSE_ERR_DEVICE, std::string(#expr) + ": " + (g_rccl.GetErrorString ? g_rccl.GetErrorString(_r) : "RCCL error")); \
    } while (0)

struct lynse_hip_comm {
    ncclComm_t comm = nullptr;
    int rank = 0, world = 1, device = 0;
    // result blocks of the batches in flight: this rank's (local) and everybody's (gathered), device memory — one pair per
    // search context of the shard (lynse_hip_flat_search_submit_*), the last pair for the synchronous entry points
    static constexpr int N_SLOTS = lynse_hip_flat::MAX_CTX + 1;
    char* local[N_SLOTS] = {};
    char* gathered[N_SLOTS] = {};
    size_t block_cap[N_SLOTS] = {};
    uint32_t* h_status = nullptr;  // pinned: one word per slot, written by k_merge (OR of the shards' status words)
    // searches in flight: every exchange (all-gather + merge) is enqueued on ONE stream of the communicator, in ticket order,
    // behind an event of the ticket's scan — RCCL sees a single stream however many search contexts feed it
    hipStream_t xstream = nullptr;
    hipEvent_t ev_local[N_SLOTS] = {};
    uint32_t* d_word = nullptr;  // self-check scratch
    hipEvent_t ev_sync = nullptr;  // bounded waits of the blocking entry points (stream_wait_bounded)
    // a BLOCKING collective of this communicator timed out (a rank is gone): its all-gather / merge may still be enqueued and may
    // still write the caller's output arrays and the slot's blocks — every later sharded call fails fast instead of queueing another
    // 30 s behind the hung collective, and the output buffers of the timed-out call must stay allocated until lynse_hip_comm_destroy
    std::atomic<bool> failed{false};
    std::mutex mu;
};

static int comm_check_alive(const lynse_hip_comm* c) {
    if (c->failed.load(std::memory_order_acquire))
        return set_error(LYNSE_ERR_DEVICE, "a collective of this communicator timed out earlier (a rank is gone): destroy the communicator; the output "
                                           "buffers of the call that timed out must stay allocated until then");
    return LYNSE_OK;
}

static void comm_block_layout(uint64_t nq, uint32_t k, uint64_t* rows_off, uint64_t* dists_off, uint64_t* counts_off, uint64_t* status_off,
                              uint64_t* total) {
    *rows_off = 0;                                   // the layout of sharded.block_layout / the 12 B-per-candidate block of rpc.rs:1156-1177
    *dists_off = *rows_off + nq * k * 8;
    *counts_off = *dists_off + nq * k * 4;
    *status_off = (*counts_off + nq * 4 + 15) / 16 * 16;  // one status word per shard (bit 0: a query overflowed; searches in flight)
    *total = *status_off + 16;
}

extern "C" int lynse_hip_comm_load_rccl(const char* path) {
    std::lock_guard<std::mutex> lk(g_rccl_mu);
    return rccl_load_locked(path);
}

extern "C" int lynse_hip_comm_unique_id(uint8_t* id128) {
    if (!id128) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    {
        std::lock_guard<std::mutex> lk(g_rccl_mu);
        LY_TRY(rccl_load_locked(nullptr));
    }
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 opaque bytes");
    ncclUniqueId id;
    LY_NCCL(g_rccl.GetUniqueId(&id));
    memcpy(id128, &id, sizeof id);
    return LYNSE_OK;
}

extern "C" int lynse_hip_comm_destroy(lynse_hip_comm* c) {
    if (!c) return LYNSE_OK;
    (void)hipSetDevice(c->device);
    if (c->comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(c->comm);
    for (int i = 0; i < lynse_hip_comm::N_SLOTS; ++i)
        for (void* p : {(void*)c->local[i], (void*)c->gathered[i]})
            if (p) (void)hipFree(p);
    if (c->d_word) (void)hipFree(c->d_word);
    if (c->h_status) (void)hipHostFree(c->h_status);
    for (int i = 0; i < lynse_hip_comm::N_SLOTS; ++i)
        if (c->ev_local[i]) (void)hipEventDestroy(c->ev_local[i]);
    if (c->ev_sync) (void)hipEventDestroy(c->ev_sync);
    if (c->xstream) (void)hipStreamDestroy(c->xstream);
    delete c;
    return LYNSE_OK;
}

extern "C" int lynse_hip_comm_create(const uint8_t* id128, int rank, int world, int device, lynse_hip_comm** out) {
    if (!id128 || !out) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    if (world < 1 || rank < 0 || rank >= world) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "rank / world out of range");
    {
        std::lock_guard<std::mutex> lk(g_rccl_mu);
        LY_TRY(rccl_load_locked(nullptr));
    }
    LY_HIP(hipSetDevice(device));
    lynse_hip_comm* c = new lynse_hip_comm();
    c->rank = rank; c->world = world; c->device = device;
    ncclUniqueId id;
    memcpy(&id, id128, sizeof id);
    ncclResult_t r = g_rccl.CommInitRank(&c->comm, world, id, rank);
    if (r != ncclSuccess) {
        const std::string msg = std::string("ncclCommInitRank: ") + g_rccl.GetErrorString(r);
        c->comm = nullptr;
        lynse_hip_comm_destroy(c);
        return set_error(LYNSE_ERR_DEVICE, msg);
    }
    if (hipMalloc(&c->d_word, 2 * sizeof(uint32_t)) != hipSuccess ||
        hipHostMalloc(&c->h_status, lynse_hip_comm::N_SLOTS * sizeof(uint32_t), hipHostMallocDefault) != hipSuccess ||
        hipStreamCreateWithFlags(&c->xstream, hipStreamNonBlocking) != hipSuccess) {
        lynse_hip_comm_destroy(c);
        return set_error(LYNSE_ERR_OUT_OF_MEMORY, "hipMalloc failed");
    }
    *out = c;
    return LYNSE_OK;
}

extern "C" int lynse_hip_comm_rank(const lynse_hip_comm* c) { return c ? c->rank : -1; }
extern "C" int lynse_hip_comm_world(const lynse_hip_comm* c) { return c ? c->world : 0; }

// Self-check of the communicator: an all-reduce(sum) of one word per rank must come back as `world` on every rank.
extern "C" int lynse_hip_comm_ranks_seen(lynse_hip_comm* c, int* out) {
    if (!c || !out) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    std::lock_guard<std::mutex> lk(c->mu);
    LY_HIP(hipSetDevice(c->device));
    const uint32_t one = 1;
    LY_TRY(h2d_done(c->d_word, &one, 4));
    LY_NCCL(g_rccl.AllReduce(c->d_word, c->d_word + 1, 1, ncclUint32, ncclSum, c->comm, c->xstream));
    LY_TRY(stream_wait_bounded(c->xstream, &c->ev_sync, c->world > 1 ? collective_timeout_ms() : 0u));
    uint32_t got = 0;
    LY_HIP(hipMemcpy(&got, c->d_word + 1, 4, hipMemcpyDeviceToHost));
    *out = (int)got;
    return LYNSE_OK;
}

static int comm_reserve_blocks(lynse_hip_comm* c, int slot, size_t block_bytes) {
    if (c->block_cap[slot] >= block_bytes) return LYNSE_OK;
    for (void* p : {(void*)c->local[slot], (void*)c->gathered[slot]})
        if (p) (void)hipFree(p);
    c->local[slot] = c->gathered[slot] = nullptr;
    c->block_cap[slot] = 0;
    LY_HIP(hipMalloc(&c->local[slot], block_bytes));
    LY_HIP(hipMalloc(&c->gathered[slot], block_bytes * (size_t)c->world));
    c->block_cap[slot] = block_bytes;
    return LYNSE_OK;
}

// The exchange half of the blocking sharded entry points: `lrc` is what the local search returned.  A rank that FAILED locally still
// takes part (empty block, failure bit in its status word): its peers return an error from the merged word instead of waiting
// out the timeout inside the all-gather.  The wait behind the collective is bounded.
static int sharded_exchange_blocking(lynse_hip_comm* c, int slot, hipStream_t st, int lrc, const std::string& lmsg, uint64_t nq, uint32_t k, int metric,
                                     uint64_t ro, uint64_t dof, uint64_t co, uint64_t so, uint64_t total,
                                     uint64_t* d_out_rows, float* d_out_dists, uint32_t* d_out_counts) {
    char* local = c->local[slot];
    if (c->world == 1) {  // nothing to exchange: the block is the answer
        if (lrc != LYNSE_OK) return set_error(lrc, lmsg);
        LY_HIP(hipMemcpyAsync(d_out_rows, local + ro, nq * k * 8, hipMemcpyDeviceToDevice, st));
        LY_HIP(hipMemcpyAsync(d_out_dists, local + dof, nq * k * 4, hipMemcpyDeviceToDevice, st));
        LY_HIP(hipMemcpyAsync(d_out_counts, local + co, nq * 4, hipMemcpyDeviceToDevice, st));
        LY_HIP(hipStreamSynchronize(st));
        return LYNSE_OK;
    }
    if (lrc != LYNSE_OK) {   // an empty block with the failure bit (every byte 2: bit 0, the overflow bit, stays clear)
        LY_HIP(hipMemsetAsync(local + co, 0, nq * 4, st));
        LY_HIP(hipMemsetAsync(local + so, 2, 16, st));
    }
    // exchange and merge, stream-ordered behind the scan: no host synchronisation in between
    c->h_status[slot] = 0;
    LY_NCCL(g_rccl.AllGather(local, c->gathered[slot], total, ncclUint8, c->comm, st));
    LY_TRY(merge_topk_device_impl(c->gathered[slot], total, ro, dof, co, (uint32_t)c->world, nq, k, metric, d_out_rows, d_out_dists, d_out_counts, st, so,
                                  c->h_status + slot));
    {
        const int wrc = stream_wait_bounded(st, &c->ev_sync, collective_timeout_ms());
        if (wrc == LYNSE_ERR_TIMEOUT) c->failed.store(true, std::memory_order_release);   // (the collective and the merge stay enqueued: see lynse_hip_comm::failed)
        if (wrc != LYNSE_OK) return wrc;
    }
    if (lrc != LYNSE_OK) return set_error(lrc, lmsg);
    if (status_failed(c->h_status[slot])) return set_error(LYNSE_ERR_DEVICE, "another rank of the sharded collection failed in this batch (its error is on that rank)");
    return LYNSE_OK;
}

// Whole-collection search of a row-sharded collection: scan of the local shard -> ncclAllGather of the per-rank result
// blocks -> device k-way merge, on the shard's stream; outputs (identical on every rank) are device memory.  A collective:
// every rank of the communicator must call it with the same nq / k / metric.  `packed` = queries are packed u64 words.
static int sharded_search(lynse_hip_flat* h, lynse_hip_comm* c, const void* d_queries, bool packed, uint64_t nq, uint32_t k, int metric,
                          uint64_t* d_out_rows, float* d_out_dists, uint32_t* d_out_counts) {
    if (metric_additive(metric)) return metric_check(metric);   // (before the handles: a refusal needs no communicator)
    if (!h || !c) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    LY_TRY(metric_check(metric));
    if (h->device != c->device) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "the shard and the communicator live on different devices");
    if (nq == 0) return LYNSE_OK;
    if (!d_queries || !d_out_counts || (k && (!d_out_rows || !d_out_dists))) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    LY_TRY(comm_check_alive(c));
    std::lock_guard<std::mutex> lk(c->mu);
    LY_HIP(hipSetDevice(c->device));
    hipStream_t st = h->ctx[0].stream;  // the exchange is stream-ordered behind the scan: one context, exclusive
    if (k == 0) {
        LY_HIP(hipMemsetAsync(d_out_counts, 0, nq * 4, st));
        LY_HIP(hipStreamSynchronize(st));
        return LYNSE_OK;
    }
    if ((uint64_t)c->world * k > 8192) return set_error(LYNSE_ERR_UNSUPPORTED, "world * k exceeds the merge kernel capacity (8192)");
    uint64_t ro, dof, co, so, total;
    comm_block_layout(nq, k, &ro, &dof, &co, &so, &total);
    constexpr int slot = lynse_hip_comm::N_SLOTS - 1;  // (the other pairs belong to the searches in flight)
    LY_TRY(comm_reserve_blocks(c, slot, total));
    char* local = c->local[slot];
    LY_HIP(hipMemsetAsync(local + so, 0, 16, st));  // status word: this path retries an overflow locally, before the exchange
    // 1. local shard (rows come back as GLOBAL rows: the handle's row map, lynse_hip_flat_set_row_map)
    const int lrc = search_impl(h, d_queries, packed, nq, k, metric, reinterpret_cast<uint64_t*>(local + ro), reinterpret_cast<float*>(local + dof),
                                reinterpret_cast<uint32_t*>(local + co), true, st);
    const std::string lmsg = lrc != LYNSE_OK ? g_last_error : std::string();
    // 2. + 3. the exchange (also behind a local failure: the peers must not wait for this rank)
    return sharded_exchange_blocking(c, slot, st, lrc, lmsg, nq, k, metric, ro, dof, co, so, total, d_out_rows, d_out_dists, d_out_counts);
}

extern "C" int lynse_hip_flat_search_sharded_f32_device(lynse_hip_flat* h, lynse_hip_comm* c, const float* d_queries, uint64_t nq, uint32_t k,
                                                        int metric, uint64_t* d_out_rows, float* d_out_dists, uint32_t* d_out_counts) {
    return sharded_search(h, c, d_queries, false, nq, k, metric, d_out_rows, d_out_dists, d_out_counts);
}

extern "C" int lynse_hip_flat_search_sharded_packed_u64_device(lynse_hip_flat* h, lynse_hip_comm* c, const uint64_t* d_query_words, uint64_t nq,
                                                               uint32_t k, int metric, uint64_t* d_out_rows, float* d_out_dists,
                                                               uint32_t* d_out_counts) {
    return sharded_search(h, c, d_query_words, true, nq, k, metric, d_out_rows, d_out_dists, d_out_counts);
}

// Row-sharded IVF (BASELINE config 4): every rank holds its rows of every list under the SAME centroids (sharded.ShardedIvf;
// lynse_hip_ivf_set_row_map makes the local search return GLOBAL rows, lynse_hip_ivf_set_routing(h, 2) switches the
// all-lists-empty fallback off: an empty local part of the probed lists is not "no candidates"), routes identically, scans
// its part of the probed lists, then the FLAT exchange: ONE ncclAllGather of the result blocks + the device k-way merge in
// the canonical (distance, global row) order, stream-ordered on the shard's stream.  Replaces the reference's scatter /
// gather of an index search over shard nodes (src/cluster.rs:101-123, :173-217, merge :327-393).  A collective: every rank
// calls it with the same nq / k / nprobe.  Outputs (identical on every rank) are device memory.
extern "C" int lynse_hip_ivf_search_sharded_f32_device(lynse_hip_ivf* h, lynse_hip_comm* c, const float* d_queries, uint64_t nq, uint32_t k,
                                                       uint32_t nprobe, uint64_t* d_out_rows, float* d_out_dists, uint32_t* d_out_counts) {
    if (!h || !c) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    if (nq == 0) return LYNSE_OK;
    if (!d_queries || !d_out_counts || (k && (!d_out_rows || !d_out_dists))) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    {
        IVF_GUARD(h);
        if (h->sq8) return set_error(LYNSE_ERR_UNSUPPORTED, "an IVF-*-SQ8 index is not row-sharded");
        if (h->spann) return set_error(LYNSE_ERR_UNSUPPORTED, "a SPANN index is not row-sharded");
    }
    LY_TRY(comm_check_alive(c));
    std::lock_guard<std::mutex> lk(c->mu);
    LY_HIP(hipSetDevice(c->device));
    hipStream_t st = nullptr;
    int index_metric = 0;
    {   // (insert / delete replace h->store: its fields are read under the index guard; a sharded index is not inserted into while it is
        // searched — the stream of context 0 outlives this block only because of that contract)
        IVF_GUARD(h);
        if (!h->store) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
        if (h->store->device != c->device) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "the shard and the communicator live on different devices");
        st = h->store->ctx[0].stream;
        index_metric = h->metric;
    }
    if (k == 0) {
        LY_HIP(hipMemsetAsync(d_out_counts, 0, nq * 4, st));
        LY_HIP(hipStreamSynchronize(st));
        return LYNSE_OK;
    }
    if ((uint64_t)c->world * k > 8192) return set_error(LYNSE_ERR_UNSUPPORTED, "world * k exceeds the merge kernel capacity (8192)");
    uint64_t ro, dof, co, so, total;
    comm_block_layout(nq, k, &ro, &dof, &co, &so, &total);
    constexpr int slot = lynse_hip_comm::N_SLOTS - 1;
    LY_TRY(comm_reserve_blocks(c, slot, total));
    char* local = c->local[slot];
    LY_HIP(hipMemsetAsync(local + so, 0, 16, st));  // status word: the local search retries its own overflows before the exchange
    // 1. the local part of the probed lists (an empty shard answers with zero counts)
    const int lrc = ivf_search_impl(h, d_queries, nq, k, nprobe, reinterpret_cast<uint64_t*>(local + ro), reinterpret_cast<float*>(local + dof),
                                    reinterpret_cast<uint32_t*>(local + co), false, nullptr, 0, -1, true);
    const std::string lmsg = lrc != LYNSE_OK ? g_last_error : std::string();
    // 2. + 3. exchange and merge behind the scan, one stream (also behind a local failure)
    return sharded_exchange_blocking(c, slot, st, lrc, lmsg, nq, k, index_metric, ro, dof, co, so, total, d_out_rows, d_out_dists, d_out_counts);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Row-sharded IVF TRAINING (BASELINE config 4: "collection sharded across 8 x MI355X"; SURVEY 8(e): all-reduce of nlist * D * 4 +
// nlist * 4 bytes per Lloyd iteration).  Every rank calls this with ITS rows (global row g = local row g / world on rank g % world)
// and gets the SAME centroids plus the assignments of its rows: k-means over the whole collection (kmeans.rs:74-139 — FastRng
// sample + farthest-first init over all rows, assignment with the single-row kernels, last-maximum / empty-cluster rules and the
// stop test on the global counts) with the centroid sums formed per rank (sequential over the rank's members, kmeans.rs:273-286 on
// the shard) and added over the ranks IN RANK ORDER, ((p0 + p1) + p2) + ... (lo_kmeans_train_sharded: defined bit for bit at any
// world size).  The reduction is either the library's RCCL communicator (`c`: per iteration one ncclAllGather of the per-rank sums +
// a rank-ordered add kernel + one integer ncclAllReduce, on device buffers) or a callback of the launcher (`reduce`: sums a HOST
// buffer over all ranks in place; dtype 0 = f32 in any order, 1 = u32, 2 = f32 in rank order; returns 0) — torch.distributed over
// gloo or RCCL, an MPI wrapper, or a test's in-process stand-in.  The reference's own cluster mode trains
// one index per shard node (python/lynse/cluster.py); this is what lets ONE set of centroids serve a collection that no single
// device ever holds.  A collective: every rank passes the same n_global / nlist / max_iter / metric.
extern "C" int lynse_hip_ivf_kmeans_sharded(const float* rows_local, uint64_t n_local, int rows_on_device, uint64_t n_global, uint32_t rank,
                                            uint32_t world, uint32_t dim, uint32_t nlist, uint32_t max_iter, int metric, int device,
                                            lynse_hip_comm* c, lynse_hip_reduce_fn reduce, void* reduce_ctx, float* out_centroids,
                                            uint32_t* out_assignments, uint32_t* out_k) {
    if (!out_centroids || !out_k || (n_local && (!rows_local || !out_assignments))) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    if (world == 0 || rank >= world || dim == 0 || nlist == 0) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "bad shard geometry");
    if (metric_additive(metric)) return metric_check(metric);
    if (metric < M_IP || metric > M_COS) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "sharded training takes ip / l2 / cosine");
    if (n_local != (n_global > rank ? (n_global - rank + world - 1) / world : 0)) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "n_local does not match rows g % world == rank of n_global");
    if (world > 1 && !c && !reduce) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "a communicator or a reduction callback is needed");
    if (c && (c->world != (int)world || c->rank != (int)rank)) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "the communicator has another geometry");
    if (c) LY_TRY(comm_check_alive(c));
    KmShard sh;
    sh.rank = rank; sh.world = world; sh.n_global = n_global;
    void* d_buf = nullptr;
    size_t d_cap = 0;
    hipEvent_t ev_sums = nullptr;
    struct Free { void*& p; hipEvent_t& e; ~Free() { if (p) (void)hipFree(p); if (e) (void)hipEventDestroy(e); } } free_buf{d_buf, ev_sums};
    auto reserve = [&](size_t bytes) -> bool {
        if (bytes <= d_cap) return true;
        if (d_buf) (void)hipFree(d_buf);
        d_buf = nullptr; d_cap = 0;
        if (hipMalloc(&d_buf, bytes) != hipSuccess) return false;
        d_cap = bytes;
        return true;
    };
    // the generic form (the init sample, once per training): a host buffer through device memory.  dtype 2 never comes here with a
    // communicator (reduce_iter below takes every Lloyd iteration).
    sh.reduce = [&](void* buf, uint64_t count, int dtype) -> int {
        if (world == 1) return 0;
        if (!c) return reduce(reduce_ctx, buf, count, dtype);
        if (dtype == 2) return 1;
        std::lock_guard<std::mutex> lk(c->mu);
        if (hipSetDevice(c->device) != hipSuccess) return 1;
        const size_t bytes = (size_t)count * 4;
        if (!reserve(bytes)) return 1;
        if (hipMemcpyAsync(d_buf, buf, bytes, hipMemcpyHostToDevice, c->xstream) != hipSuccess) return 1;
        if (g_rccl.AllReduce(d_buf, d_buf, count, dtype ? ncclUint32 : ncclFloat32, ncclSum, c->comm, c->xstream) != ncclSuccess) return 1;
        if (hipMemcpyAsync(buf, d_buf, bytes, hipMemcpyDeviceToHost, c->xstream) != hipSuccess) return 1;
        if (stream_wait_bounded(c->xstream, &c->ev_sync, collective_timeout_ms()) != LYNSE_OK) { c->failed.store(true, std::memory_order_release); return 2; }   // (2: the wait timed out — a rank is gone)
        return 0;
    };
    // A Lloyd iteration's reduction on DEVICE buffers, stream-ordered behind the sums kernel (no host bounce): ncclAllGather of the
    // per-rank sums (world x nlist x dim floats: 8 x 12.6 MB at BASELINE config 4) -> k_sum_rank_order, ((p0 + p1) + p2) + ... — the
    // order lo_kmeans_train_sharded specifies, whatever the world size — and ONE integer ncclAllReduce of the member counts + the
    // "changed" word; the reduced sums and words are read back once (the centroid update is host code, as without sharding).
    // LYNSE_HIP_KM_FORCE_COLLECTIVE=1 runs it at world 1 too (tests: the kernels and the one-rank collectives on real hardware).
    const bool force_collective = env_on("LYNSE_HIP_KM_FORCE_COLLECTIVE", false);   // (read per call: tests flip it)
    if (c && (world > 1 || force_collective)) {
        sh.reduce_iter = [&](float* d_sums, uint64_t count, const uint64_t* d_off, uint32_t k, uint32_t changed, hipStream_t st, float* h_sums,
                             uint32_t* h_counts) -> int {
            std::lock_guard<std::mutex> lk(c->mu);
            if (hipSetDevice(c->device) != hipSuccess) return 1;
            const size_t gather_b = ((size_t)world * count * 4 + 255) / 256 * 256, words_b = ((size_t)(k + 1) * 4 + 255) / 256 * 256;
            if (!reserve(gather_b + 2 * words_b)) return 1;
            float* d_gather = static_cast<float*>(d_buf);
            uint32_t* d_words = reinterpret_cast<uint32_t*>(static_cast<char*>(d_buf) + gather_b);
            uint32_t* d_words_sum = reinterpret_cast<uint32_t*>(static_cast<char*>(d_buf) + gather_b + words_b);
            if (!ev_sums && hipEventCreateWithFlags(&ev_sums, hipEventDisableTiming) != hipSuccess) return 1;
            if (hipEventRecord(ev_sums, st) != hipSuccess || hipStreamWaitEvent(c->xstream, ev_sums, 0) != hipSuccess) return 1;
            if (g_rccl.AllGather(d_sums, d_gather, count, ncclFloat32, c->comm, c->xstream) != ncclSuccess) return 1;
            hipLaunchKernelGGL(k_sum_rank_order, dim3((uint32_t)std::min<uint64_t>((count + 255) / 256, 4096)), dim3(256), 0, c->xstream,
                               d_gather, world, count, d_sums);
            hipLaunchKernelGGL(k_counts_from_offsets, dim3((k + 1 + 255) / 256), dim3(256), 0, c->xstream, d_off, k, changed, d_words);
            if (hipGetLastError() != hipSuccess) return 1;
            if (g_rccl.AllReduce(d_words, d_words_sum, (size_t)k + 1, ncclUint32, ncclSum, c->comm, c->xstream) != ncclSuccess) return 1;
            if (hipMemcpyAsync(h_sums, d_sums, (size_t)count * 4, hipMemcpyDeviceToHost, c->xstream) != hipSuccess) return 1;
            if (hipMemcpyAsync(h_counts, d_words_sum, ((size_t)k + 1) * 4, hipMemcpyDeviceToHost, c->xstream) != hipSuccess) return 1;
            if (stream_wait_bounded(c->xstream, &c->ev_sync, collective_timeout_ms()) != LYNSE_OK) { c->failed.store(true, std::memory_order_release); return 2; }
            return 0;
        };
    }
    std::vector<float> cen;
    std::vector<uint32_t> asg;
    uint32_t k = 0;
    LY_TRY(ivf_kmeans(rows_local, n_local, dim, nlist, max_iter, metric, device, &cen, &asg, &k, rows_on_device != 0, &sh));
    *out_k = k;
    memcpy(out_centroids, cen.data(), (size_t)k * dim * 4);
    if (n_local) memcpy(out_assignments, asg.data(), (size_t)n_local * 4);
    return LYNSE_OK;
}

// IVFIndex::build (ivf.rs:132-179) for a row shard of a collection that is spread over the ranks of a node, in one call: the
// all-reduced training above over the rank's device-resident rows, then the rank's slab store under the shared centroids with
// global row ids (row l of rank r = global row l * world + r) and the shard routing rule (no all-lists-empty fallback on a shard).
// What lynse_hip_ivf_search_sharded_f32_device and the IVF tickets search.  A collective.  `ivfflat_routing` != 0: IvfFlatMmap
// semantics (L2 cells whatever the search metric, ivf_flat_mmap.rs:56-159).
extern "C" int lynse_hip_ivf_build_sharded_device(const float* d_rows_local, uint64_t n_local, uint64_t n_global, uint32_t rank, uint32_t world,
                                                  uint32_t dim, uint32_t nlist, uint32_t max_iter, int metric, int ivfflat_routing, int device,
                                                  lynse_hip_comm* c, lynse_hip_reduce_fn reduce, void* reduce_ctx, lynse_hip_ivf** out) {
    if (!out) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    if (metric_additive(metric)) return metric_check(metric);
    if (ivfflat_routing && n_global < nlist) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "IVF requires at least as many vectors as partitions");   // ivf_flat_mmap.rs:69-75
    const uint32_t kmax = (uint32_t)std::min<uint64_t>(nlist, n_global);
    std::vector<float> cen((size_t)kmax * dim);
    std::vector<uint32_t> asg(std::max<uint64_t>(n_local, 1));
    uint32_t k = 0;
    LY_TRY(lynse_hip_ivf_kmeans_sharded(d_rows_local, n_local, 1, n_global, rank, world, dim, nlist, max_iter, ivfflat_routing ? (int)M_L2 : metric, device, c,
                                        reduce, reduce_ctx, cen.data(), asg.data(), &k));
    lynse_hip_ivf* h = nullptr;
    LY_TRY(lynse_hip_ivf_load_device(d_rows_local, n_local, dim, cen.data(), k, asg.data(), metric, device, &h));
    int rc = lynse_hip_ivf_set_row_map(h, world, rank);
    if (rc == LYNSE_OK && ivfflat_routing) rc = lynse_hip_ivf_set_routing(h, 1);
    if (rc == LYNSE_OK && world > 1) rc = lynse_hip_ivf_set_routing(h, 2);
    if (rc != LYNSE_OK) { lynse_hip_ivf_destroy(h); return rc; }
    *out = h;
    return LYNSE_OK;
}
