// async_host.inc — searches IN FLIGHT: submit / wait.  Included by lynse_hip.hip (after comm_host.inc).
//
// The reference serves concurrent readers (`Arc<RwLock<Collection>>` with `inner.read()` on the search path,
// src/python/mod.rs:950, :1187; its RPC / HTTP handlers call search from many workers, src/rpc.rs:588-590): a batch does not
// wait for the previous one to be answered.  The blocking entry points pay one host round trip per batch (the candidate
// overflow flags come back before the results are final) and leave the GPU idle between the short dependent kernels of
// one batch.  lynse_hip_flat_search_submit_* enqueues a whole batch — query staging, coarse scan stages, selects, exact
// rescoring, and for a row-sharded collection the ncclAllGather of the result blocks and the device merge — on ONE of the
// handle's search contexts (stream + workspace) and returns a ticket; lynse_hip_flat_search_wait blocks until that batch
// is final.  The kernels of up to n_ctx batches overlap on the device and the host never sits between them.
//
// Exactness is unchanged: the plan submitted is the ordinary level-0 plan; the overflow flags of the batch are OR-ed
// into one status word that travels WITH the result block (through the all-gather for a sharded collection, so every
// rank sees the same word), and wait() re-runs an overflowed batch on the next plan levels — on every rank, in ticket
// order, so the collectives stay aligned — before it returns.
//
// Rules: a ticket is COUNTED in the handle (`inflight`, bumped under the reader lock), it does not keep the lock: any thread
// may wait for it, and one thread may hold several.  Writers — append / finalize / lazy builds and the filtered / large-k
// searches — return an error while tickets are outstanding (writer_lock).  Sharded submits are collectives: every rank
// submits (and waits for) the same sequence, and whether a batch is pipelined or answered by the blocking exchange is
// decided from values that are the same on every rank (nq, k, metric, query kind) — never from the size or the
// build state of the local shard, which differ between ranks.

struct lynse_hip_ticket {
    lynse_hip_flat* h = nullptr;
    lynse_hip_comm* c = nullptr;
    int slot = -1;            // leased search context; -1 = the search completed inside submit
    bool packed = false, i8c = false, sampled = false, profiled = false, sts = false;
    int failed_rc = LYNSE_OK;      // sharded: the local pipeline could not be enqueued — the exchange ran with an empty block + the failure bit
    std::string failed_msg;
    const void* d_q = nullptr;
    uint64_t nq = 0;
    uint32_t k = 0, kk = 0;
    int metric = 0;
    uint64_t* out_rows = nullptr;
    float* out_dists = nullptr;
    uint32_t* out_counts = nullptr;
    hipEvent_t ev_begin = nullptr, ev_end = nullptr, ev_done = nullptr;
    ScanProf sprof;   // events of the ticket taken from the context's pool, scan launches of a profiled search
};

namespace {

// a free search context WITHOUT blocking (a single thread that submits more than n_ctx batches would wait for itself)
int ctx_try_acquire(lynse_hip_flat* h, int* slot) {
    {
        std::lock_guard<std::mutex> lk(h->ctx_mu);
        int s = 0;
        while (s < h->n_ctx && ((h->ctx_busy >> s) & 1u)) ++s;
        if (s >= h->n_ctx) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "every search context of the handle is in flight: wait for a ticket first (LYNSE_HIP_CONTEXTS)");
        h->ctx_busy |= 1u << s;
        *slot = s;
    }
    if (!h->ctx[*slot].stream && hipStreamCreateWithFlags(&h->ctx[*slot].stream, hipStreamNonBlocking) != hipSuccess) {
        std::lock_guard<std::mutex> lk(h->ctx_mu);
        h->ctx_busy &= ~(1u << *slot);
        return set_error(LYNSE_ERR_DEVICE, "hipStreamCreate failed");
    }
    return LYNSE_OK;
}

void ctx_release(lynse_hip_flat* h, int slot) {
    {
        std::lock_guard<std::mutex> lk(h->ctx_mu);
        h->ctx_busy &= ~(1u << slot);
    }
    h->ctx_cv.notify_one();
}

struct SlotScope {  // the helpers address the workspace / stream of the calling thread's context (cur())
    int prev;
    explicit SlotScope(int s) : prev(tl_ctx_slot) { tl_ctx_slot = s; }
    ~SlotScope() { tl_ctx_slot = prev; }
};

// where the local pipeline of a ticket writes: the caller's arrays, or this rank's result block of the exchange
struct LocalDst { uint64_t* rows; float* dists; uint32_t* counts; uint32_t* status; };

LocalDst ticket_dst(const lynse_hip_ticket* t, uint64_t* so_out = nullptr, uint64_t* total_out = nullptr) {
    if (!t->c) return {t->out_rows, t->out_dists, t->out_counts, nullptr};
    uint64_t ro, dof, co, so, total;
    comm_block_layout(t->nq, t->k, &ro, &dof, &co, &so, &total);
    if (so_out) *so_out = so;
    if (total_out) *total_out = total;
    char* local = t->c->local[t->slot];
    return {reinterpret_cast<uint64_t*>(local + ro), reinterpret_cast<float*>(local + dof), reinterpret_cast<uint32_t*>(local + co),
            reinterpret_cast<uint32_t*>(local + so)};
}

// stage the queries of the ticket and enqueue one plan level of the local pipeline on the ticket's context
int ticket_enqueue_local(lynse_hip_ticket* t, int level, bool i8c, bool allow_sts = true) {
    lynse_hip_flat* h = t->h;
    Workspace& w = cur(h).ws;
    hipStream_t st = cur(h).stream;
    const LocalDst d = ticket_dst(t);
    if (d.status) LY_HIP(hipMemsetAsync(d.status, 0, 16, st));
    if (h->n == 0) {  // an empty shard of a sharded collection: an empty block (the exchange still runs on every rank)
        LY_HIP(hipMemsetAsync(d.counts, 0, t->nq * 4, st));
        for (uint64_t i = 0; i < t->nq; ++i) { w.h_hdr[i] = 0; w.h_hdr[w.qcap + i] = 0; }
        t->sampled = false;
        return LYNSE_OK;
    }
    if (t->packed) LY_HIP(hipMemcpyAsync(w.QW, t->d_q, (size_t)t->nq * h->words * 8, hipMemcpyDeviceToDevice, st));
    // float queries are read in place (the caller keeps them valid until wait); counts + per-query overflow flags go straight
    // into the pinned header of the context (a sharded ticket looks at the status word of the exchange first)
    ChunkReq rq;
    rq.nq = (uint32_t)t->nq; rq.k = t->kk; rq.out_k = t->k; rq.metric = t->metric; rq.level = level;
    rq.qsrc = t->packed ? nullptr : (const float*)t->d_q; rq.i8c = i8c; rq.allow_sts = allow_sts;
    rq.out.rows = d.rows; rq.out.dists = d.dists; rq.out.counts2 = d.counts; rq.out.any_ovf = d.status; rq.out.hdr_direct = true;
    ChunkResult res;
    LY_TRY(run_chunk(h, rq, st, &t->sprof, &res));
    t->sampled = res.sampled;
    if (level == 0 && allow_sts) t->sts = res.used_sts;
    return LYNSE_OK;
}

// exchange + merge of a sharded ticket: on the communicator's ONE exchange stream (RCCL sees a single stream, the exchanges
// of the tickets run in submit order on every rank), behind an event of the ticket's local pipeline
// (comm_locked: the caller holds c->mu — the submit paths take it FIRST, in front of the shard's reader / writer lock, like the blocking
// sharded entry points do: taking it under that lock was a lock-order inversion against them, found by the ThreadSanitizer run)
int ticket_enqueue_exchange(lynse_hip_ticket* t, bool comm_locked = false) {
    lynse_hip_comm* c = t->c;
    hipStream_t st = cur(t->h).stream;
    uint64_t ro, dof, co, so, total;
    comm_block_layout(t->nq, t->k, &ro, &dof, &co, &so, &total);
    c->h_status[t->slot] = 0;
    std::unique_lock<std::mutex> lk(c->mu, std::defer_lock);
    if (!comm_locked) lk.lock();
    if (!c->ev_local[t->slot]) LY_HIP(hipEventCreateWithFlags(&c->ev_local[t->slot], hipEventDisableTiming));
    LY_HIP(hipEventRecord(c->ev_local[t->slot], st));
    LY_HIP(hipStreamWaitEvent(c->xstream, c->ev_local[t->slot], 0));
    const char* blocks = c->local[t->slot];
    if (c->world > 1) {
        LY_NCCL(g_rccl.AllGather(c->local[t->slot], c->gathered[t->slot], total, ncclUint8, c->comm, c->xstream));
        blocks = c->gathered[t->slot];
    }
    return merge_topk_device_impl(blocks, total, ro, dof, co, (uint32_t)c->world, t->nq, t->k, t->metric, t->out_rows, t->out_dists,
                                  t->out_counts, c->xstream, so, c->h_status + t->slot);
}

// LYNSE_HIP_DEBUG_FAIL_SUBMIT=1 (tests): the preparation of a sharded submit, FLAT or IVF, fails locally; read per call
bool debug_fail_submit() { return env_on("LYNSE_HIP_DEBUG_FAIL_SUBMIT", false); }

int submit_impl(lynse_hip_flat* h, lynse_hip_comm* c, const void* d_queries, bool packed, uint64_t nq, uint32_t k, int metric,
                uint64_t* d_out_rows, float* d_out_dists, uint32_t* d_out_counts, lynse_hip_ticket** out) {
    if (!h || !out) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    *out = nullptr;
    LY_TRY(metric_check(metric));
    if (nq && (!d_queries || !d_out_counts || (k && (!d_out_rows || !d_out_dists)))) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    if (c && h->device != c->device) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "the shard and the communicator live on different devices");
    if (c && (uint64_t)c->world * k > 8192) return set_error(LYNSE_ERR_UNSUPPORTED, "world * k exceeds the merge kernel capacity (8192)");
    if (c) LY_TRY(comm_check_alive(c));
    LY_TRY(use_device(h));
    const bool binary = metric >= M_HAMMING;
    if (packed && !binary) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "packed queries need a binary metric");
    if (!packed && binary) return set_error(LYNSE_ERR_UNSUPPORTED, "searches in flight take packed queries for the binary metrics");
    // lock order: the communicator's mutex, then the shard's reader / writer lock (sharded_search takes them in this order)
    std::unique_lock<std::mutex> comm_lk;
    if (c) comm_lk = std::unique_lock<std::mutex>(c->mu);
    // (everything below reads the shard's state — row count, capacities, what is built — under the reader lock: `kk = min(k, h->n)` used
    // to be formed in front of it, next to a concurrent append: found by the ThreadSanitizer run, tests/test_tsan_host.py)
    std::shared_lock<std::shared_mutex> rlk(h->rw);
    if (!binary && h->packed_only) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "store holds packed rows; float metrics unavailable");
    std::unique_ptr<lynse_hip_ticket> t(new lynse_hip_ticket());
    t->h = h; t->c = c; t->packed = packed; t->d_q = d_queries; t->nq = nq; t->k = k; t->metric = metric;
    t->out_rows = d_out_rows; t->out_dists = d_out_dists; t->out_counts = d_out_counts;
    t->kk = (uint32_t)std::min<uint64_t>(k, h->n);

    // Can this batch be pipelined?  One pass of the staged pipeline over a shard whose derived data is up to date.
    // SHARDED (a collective): the answer may only depend on what is identical on every rank — the shape of the batch.
    // Everything local is handled INSIDE the pipelined path: an empty shard sends an empty block, a small shard takes the
    // staged pipeline instead of the fused few-query kernel, missing SQ8 codes mean the f16 coarse pass for this batch,
    // and statistics / shadow / packed words still to build are built here, before the first ticket exists (appends are
    // refused while tickets are outstanding, so they cannot go stale under one).
    const bool shape_ok = nq > 0 && nq <= QCHUNK && k > 0 && k <= h->cap / 4 && !(binary && h->words > 16u * BIN_MAX_CHUNKS) &&
                          !(binary && (size_t)QCHUNK * h->words * 8 + QCHUNK * 4 > 150 * 1024);
    auto basic_ready = [&]() {
        if (h->n == 0) return true;
        if (binary) return h->packed_only || (h->packed != nullptr && h->n_packed == h->n);
        if (h->n_stats != h->n) return false;
        // (the f16 shadow is a lazy copy: a batch that takes the certified int8 pass does not need it)
        const bool int8 = i8c_eligible(h, metric, false, nq) && i8c_codes_ready(h, metric, nq) && i8c_codes_finite(h, metric, nq);
        return int8 || shadow_ready(h);
    };
    // (the SQ8 codes of the certified int8 pass are built here too while no ticket exists; with tickets outstanding a
    // batch that would have used them runs on the f16 coarse pass — a local choice, the results are the same)
    auto sq8_wanted = [&]() { return !binary && h->n > 0 && i8c_eligible(h, metric, false, nq) && !i8c_codes_ready(h, metric, nq); };
    // The f16 shadow is a LAZY copy (round 4): a shard that has only answered int8 batches does not hold it.  A batch that needs it while
    // tickets are outstanding — <= 32 queries on a small shard, L2 / cosine below 256 dimensions, a rank whose codes are not finite or
    // whose int8 pass struck out: LOCAL conditions, different from rank to rank — used to fail here (writer_lock refuses while tickets
    // are outstanding), and a sharded peer that did enqueue its all-gather stalled until the wait timeout.  Build it the way wait() does:
    // under the handle's exclusive lock (blocking readers wait), on context 0's stream.  Appends are refused while tickets are
    // outstanding, so the only copy that can be missing or stale here is one that NO ticket in flight reads (they all took the int8 pass).
    // A SHARDED submit whose shape is pipelined is a collective from here on: the peers enqueue their all-gather for this ticket, so a
    // LOCAL failure of anything below (a lazy build that runs out of memory, the writer lock refused behind outstanding tickets, the
    // workspace, an event, the pipeline itself) must not end the call in front of the exchange — the peers would wait out the collective
    // timeout and poison their handles.  Such a failure is carried to the exchange as `pre_rc`: empty block, failure bit (ADVICE r5).
    int pre_rc = LYNSE_OK;
    std::string pre_msg;
    auto prepare = [&]() -> int {
    if (c && shape_ok) {   // tests: a simulated local failure of a sharded submit (LYNSE_HIP_DEBUG_FAIL_SUBMIT=1; read per call)
        if (debug_fail_submit()) return set_error(LYNSE_ERR_OUT_OF_MEMORY, "LYNSE_HIP_DEBUG_FAIL_SUBMIT: simulated local failure of a sharded submit");
    }
    if (shape_ok && !binary && h->n > 0 && h->n_stats == h->n && h->inflight.load() != 0 && !basic_ready()) {
        rlk.unlock();
        {
            std::unique_lock<std::shared_mutex> sx(h->rw);
            SlotScope scope(0);
            LY_TRY(ensure_shadow_locked(h));
        }
        rlk.lock();
    }
    if (c && shape_ok && (!basic_ready() || (sq8_wanted() && h->inflight.load() == 0))) {
        rlk.unlock();
        {
            LY_WRITER(h, xlk);
            SlotScope scope(0);
            if (binary) LY_TRY(ensure_packed_locked(h));
            else {
                LY_TRY(finalize_locked(h));
                if (i8c_eligible(h, metric, false, nq)) { LY_TRY(ensure_workspace(h, k)); LY_TRY(ensure_i8c_codes_locked(h, metric, nq)); }
                if (!(i8c_eligible(h, metric, false, nq) && i8c_codes_ready(h, metric, nq) && i8c_codes_finite(h, metric, nq))) LY_TRY(ensure_shadow_locked(h));
            }
        }
        rlk.lock();
        if (!basic_ready()) return set_error(LYNSE_ERR_INTERNAL, "derived data changed while the batch was being submitted");
    }
    return LYNSE_OK;
    };
    pre_rc = prepare();
    if (pre_rc != LYNSE_OK) {
        if (!(c && shape_ok)) return pre_rc;
        pre_msg = g_last_error;
        if (!rlk.owns_lock()) rlk.lock();
    }
    bool eligible;
    if (c) {
        eligible = shape_ok;
    } else {
        const bool ready = basic_ready() && (binary || !i8c_eligible(h, metric, false, nq) || i8c_codes_ready(h, metric, nq));
        eligible = ready && shape_ok && h->n > 0 && !(h->n > h->cap && t->kk > h->cap / 4) && !small_path_ok(h, nq, t->kk, metric, false);
    }
    if (!eligible) {
        // the blocking path answers it inside submit (it may need the writer lock: no tickets may be outstanding then)
        rlk.unlock();
        if (comm_lk.owns_lock()) comm_lk.unlock();   // (sharded_search takes the communicator's mutex itself)
        if (h->inflight.load() != 0)
            return set_error(LYNSE_ERR_INVALID_ARGUMENT, "this search cannot be pipelined (shape, or derived data to build): wait for the outstanding tickets first");
        if (c) LY_TRY(sharded_search(h, c, d_queries, packed, nq, k, metric, d_out_rows, d_out_dists, d_out_counts));
        else LY_TRY(search_impl(h, d_queries, packed, nq, k, metric, d_out_rows, d_out_dists, d_out_counts, true, nullptr));
        *out = t.release();
        return LYNSE_OK;
    }
    int slot = -1;
    int rc = ctx_try_acquire(h, &slot);
    if (rc != LYNSE_OK) return rc;
    t->slot = slot;
    auto body = [&]() -> int {
        SlotScope scope(slot);
        // what the EXCHANGE itself needs comes first and may end the call: without its result blocks or the completion event this rank
        // cannot take part at all
        if (c) {
            uint64_t ro, dof, co, so, total;
            comm_block_layout(nq, k, &ro, &dof, &co, &so, &total);
            LY_TRY(comm_reserve_blocks(c, slot, total));   // (c->mu is held: comm_lk)
        }
        hipStream_t st = cur(h).stream;
        LY_TRY(get_event(h, t->sprof.ev_used++, &t->ev_done));
        auto local_part = [&]() -> int {
            if (pre_rc != LYNSE_OK) { g_last_error = pre_msg; return pre_rc; }
            LY_TRY(ensure_workspace(h, k));
            t->profiled = profile_begin_search(h);
            if (t->profiled) {
                LY_TRY(get_event(h, t->sprof.ev_used++, &t->ev_begin));
                LY_TRY(get_event(h, t->sprof.ev_used++, &t->ev_end));
                LY_HIP(hipEventRecord(t->ev_begin, st));
            }
            t->i8c = !binary && h->n > 0 && i8c_eligible(h, metric, false, nq) && i8c_codes_ready(h, metric, nq) && i8c_codes_finite(h, metric, nq);
            return ticket_enqueue_local(t.get(), 0, t->i8c);
        };
        const int lrc = local_part();
        if (lrc != LYNSE_OK) {
            if (!c) return lrc;
            // a collective: the peers have enqueued (or will enqueue) their all-gather for this ticket.  This rank still takes part, with
            // an empty block and the failure bit in its status word; every rank's wait() then returns an error instead of a timeout
            t->failed_rc = lrc;
            t->failed_msg = g_last_error;
            t->profiled = false;
            const LocalDst d = ticket_dst(t.get());
            LY_HIP(hipMemsetAsync(d.counts, 0, nq * 4, st));
            LY_HIP(hipMemsetAsync(d.status, 2, 16, st));
        }
        if (t->profiled && t->ev_end) LY_HIP(hipEventRecord(t->ev_end, st));
        if (c) LY_TRY(ticket_enqueue_exchange(t.get(), true));
        LY_HIP(hipEventRecord(t->ev_done, c ? c->xstream : st));
        return LYNSE_OK;
    };
    rc = body();
    if (rc != LYNSE_OK) {
        (void)hipStreamSynchronize(h->ctx[slot].stream);
        ctx_release(h, slot);
        return rc;
    }
    h->inflight.fetch_add(1, std::memory_order_release);  // (still under the reader lock: a writer that gets the lock sees it)
    *out = t.release();
    return LYNSE_OK;
}

}  // namespace

extern "C" int lynse_hip_flat_search_submit_f32_device(lynse_hip_flat* h, lynse_hip_comm* c, const float* d_queries, uint64_t nq, uint32_t k,
                                                       int metric, uint64_t* d_out_rows, float* d_out_dists, uint32_t* d_out_counts,
                                                       lynse_hip_ticket** out) {
    return submit_impl(h, c, d_queries, false, nq, k, metric, d_out_rows, d_out_dists, d_out_counts, out);
}

extern "C" int lynse_hip_flat_search_submit_packed_u64_device(lynse_hip_flat* h, lynse_hip_comm* c, const uint64_t* d_query_words, uint64_t nq,
                                                              uint32_t k, int metric, uint64_t* d_out_rows, float* d_out_dists,
                                                              uint32_t* d_out_counts, lynse_hip_ticket** out) {
    return submit_impl(h, c, d_query_words, true, nq, k, metric, d_out_rows, d_out_dists, d_out_counts, out);
}

// Blocks until the batch of the ticket is final in the caller's device arrays, then frees the ticket (also on error).
extern "C" int lynse_hip_flat_search_wait(lynse_hip_ticket* tp) {
    if (!tp) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "ticket is NULL");
    std::unique_ptr<lynse_hip_ticket> t(tp);
    if (t->slot < 0) return LYNSE_OK;  // answered inside submit
    lynse_hip_flat* h = t->h;
    lynse_hip_comm* c = t->c;
    struct Release {
        lynse_hip_ticket* t;
        // timed out: the device may still be reading the store and writing into the context — the context stays leased AND the ticket
        // stays counted, so that the writer guard (append / finalize / lazy builds reallocate what those kernels touch) never opens
        // again on this handle: it is poisoned until it is destroyed
        bool keep_ctx = false;
        ~Release() {
            if (keep_ctx) return;
            ctx_release(t->h, t->slot);
            t->h->inflight.fetch_sub(1, std::memory_order_release);
        }
    } release{t.get()};
    LY_TRY(use_device(h));
    SlotScope scope(t->slot);
    tl_prof = t->profiled;
    Workspace& w = cur(h).ws;
    hipStream_t st = cur(h).stream;
    const bool binary = t->metric >= M_HAMMING;
    {
        const uint32_t to = c ? collective_timeout_ms() : g_wait_timeout_ms.load();   // a ticket that ends in a collective: never wait for a dead peer forever
        const int wrc = event_wait_bounded(t->ev_done, to);
        if (wrc != LYNSE_OK) { release.keep_ctx = wrc == LYNSE_ERR_TIMEOUT; return wrc; }
    }
    if (t->failed_rc != LYNSE_OK) return set_error(t->failed_rc, t->failed_msg);   // (this rank's part failed at submit; the exchange has run)
    if (c && status_failed(c->h_status[t->slot]))
        return set_error(LYNSE_ERR_DEVICE, "another rank of the sharded collection failed in this batch (its error is on that rank)");
    uint64_t fallback_queries = 0;
    auto local_overflows = [&]() -> uint32_t {  // (non-sharded: the pinned header of the context)
        uint32_t nov = 0;
        for (uint64_t i = 0; i < t->nq; ++i) nov += w.h_hdr[w.qcap + i] ? 1 : 0;
        return nov;
    };
    const bool any = c ? ((c->h_status[t->slot] & STATUS_REDO) != 0) : (local_overflows() != 0);
    if (any) {
        // Rare: a query overflowed its candidate buffers on the plan submitted.  The blocking path's ladder, on this
        // ticket's own context: (int8 coarse pass ->) f16 coarse pass -> contiguous plan -> exhaustive plan.  Sharded: every
        // rank saw the same OR-ed status word, so every rank is here for the same ticket; a rank whose own shard did
        // not overflow keeps its block, and all of them repeat the exchange.
        LY_HIP(hipStreamSynchronize(st));  // (the pinned header of the context holds the per-query flags)
        uint32_t nov = local_overflows();
        fallback_queries += nov;
        bool i8c = t->i8c;
        // the ladder below scans the f16 shadow (a lazy copy).  Tickets hold no lock, and writers refuse to run while tickets are
        // outstanding — so nobody appends; the copy is created under the handle's exclusive lock (blocking readers wait), on this
        // ticket's own stream, and in-flight int8 scans never read it
        if (!binary && !shadow_ready(h)) {
            std::unique_lock<std::shared_mutex> sx(h->rw);
            LY_TRY(ensure_shadow_locked(h));
        }
        if (t->sts) {   // the self-tightening scan overflowed: the staged plan of the same coarse pass first (no strike; on every rank — the
                        // status word all ranks saw is the same, and whether a ticket used the single-launch scan follows from its shape)
            LY_TRY(ticket_enqueue_local(t.get(), 0, i8c, false));
            LY_HIP(hipStreamSynchronize(st));
            nov = local_overflows();
            if (nov) fallback_queries += nov;
        }
        const bool sampled0 = t->sampled;   // (read AFTER the retry: the single-launch scan ran the stage {0, n} and left it false)
        for (int level = 0; level < 3 && nov; ++level) {
            if (level == 0) {
                if (!i8c) continue;                 // level 0 on the f16 coarse pass is what was submitted
                i8c = false;                        // same level again with the f16 coarse pass
                i8c_add_strike(h, t->metric);
            } else if (level == 1 && !sampled0) {
                continue;                           // level 1 would repeat the contiguous plan already run
            }
            LY_TRY(ticket_enqueue_local(t.get(), level, i8c, false));
            LY_HIP(hipStreamSynchronize(st));
            nov = local_overflows();
            if (nov && level < 2) fallback_queries += nov;
        }
        if (nov) return set_error(LYNSE_ERR_INTERNAL, "candidate overflow on the exhaustive plan");
        if (c) {   // the repeated exchange is a collective like the first: its wait is bounded the same way
            LY_TRY(ticket_enqueue_exchange(t.get()));
            LY_HIP(hipEventRecord(t->ev_done, c->xstream));
            const int wrc = event_wait_bounded(t->ev_done, collective_timeout_ms());
            if (wrc != LYNSE_OK) { release.keep_ctx = wrc == LYNSE_ERR_TIMEOUT; return wrc; }
            if (status_failed(c->h_status[t->slot])) return set_error(LYNSE_ERR_DEVICE, "another rank of the sharded collection failed while the batch was re-answered");
            if (c->h_status[t->slot] != 0) return set_error(LYNSE_ERR_INTERNAL, "a shard still reports an overflow after the retry");
        }
    }
    if (t->profiled && t->ev_begin)
        LY_TRY(prof_accumulate(h, cur(h), t->ev_begin, t->ev_end, t->sprof.scan_events, binary, fallback_queries));
    return LYNSE_OK;
}
