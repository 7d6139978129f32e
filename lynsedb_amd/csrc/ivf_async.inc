// ivf_async.inc — IVF searches IN FLIGHT: submit / wait.  Included by lynse_hip.hip (after async_host.inc).
//
// IVFIndex::search (ivf.rs:181-348) under the reference's concurrent readers (`inner.read()`, src/python/mod.rs:950, :1187): the
// blocking entry points (lynse_hip_ivf_search_f32*, lynse_hip_ivf_search_sharded_f32_device) synchronise with the host once per batch
// — twice when the centroid ranking goes through the centroid store's own search — and hold the index for the whole batch.
// lynse_hip_ivf_search_submit_f32_device ENQUEUES a batch on one of the slab store's search contexts 1.. (stream + workspace + its own
// set of grouping buffers, IvfScratch): query images, the centroid ranking (one plan level of the centroid store's pipeline on the
// same stream), device-side grouping, the window scans / selects, exact rescoring, k_final — and for a row-sharded index the
// ncclAllGather of the result blocks + the device merge on the communicator's exchange stream — and returns a ticket;
// lynse_hip_ivf_search_wait blocks until that batch is final.  The kernels of up to n_ctx - 1 batches overlap on the device.
//
// Exactness is unchanged: everything the blocking path checks on the host between its steps — a candidate overflow of the scan or of
// the centroid ranking, the all-lists-empty fallback of IVFIndex (ivf.rs:258-265) — is OR-ed into one status word that travels with
// the result block (through the all-gather of a sharded ticket: every rank sees the same word) and is left in pinned headers; wait()
// re-answers such a batch with the blocking ladder on the ticket's own context, on every rank, before the exchange is repeated.
//
// Rules: the index guard + the store's exclusive lock are held while a batch is ENQUEUED (microseconds of host work), not while it
// runs; tickets are counted (`inflight`) and insert / delete are refused meanwhile.  Blocking searches keep working next to tickets
// (context 0).  Sharded submits are collectives: every rank submits and waits for the same sequence.  A batch whose shape the
// device-side grouping cannot take (binary index, nprobe >= nlist, more than IVF_GROUP_MAX_PAIRS (query, list) pairs ...) is
// answered by the blocking path inside submit — the local part only for a sharded ticket: its exchange is enqueued like any other's.

struct lynse_hip_ivf_ticket {
    lynse_hip_ticket base;      // h = the slab store, c, slot, queries, outputs, events (ticket_dst / ticket_enqueue_exchange address these)
    lynse_hip_ivf* ih = nullptr;
    uint32_t nprobe = 1;
    bool enqueued = false;      // the local part is in flight (else: it was answered synchronously inside submit)
    bool routed_by_chunk = false;
};

namespace {

// the shapes the device-side grouping of ivf_search_chunk_staged takes (its `dev_group` conditions)
bool ivf_async_shape_ok(lynse_hip_ivf* h, uint32_t nq, uint32_t nprobe) {
    lynse_hip_flat* s = h->store;
    const Workspace& w = cur(s).ws;
    const int dg_env = ivf_device_grouping();
    const uint32_t np_eff = std::min<uint32_t>(nprobe, h->nlist);
    const uint32_t pass_lists = std::max<uint32_t>(1, w.cap / 16);
    const uint64_t win_bound = (uint64_t)nq * (h->worst_rows[np_eff] / (uint32_t)SCAN_BR + 2ull * np_eff) + 16;
    return dg_env && !h->binary && np_eff < h->nlist && np_eff <= pass_lists && (uint64_t)nq * np_eff <= IVF_GROUP_MAX_PAIRS &&
           h->nlist <= IVF_GROUP_MAX_LISTS && win_bound * 3 * sizeof(IvfTile) <= (512ull << 20);
}

// the blocking ladder of ivf_search_impl for ONE chunk with device queries / outputs, on the calling thread's context
int ivf_chunk_blocking(lynse_hip_ivf* h, const float* d_q, uint32_t nq, uint32_t kk, uint32_t k, uint32_t nprobe, const LocalDst& d) {
    bool ovf = false;
    LY_TRY(ivf_search_chunk(h, d_q, nq, kk, k, nprobe, d.rows, d.dists, d.counts, false, &ovf, nullptr, nullptr, true));
    if (ovf) {
        LY_TRY(ivf_search_chunk(h, d_q, nq, kk, k, nprobe, d.rows, d.dists, d.counts, true, &ovf, nullptr, nullptr, true));
        if (ovf) return set_error(LYNSE_ERR_INTERNAL, "candidate overflow on the exhaustive IVF plan");
    }
    return LYNSE_OK;
}

}  // namespace

extern "C" int lynse_hip_ivf_search_submit_f32_device(lynse_hip_ivf* h, lynse_hip_comm* c, const float* d_queries, uint64_t nq, uint32_t k,
                                                      uint32_t nprobe, uint64_t* d_out_rows, float* d_out_dists, uint32_t* d_out_counts,
                                                      lynse_hip_ivf_ticket** out) {
    if (!h || !out) return set_error(LYNSE_ERR_INDEX_NOT_BUILT, "IVF index is not built");
    *out = nullptr;
    if (nq == 0 || nq > QCHUNK) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "a search in flight takes 1..256 queries");
    if (!d_queries || !d_out_counts || (k && (!d_out_rows || !d_out_dists))) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    if (k == 0) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "k must be positive for a search in flight");
    if (c && (uint64_t)c->world * k > 8192) return set_error(LYNSE_ERR_UNSUPPORTED, "world * k exceeds the merge kernel capacity (8192)");
    if (c) LY_TRY(comm_check_alive(c));
    // lock order: the communicator's mutex, the index guard, the store's lock (lynse_hip_ivf_search_sharded_f32_device takes them so)
    std::unique_lock<std::mutex> comm_lk;
    if (c) comm_lk = std::unique_lock<std::mutex>(c->mu);
    const std::shared_ptr<std::mutex> guard = ivf_guard_of(h);
    std::lock_guard<std::mutex> glk(*guard);
    if (!h->store) return set_error(LYNSE_ERR_INDEX_NOT_BUILT, "IVF index is not built");
    if (h->binary) return set_error(LYNSE_ERR_UNSUPPORTED, "searches in flight are defined for float IVF indexes");
    if (h->sq8) return set_error(LYNSE_ERR_UNSUPPORTED, "searches in flight are not defined for IVF-*-SQ8 indexes (pool + rerank)");
    if (h->spann) return set_error(LYNSE_ERR_UNSUPPORTED, "searches in flight are not defined for SPANN indexes");
    lynse_hip_flat* s = h->store;
    if (c && s->device != c->device) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "the shard and the communicator live on different devices");
    std::unique_lock<std::shared_mutex> lk(s->rw);
    LY_TRY(use_device(s));
    if (nprobe == 0) nprobe = 1;   // ivf.rs:192-196
    const uint32_t kk = (uint32_t)std::min<uint64_t>(k, s->n);
    const int metric = h->metric;
    std::unique_ptr<lynse_hip_ivf_ticket> t(new lynse_hip_ivf_ticket());
    t->ih = h; t->nprobe = nprobe;
    t->base.h = s; t->base.c = c; t->base.d_q = d_queries; t->base.nq = nq; t->base.k = k; t->base.kk = kk; t->base.metric = metric;
    t->base.out_rows = d_out_rows; t->base.out_dists = d_out_dists; t->base.out_counts = d_out_counts;

    // derived data: built while no ticket is in flight (the first submit), only checked afterwards.  A SHARDED submit is a collective
    // from here on (the peers enqueue their all-gather for this ticket): a LOCAL failure below — a build out of memory, derived data
    // still to build, k beyond this rank's staged pipeline — is carried to the exchange as `pre_rc` (empty block + failure bit) instead
    // of ending the call in front of it (ADVICE r5)
    const bool idle = h->inflight == 0;
    auto prepare = [&]() -> int {
        if (c) {   // tests: a simulated local failure of a sharded submit (LYNSE_HIP_DEBUG_FAIL_SUBMIT=1; read per call)
            if (debug_fail_submit()) return set_error(LYNSE_ERR_OUT_OF_MEMORY, "LYNSE_HIP_DEBUG_FAIL_SUBMIT: simulated local failure of a sharded submit");
        }
        if (s->n > 0) {
            if (idle) {
                SlotScope scope(0);
                LY_TRY(finalize_locked(s));
                LY_TRY(ensure_shadow_locked(s));
                if (h->cstore) {
                    std::unique_lock<std::shared_mutex> clk(h->cstore->rw);
                    LY_TRY(finalize_locked(h->cstore));
                    LY_TRY(ensure_shadow_locked(h->cstore));
                }
            } else if (s->n_stats != s->n || !shadow_ready(s)) {
                return set_error(LYNSE_ERR_INVALID_ARGUMENT, "derived data of the index is still to build: wait for the outstanding tickets first");
            }
        }
        if (s->n > 0 && kk > s->cap / 4) return set_error(LYNSE_ERR_UNSUPPORTED, "k beyond the staged pipeline: use the blocking search");
        return LYNSE_OK;
    };
    const int pre_rc = prepare();
    const std::string pre_msg = pre_rc != LYNSE_OK ? g_last_error : std::string();
    if (pre_rc != LYNSE_OK && !c) return pre_rc;

    int slot = -1;
    {   // contexts 1..: context 0 stays with the blocking searches
        std::lock_guard<std::mutex> clk(s->ctx_mu);
        int x = 1;
        while (x < s->n_ctx && ((s->ctx_busy >> x) & 1u)) ++x;
        if (x >= s->n_ctx) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "every search context of the index is in flight: wait for a ticket first (LYNSE_HIP_CONTEXTS)");
        s->ctx_busy |= 1u << x;
        slot = x;
    }
    auto give_back = [&]() { ctx_release(s, slot); };
    if (!s->ctx[slot].stream && hipStreamCreateWithFlags(&s->ctx[slot].stream, hipStreamNonBlocking) != hipSuccess) {
        give_back();
        return set_error(LYNSE_ERR_DEVICE, "hipStreamCreate failed");
    }
    t->base.slot = slot;
    auto body = [&]() -> int {
        SlotScope scope(slot);
        tl_prof = false;
        hipStream_t st = cur(s).stream;
        if (c) {
            uint64_t ro, dof, co, so, total;
            comm_block_layout(nq, k, &ro, &dof, &co, &so, &total);
            LY_TRY(comm_reserve_blocks(c, slot, total));   // (c->mu is held: comm_lk)
        }
        LY_TRY(get_event(s, t->base.sprof.ev_used++, &t->base.ev_done));
        const LocalDst d = ticket_dst(&t->base);
        if (d.status) LY_HIP(hipMemsetAsync(d.status, 0, 16, st));
        auto local_part = [&]() -> int {
        if (pre_rc != LYNSE_OK) { g_last_error = pre_msg; return pre_rc; }
        LY_TRY(ensure_workspace(s, k));
        if (s->n == 0) {   // an empty shard of a sharded index: an empty block (the exchange still runs on every rank)
            LY_HIP(hipMemsetAsync(d.counts, 0, nq * 4, st));
        } else if (ivf_async_shape_ok(h, (uint32_t)nq, nprobe)) {
            if (h->cstore) {   // the centroid ranking runs on the centroid store's context of the same slot
                const uint32_t np_eff = std::min<uint32_t>(nprobe, h->nlist);
                LY_TRY(ensure_workspace(h->cstore, np_eff));
            }
            bool i8c = ivf_i8c_eligible(h, metric, (uint32_t)nq, false, false);
            if (i8c) {
                if (idle) LY_TRY(ensure_i8c_codes_locked(s, metric));
                i8c = i8c_codes_ready(s, metric, nq) && i8c_codes_finite(s, metric);
            }
            IvfAsync as{d.status, false};
            bool ovf_unused = false;
            LY_TRY(ivf_search_chunk_staged(h, d_queries, (uint32_t)nq, kk, k, nprobe, d.rows, d.dists, d.counts, false, &ovf_unused, nullptr, nullptr, true, i8c, false, &as));
            t->enqueued = true;
            t->base.i8c = i8c;
            t->routed_by_chunk = as.routed_by_chunk;
        } else {
            // a shape the device-side grouping does not take: the blocking ladder, here, on the ticket's context (results are final when
            // it returns); a sharded ticket still exchanges in flight
            LY_TRY(ivf_chunk_blocking(h, d_queries, (uint32_t)nq, kk, k, nprobe, d));
        }
        return LYNSE_OK;
        };
        const int lrc = local_part();
        if (lrc != LYNSE_OK) {
            if (!c) return lrc;
            // a collective: this rank still takes part in the exchange, with an empty block and the failure bit in its status word —
            // every rank's wait() returns an error instead of waiting out the timeout inside the all-gather
            t->base.failed_rc = lrc;
            t->base.failed_msg = g_last_error;
            LY_HIP(hipMemsetAsync(d.counts, 0, nq * 4, st));
            LY_HIP(hipMemsetAsync(d.status, 2, 16, st));
        }
        if (c) LY_TRY(ticket_enqueue_exchange(&t->base, true));
        LY_HIP(hipEventRecord(t->base.ev_done, c ? c->xstream : st));
        return LYNSE_OK;
    };
    const int rc = body();
    if (rc != LYNSE_OK) {
        (void)hipStreamSynchronize(s->ctx[slot].stream);
        give_back();
        return rc;
    }
    h->inflight += 1;
    (t->enqueued ? h->tk_async : h->tk_sync) += 1;
    *out = t.release();
    return LYNSE_OK;
}

// Blocks until the batch of the ticket is final in the caller's device arrays, then frees the ticket (also on error).
extern "C" int lynse_hip_ivf_search_wait(lynse_hip_ivf_ticket* tp) {
    if (!tp) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "ticket is NULL");
    std::unique_ptr<lynse_hip_ivf_ticket> t(tp);
    lynse_hip_ivf* h = t->ih;
    lynse_hip_flat* s = t->base.h;
    lynse_hip_comm* c = t->base.c;
    const int slot = t->base.slot;
    struct Release {
        lynse_hip_ivf* h; lynse_hip_flat* s; int slot;
        // timed out: the device may still be reading the slab store and writing into the context — the context stays leased and the
        // ticket stays counted: insert / delete (they swap and free the store) are refused on this index for good
        bool keep_ctx = false;
        ~Release() {
            if (keep_ctx) return;
            ctx_release(s, slot);
            const std::shared_ptr<std::mutex> guard = ivf_guard_of(h);
            std::lock_guard<std::mutex> glk(*guard);
            h->inflight -= 1;
        }
    } release{h, s, slot};
    LY_TRY(use_device(s));
    {
        const uint32_t to = c ? collective_timeout_ms() : g_wait_timeout_ms.load();
        const int wrc = event_wait_bounded(t->base.ev_done, to);
        if (wrc != LYNSE_OK) { release.keep_ctx = wrc == LYNSE_ERR_TIMEOUT; return wrc; }
    }
    const uint64_t nq = t->base.nq;
    auto local_flags = [&]() -> bool {   // what the blocking path looks at on the host between its steps
        if (!t->enqueued) return false;
        const Workspace& w = s->ctx[slot].ws;
        bool any = h->scr[slot].h_ghdr && h->scr[slot].h_ghdr[4] != 0;            // all probed lists of some query are empty (IVFIndex: scan every list)
        for (uint64_t i = 0; i < nq; ++i) any |= w.h_hdr[QCHUNK + i] != 0;       // candidate overflow of the list scans
        if (t->routed_by_chunk) {
            const Workspace& cw = h->cstore->ctx[slot].ws;
            for (uint64_t i = 0; i < nq; ++i) any |= cw.h_hdr[cw.qcap + i] != 0;  // ... of the centroid ranking
        }
        return any;
    };
    if (t->base.failed_rc != LYNSE_OK) return set_error(t->base.failed_rc, t->base.failed_msg);   // (this rank's part failed at submit; the exchange has run)
    if (c && status_failed(c->h_status[slot]))
        return set_error(LYNSE_ERR_DEVICE, "another rank of the sharded collection failed in this batch (its error is on that rank)");
    const bool any = c ? ((c->h_status[slot] & STATUS_REDO) != 0) : local_flags();   // (overflow, or the all-lists-empty flag of a query: answered again)
    if (!any) return LYNSE_OK;
    // Rare.  Sharded: every rank saw the same OR-ed status word, so every rank is here for the same ticket; a rank whose own part is
    // clean keeps its block, and all of them repeat the exchange.
    {
        std::unique_lock<std::mutex> comm_lk;   // (lock order: communicator, index guard, store)
        if (c) comm_lk = std::unique_lock<std::mutex>(c->mu);
        const std::shared_ptr<std::mutex> guard = ivf_guard_of(h);
        std::lock_guard<std::mutex> glk(*guard);
        std::unique_lock<std::shared_mutex> lk(s->rw);
        SlotScope scope(slot);
        tl_prof = false;
        hipStream_t st = cur(s).stream;
        LY_HIP(hipStreamSynchronize(st));   // (the pinned headers of the context)
        const LocalDst d = ticket_dst(&t->base);
        h->tk_redo += 1;
        if (local_flags()) LY_TRY(ivf_chunk_blocking(h, (const float*)t->base.d_q, (uint32_t)nq, t->base.kk, t->base.k, t->nprobe, d));
        if (c) {
            LY_HIP(hipMemsetAsync(d.status, 0, 16, st));
            LY_TRY(ticket_enqueue_exchange(&t->base, true));
            LY_HIP(hipEventRecord(t->base.ev_done, c->xstream));
            const int wrc = event_wait_bounded(t->base.ev_done, collective_timeout_ms());   // (a collective like the first exchange: bounded)
            if (wrc != LYNSE_OK) { release.keep_ctx = wrc == LYNSE_ERR_TIMEOUT; return wrc; }
            if (status_failed(c->h_status[slot])) return set_error(LYNSE_ERR_DEVICE, "another rank of the sharded collection failed while the batch was re-answered");
            if (c->h_status[slot] != 0) return set_error(LYNSE_ERR_INTERNAL, "a shard still reports an overflow after the retry");
        }
    }
    return LYNSE_OK;
}

// out[0..2]: tickets whose local part was enqueued without a host synchronisation / answered inside submit / re-answered inside wait
// (tests and monitoring: that a batch really ran in flight is not visible in its results)
extern "C" int lynse_hip_ivf_ticket_stats(lynse_hip_ivf* h, uint64_t* out) {
    if (!h || !out) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    const std::shared_ptr<std::mutex> guard = ivf_guard_of(h);
    std::lock_guard<std::mutex> glk(*guard);
    out[0] = h->tk_async; out[1] = h->tk_sync; out[2] = h->tk_redo;
    return LYNSE_OK;
}
