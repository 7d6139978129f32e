// graph_host.inc — the host code the graph indexes on a FLAT handle share (hnsw_host.inc: HNSW-*, diskann_host.inc: DISKANN-*).
// Included from lynse_hip.hip before both; device code in graph.h.  Here: the lock, the handle check and the clock of their entries,
// the guards of their builds, the list normaliser of their loaders, and the search: its scratch and the chunked driver around the
// one kernel launch that differs.  (The refusals speak of HNSW for either index: the wording of the first user, kept.)

// the exclusive lock of the graph entries: tickets outstanding are a refusal of this index, not a bad argument
static int graph_lock(lynse_hip_flat* h, std::unique_lock<std::shared_mutex>& lk) {
    lk = std::unique_lock<std::shared_mutex>(h->rw);
    if (h->inflight.load(std::memory_order_acquire) != 0) {
        lk.unlock();
        return set_error(LYNSE_ERR_UNSUPPORTED, "HNSW: searches are in flight on this handle: wait for the outstanding tickets first");
    }
    return LYNSE_OK;
}
static int graph_check_handle(const lynse_hip_flat* h) {
    if (h->dtype != LYNSE_DTYPE_F32) return set_error(LYNSE_ERR_UNSUPPORTED, "HNSW on an F16 shard is not supported");
    if (h->packed_only) return set_error(LYNSE_ERR_UNSUPPORTED, "HNSW is defined for float rows (ip / l2 / cosine)");
    if (h->row_stride != 1 || h->row_offset != 0) return set_error(LYNSE_ERR_UNSUPPORTED, "an HNSW index is not row-sharded");
    return LYNSE_OK;
}
static inline double graph_now_us() {
    return (double)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count() * 1e-3;
}

struct GraphEvFree { hipEvent_t &a, &b; ~GraphEvFree() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); } };

// One list of a loaded graph brought into the stored form: GRAPH_PAD entries dropped, a neighbour named twice kept once (its first
// place); a neighbour >= n is refused with `beyond`, one that `extra` refuses with extra's own error.  dst: `cap` slots of GRAPH_PAD.
template <class Extra>
static int graph_take_list(const uint32_t* src, uint32_t cap, uint64_t n, const char* beyond, uint32_t* dst, Extra&& extra) {
    uint32_t w = 0;
    for (uint32_t s = 0; s < cap; ++s) {
        const uint32_t v = src[s];
        if (v == GRAPH_PAD) continue;
        if (v >= n) return set_error(LYNSE_ERR_INVALID_ARGUMENT, beyond);
        LY_TRY(extra(v));
        if (std::find(dst, dst + w, v) == dst + w) dst[w++] = v;
    }
    return LYNSE_OK;
}
static int graph_take_list(const uint32_t* src, uint32_t cap, uint64_t n, const char* beyond, uint32_t* dst) {
    return graph_take_list(src, cap, n, beyond, dst, [](uint32_t) { return LYNSE_OK; });
}

// The scratch of an index's searches, and what they measured with profiling on
struct GraphSearchScratch {
    DevBuf<float> q, dists;
    DevBuf<uint64_t> rows;
    DevBuf<uint32_t> vis, counts, status;
    double searches = 0.0, search_us = 0.0, scored = 0.0;   // searches timed, their kernel microseconds (HIP events), distances scored
};

// one chunk of queries as its kernel sees it: device pointers, the visited bitmaps zeroed
struct GraphSearchChunk {
    uint32_t nqc;
    const float* Q;         // [nqc][D]
    uint32_t* vis;          // [nqc][vis_words]
    uint32_t vis_words;
    uint64_t* out_rows;     // [nqc][k]
    float* out_dists;
    uint32_t *out_counts, *out_scored;   // [nqc]
    uint32_t* status;
    size_t lds;
    hipStream_t st;
};

// The search of a graph over n rows once its entry has checked the arguments, the index, ef and the LDS.  Queries go in chunks that
// keep the visited bitmaps (n bits per query) and the results under 256 MiB each; launch(chunk) fills the kernel's arguments and
// launches one wave per query.  `outgrew`: the message of the kernel's status word.
template <class Launch>
static int graph_search(lynse_hip_flat* h, GraphSearchScratch& s, uint64_t n, size_t lds, const char* outgrew, const float* queries, uint64_t nq,
                        uint32_t k, uint64_t* out_rows, float* out_dists, uint32_t* out_counts, Launch&& launch) {
    const uint32_t D = h->dim;
    const uint32_t vis_words = (uint32_t)((n + 31) / 32);
    const uint64_t qc = std::max<uint64_t>(1, std::min<uint64_t>({nq, (256ull << 20) / ((uint64_t)vis_words * 4), (256ull << 20) / ((uint64_t)k * 12), 1ull << 20}));
    LY_TRY(s.q.reserve((size_t)qc * D));
    LY_TRY(s.vis.reserve((size_t)qc * vis_words));
    LY_TRY(s.rows.reserve((size_t)qc * k));
    LY_TRY(s.dists.reserve((size_t)qc * k));
    LY_TRY(s.counts.reserve((size_t)qc * 2));   // counts, then the distances scored
    LY_TRY(s.status.reserve(1));
    hipStream_t st = cur(h).stream;
    const bool timed = h->profiling.load();
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (timed) { LY_HIP(hipEventCreate(&e0)); LY_HIP(hipEventCreate(&e1)); }
    GraphEvFree evfree{e0, e1};
    std::vector<uint32_t> scored;
    LY_HIP(hipMemsetAsync(s.status.p, 0, 4, st));
    for (uint64_t q0 = 0; q0 < nq; q0 += qc) {
        const uint32_t nqc = (uint32_t)std::min<uint64_t>(qc, nq - q0);
        LY_HIP(hipMemcpyAsync(s.q.p, queries + q0 * D, (size_t)nqc * D * 4, hipMemcpyHostToDevice, st));
        LY_HIP(hipMemsetAsync(s.vis.p, 0, (size_t)nqc * vis_words * 4, st));
        const GraphSearchChunk c{nqc, s.q.p, s.vis.p, vis_words, s.rows.p, s.dists.p, s.counts.p, s.counts.p + qc, s.status.p, lds, st};
        if (timed) LY_HIP(hipEventRecord(e0, st));
        LY_TRY(launch(c));
        if (timed) LY_HIP(hipEventRecord(e1, st));
        LY_HIP(hipMemcpyAsync(out_rows + q0 * k, s.rows.p, (size_t)nqc * k * 8, hipMemcpyDeviceToHost, st));
        LY_HIP(hipMemcpyAsync(out_dists + q0 * k, s.dists.p, (size_t)nqc * k * 4, hipMemcpyDeviceToHost, st));
        LY_HIP(hipMemcpyAsync(out_counts + q0, s.counts.p, (size_t)nqc * 4, hipMemcpyDeviceToHost, st));
        if (timed) {
            scored.resize(nqc);
            LY_HIP(hipMemcpyAsync(scored.data(), s.counts.p + qc, (size_t)nqc * 4, hipMemcpyDeviceToHost, st));
        }
        LY_TRY(stream_wait(st));
        if (timed) {
            float ms = 0.0f;
            LY_HIP(hipEventElapsedTime(&ms, e0, e1));
            s.search_us += (double)ms * 1e3;
            for (uint32_t v : scored) s.scored += (double)v;
        }
    }
    uint32_t status = 0;
    LY_HIP(hipMemcpy(&status, s.status.p, 4, hipMemcpyDeviceToHost));
    if (status) return set_error(LYNSE_ERR_INTERNAL, outgrew);
    if (timed) s.searches += 1;
    return LYNSE_OK;
}
