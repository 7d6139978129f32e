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

// the device buffers of a build, freed on every way out
struct GraphFree { std::vector<void**> ps; ~GraphFree() { for (void** p : ps) if (*p) (void)hipFree(*p); } };
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
    float *d_q = nullptr, *d_dists = nullptr;
    uint64_t* d_rows = nullptr;
    uint32_t *d_vis = nullptr, *d_counts = nullptr, *d_status = nullptr;
    size_t q_cap = 0, dists_cap = 0, rows_cap = 0, vis_cap = 0, counts_cap = 0;
    double searches = 0.0, search_us = 0.0, scored = 0.0;   // searches timed, their kernel microseconds (HIP events), distances scored

    ~GraphSearchScratch() {
        for (void* p : {(void*)d_q, (void*)d_dists, (void*)d_rows, (void*)d_vis, (void*)d_counts, (void*)d_status})
            if (p) (void)hipFree(p);
    }
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
    LY_TRY(ivf_grow(&s.d_q, &s.q_cap, (size_t)qc * D));
    LY_TRY(ivf_grow(&s.d_vis, &s.vis_cap, (size_t)qc * vis_words));
    LY_TRY(ivf_grow(&s.d_rows, &s.rows_cap, (size_t)qc * k));
    LY_TRY(ivf_grow(&s.d_dists, &s.dists_cap, (size_t)qc * k));
    LY_TRY(ivf_grow(&s.d_counts, &s.counts_cap, (size_t)qc * 2));   // counts, then the distances scored
    if (!s.d_status) LY_HIP(hipMalloc(&s.d_status, 4));
    hipStream_t st = cur(h).stream;
    const bool timed = h->profiling.load();
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (timed) { LY_HIP(hipEventCreate(&e0)); LY_HIP(hipEventCreate(&e1)); }
    GraphEvFree evfree{e0, e1};
    std::vector<uint32_t> scored;
    LY_HIP(hipMemsetAsync(s.d_status, 0, 4, st));
    for (uint64_t q0 = 0; q0 < nq; q0 += qc) {
        const uint32_t nqc = (uint32_t)std::min<uint64_t>(qc, nq - q0);
        LY_HIP(hipMemcpyAsync(s.d_q, queries + q0 * D, (size_t)nqc * D * 4, hipMemcpyHostToDevice, st));
        LY_HIP(hipMemsetAsync(s.d_vis, 0, (size_t)nqc * vis_words * 4, st));
        const GraphSearchChunk c{nqc, s.d_q, s.d_vis, vis_words, s.d_rows, s.d_dists, s.d_counts, s.d_counts + qc, s.d_status, lds, st};
        if (timed) LY_HIP(hipEventRecord(e0, st));
        LY_TRY(launch(c));
        if (timed) LY_HIP(hipEventRecord(e1, st));
        LY_HIP(hipMemcpyAsync(out_rows + q0 * k, s.d_rows, (size_t)nqc * k * 8, hipMemcpyDeviceToHost, st));
        LY_HIP(hipMemcpyAsync(out_dists + q0 * k, s.d_dists, (size_t)nqc * k * 4, hipMemcpyDeviceToHost, st));
        LY_HIP(hipMemcpyAsync(out_counts + q0, s.d_counts, (size_t)nqc * 4, hipMemcpyDeviceToHost, st));
        if (timed) {
            scored.resize(nqc);
            LY_HIP(hipMemcpyAsync(scored.data(), s.d_counts + qc, (size_t)nqc * 4, hipMemcpyDeviceToHost, st));
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
    LY_HIP(hipMemcpy(&status, s.d_status, 4, hipMemcpyDeviceToHost));
    if (status) return set_error(LYNSE_ERR_INTERNAL, outgrew);
    if (timed) s.searches += 1;
    return LYNSE_OK;
}
