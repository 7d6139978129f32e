// text_host.inc — BM25 text search (InvertedTextIndex::search, src/engine.rs:927-1054): a handle of its own that holds the posting
// lists of ONE field selection in HBM.  Included at the end of lynse_hip.hip after sparse_host.inc; the kernels are in text.h, the cut
// and the order are the range search's (range_cut_and_order, range_host.inc).  include/lynse_hip.h TEXT SEARCH, DESIGN.md §20.

struct lynse_hip_text {
    std::shared_mutex rw;
    int device = 0;
    hipStream_t stream = nullptr;
    uint64_t n = 0, V = 0, nnz = 0, total_len = 0;
    std::vector<uint64_t> term_ptr;   // V + 1, host only: a query's slot table carries the posting ranges to the device
    uint32_t *d_post_row = nullptr, *d_post_tf = nullptr, *d_doc_len = nullptr;
    size_t post_row_cap = 0, post_tf_cap = 0, doc_len_cap = 0;
    // the scratch of a search (it runs under the exclusive lock)
    TextSlot* d_slots = nullptr;
    uint64_t *d_slot_ptr = nullptr, *d_mask = nullptr, *d_stats = nullptr;   // d_stats: live rows | their length sum | df of every slot
    float* d_avg = nullptr;
    uint32_t* d_cnt = nullptr;
    size_t slots_cap = 0, slot_ptr_cap = 0, mask_cap = 0, stats_cap = 0, avg_cap = 0, cnt_cap = 0;
    ScoreCut cut;
    PoolRerank rr;
    std::vector<TextSlot> slots;
    std::vector<uint64_t> slot_ptr, stats, df, keys, h_out;
    std::vector<uint32_t> cnt, cand, seen;
    std::vector<float> avg, w;
    bool profiling = false;
    lynse_hip_profile prof{};
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};   // the scan begins / the scan ends / the last launch of the chunk
};

static uint64_t text_sat_mul(uint64_t a, uint64_t b) { return a && b > ~0ull / a ? ~0ull : a * b; }

// Rules b, d and e for one query (no device): avg and n_docs from the live corpus, the candidate terms from the live df of every
// slot, w = count * idf with libm's logf.  A slot with df == 0 gets w = 0 and no flag; docs == 0 leaves avg = 1 and nothing else.
extern "C" int lynse_hip_text_weights(uint64_t docs, uint64_t total, const uint64_t* df, const uint32_t* count, uint32_t T, uint32_t k,
                                      float* out_avg, float* out_w, uint32_t* out_cand) {
    if (!out_avg || (T && (!df || !count || !out_w || !out_cand))) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    *out_avg = 1.0f;
    for (uint32_t t = 0; t < T; ++t) {
        out_w[t] = 0.0f;
        out_cand[t] = 0u;
    }
    if (docs == 0) return LYNSE_OK;
    const float n_docs = (float)docs;
    *out_avg = std::max((float)total / n_docs, 1.0f);
    uint64_t min_df = 0;
    for (uint32_t t = 0; t < T; ++t)
        if (df[t] && (min_df == 0 || df[t] < min_df)) min_df = df[t];
    if (min_df == 0) return LYNSE_OK;   // rule c: no term has a live posting
    const uint64_t cutoff = std::max(text_sat_mul(min_df, 4), text_sat_mul(k, 8));
    bool any = false;
    for (uint32_t t = 0; t < T; ++t) {
        if (!df[t]) continue;
        out_cand[t] = df[t] < docs && df[t] <= cutoff ? 1u : 0u;
        any = any || out_cand[t];
        const float d = (float)df[t];
        const float idf = logf(((n_docs - d) + 0.5f) / (d + 0.5f) + 1.0f);
        out_w[t] = (float)count[t] * idf;
    }
    for (uint32_t t = 0; !any && t < T; ++t) out_cand[t] = df[t] ? 1u : 0u;   // no selective term: every term seeds candidates
    return LYNSE_OK;
}

extern "C" int lynse_hip_text_create(int device, lynse_hip_text** out) {
    if (!out) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    int ndev = 0;
    LY_TRY(lynse_hip_device_count(&ndev));
    if (ndev <= 0) return set_error(LYNSE_ERR_DEVICE, "no HIP device available (this library has no CPU fallback)");
    if (device < 0 || device >= ndev) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "device ordinal out of range");
    LY_HIP(hipSetDevice(device));
    auto* h = new lynse_hip_text();
    h->device = device;
    const hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete h;
        return set_error(LYNSE_ERR_DEVICE, std::string("hipStreamCreate: ") + hipGetErrorString(e));
    }
    *out = h;
    return LYNSE_OK;
}

extern "C" int lynse_hip_text_destroy(lynse_hip_text* h) {
    if (!h) return LYNSE_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (void* p : {(void*)h->d_post_row, (void*)h->d_post_tf, (void*)h->d_doc_len, (void*)h->d_slots, (void*)h->d_slot_ptr, (void*)h->d_mask,
                    (void*)h->d_stats, (void*)h->d_avg, (void*)h->d_cnt})
        if (p) (void)hipFree(p);
    h->cut.release();
    h->rr.release();
    for (hipEvent_t e : h->ev)
        if (e) (void)hipEventDestroy(e);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return LYNSE_OK;
}

// Replaces the whole store.  Everything is checked before any device work.
extern "C" int lynse_hip_text_set(lynse_hip_text* h, const uint32_t* doc_len, uint64_t n, const uint64_t* term_ptr, uint64_t V,
                                  const uint32_t* post_row, const uint32_t* post_tf) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    if (n >= (1ull << 32)) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "text rows: a selection key carries a 32-bit row, n must be below 2^32");
    if (V >= (1ull << 32)) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "text terms: a term id is 32 bits, V must be below 2^32");
    uint64_t nnz = 0, total = 0;
    if (n == 0 || V == 0) {
        if (term_ptr && V && term_ptr[V] != 0) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "text postings: rows must be below n");
        n = V = 0;   // (no row or no term: nothing can ever match)
    } else {
        if (!doc_len || !term_ptr) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
        if (term_ptr[0] != 0) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "text postings: term_ptr must start at 0");
        for (uint64_t t = 0; t < V; ++t)
            if (term_ptr[t + 1] < term_ptr[t]) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "text postings: term_ptr must not decrease");
        nnz = term_ptr[V];
        if (nnz && (!post_row || !post_tf)) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
        std::vector<uint64_t> sum((size_t)n, 0);
        for (uint64_t t = 0; t < V; ++t)
            for (uint64_t p = term_ptr[t]; p < term_ptr[t + 1]; ++p) {
                if (post_row[p] >= n) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "text postings: rows must be below n");
                if (p > term_ptr[t] && post_row[p] <= post_row[p - 1])
                    return set_error(LYNSE_ERR_INVALID_ARGUMENT, "text postings: rows must be strictly ascending within a term");
                if (post_tf[p] == 0) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "text postings: a term frequency must be at least 1");
                sum[post_row[p]] += post_tf[p];
            }
        for (uint64_t r = 0; r < n; ++r) {
            if (doc_len[r] == 0) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "text rows: a document length must be at least 1");
            if (sum[r] != doc_len[r]) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "text rows: the term frequencies of a row must sum to its length");
            total += doc_len[r];
        }
    }
    std::unique_lock<std::shared_mutex> lk(h->rw);
    LY_HIP(hipSetDevice(h->device));
    h->n = h->V = h->nnz = h->total_len = 0;   // (a failed upload leaves an empty store, not a torn one)
    h->term_ptr.clear();
    if (n == 0) return LYNSE_OK;
    LY_TRY(ivf_grow(&h->d_doc_len, &h->doc_len_cap, (size_t)n));
    LY_TRY(ivf_grow(&h->d_post_row, &h->post_row_cap, (size_t)std::max<uint64_t>(1, nnz)));
    LY_TRY(ivf_grow(&h->d_post_tf, &h->post_tf_cap, (size_t)std::max<uint64_t>(1, nnz)));
    LY_TRY(h2d_done(h->d_doc_len, doc_len, (size_t)n * 4));
    if (nnz) {
        LY_TRY(h2d_done(h->d_post_row, post_row, (size_t)nnz * 4));
        LY_TRY(h2d_done(h->d_post_tf, post_tf, (size_t)nnz * 4));
    }
    h->term_ptr.assign(term_ptr, term_ptr + V + 1);
    h->n = n;
    h->V = V;
    h->nnz = nnz;
    h->total_len = total;
    return LYNSE_OK;
}

extern "C" int lynse_hip_text_len(lynse_hip_text* h, uint64_t* out_rows, uint64_t* out_terms, uint64_t* out_nnz) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    std::shared_lock<std::shared_mutex> lk(h->rw);
    if (out_rows) *out_rows = h->n;
    if (out_terms) *out_terms = h->V;
    if (out_nnz) *out_nnz = h->nnz;
    return LYNSE_OK;
}

extern "C" uint64_t lynse_hip_text_hbm_bytes(lynse_hip_text* h) {
    if (!h) return 0;
    std::shared_lock<std::shared_mutex> lk(h->rw);
    return ((uint64_t)h->doc_len_cap + h->post_row_cap + h->post_tf_cap) * 4;
}

extern "C" int lynse_hip_text_profile_enable(lynse_hip_text* h, int on) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    std::unique_lock<std::shared_mutex> lk(h->rw);
    h->profiling = on != 0;
    return LYNSE_OK;
}

extern "C" int lynse_hip_text_profile_get(lynse_hip_text* h, lynse_hip_profile* out, int reset) {
    if (!h || !out) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    std::unique_lock<std::shared_mutex> lk(h->rw);
    *out = h->prof;
    if (reset) h->prof = lynse_hip_profile{};
    return LYNSE_OK;
}

// InvertedTextIndex::search (:927-1054) for nq queries in CSR of (term id, count) in slot order: rules a-h of the header.
extern "C" int lynse_hip_text_search(lynse_hip_text* h, const uint64_t* q_ptr, const uint32_t* q_terms, const uint32_t* q_counts, uint64_t nq,
                                     uint32_t k, const uint64_t* bitset_words, uint64_t n_words, uint64_t* out_rows, float* out_scores,
                                     uint32_t* out_counts, uint64_t* out_passed) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    if (nq == 0) return LYNSE_OK;
    if (!out_counts) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    auto nothing = [&](uint64_t q0, uint64_t q1) {
        memset(out_counts + q0, 0, (q1 - q0) * 4);
        if (out_passed) memset(out_passed + q0, 0, (q1 - q0) * 8);
        for (uint64_t i = q0 * k; k && out_rows && out_scores && i < q1 * k; ++i) {
            out_rows[i] = ~0ull;
            out_scores[i] = -INFINITY;
        }
    };
    if (k == 0) return nothing(0, nq), LYNSE_OK;   // (:936-938)
    if (!out_rows || !out_scores || !q_ptr) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    if (nq >= (1ull << 32)) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "too many queries");
    if (q_ptr[0] != 0) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "text queries: q_ptr must start at 0");
    for (uint64_t q = 0; q < nq; ++q)
        if (q_ptr[q + 1] < q_ptr[q]) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "text queries: q_ptr must not decrease");
    if (q_ptr[nq] == 0) return nothing(0, nq), LYNSE_OK;
    if (!q_terms || !q_counts) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    std::unique_lock<std::shared_mutex> lk(h->rw);
    const uint64_t n = h->n, V = h->V;
    for (uint64_t q = 0; q < nq; ++q) {
        for (uint64_t e = q_ptr[q]; e < q_ptr[q + 1]; ++e) {
            if (q_terms[e] >= V) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "text queries: a term id must be below the number of terms");
            if (q_counts[e] == 0) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "text queries: a term count must be at least 1");
        }
        if (q_ptr[q + 1] - q_ptr[q] > TEXT_MAX_TERMS) continue;   // (refused below; a sorted copy of a short query finds its duplicates)
        h->seen.assign(q_terms + q_ptr[q], q_terms + q_ptr[q + 1]);
        std::sort(h->seen.begin(), h->seen.end());
        if (std::adjacent_find(h->seen.begin(), h->seen.end()) != h->seen.end())
            return set_error(LYNSE_ERR_INVALID_ARGUMENT, "text queries: a term id occurs twice in a query");
    }
    for (uint64_t q = 0; q < nq; ++q)
        if (q_ptr[q + 1] - q_ptr[q] > TEXT_MAX_TERMS)
            return set_error(LYNSE_ERR_UNSUPPORTED, "text search: a query of more than 256 distinct known terms is not supported");
    if (n == 0) return nothing(0, nq), LYNSE_OK;
    LY_HIP(hipSetDevice(h->device));
    const uint32_t N = (uint32_t)std::min<uint64_t>(k, n);
    const uint64_t qc = ScoreCut::chunk(nq, n, N);
    const bool sort_dev = N <= 16384;
    if (sort_dev) {
        LY_TRY(ensure_lds<k_pool_select<256>>(PoolRerank::LDS_MAX));
        LY_TRY(ensure_lds<k_pool_select<1024>>(PoolRerank::LDS_MAX));
    }
    hipStream_t st = h->stream;
    const bool masked = bitset_words != nullptr;
    const uint64_t mask_words = masked ? std::min<uint64_t>(n_words, (n + 63) / 64) : 0;
    uint64_t most_slots = 0;   // of a chunk
    for (uint64_t q0 = 0; q0 < nq; q0 += qc) most_slots = std::max(most_slots, q_ptr[std::min(nq, q0 + qc)] - q_ptr[q0]);
    if (masked) LY_TRY(ivf_grow(&h->d_mask, &h->mask_cap, (size_t)std::max<uint64_t>(1, mask_words)));
    if (masked) LY_TRY(ivf_grow(&h->d_stats, &h->stats_cap, (size_t)most_slots + 2));
    LY_TRY(ivf_grow(&h->d_slots, &h->slots_cap, (size_t)std::max<uint64_t>(1, most_slots)));
    LY_TRY(ivf_grow(&h->d_slot_ptr, &h->slot_ptr_cap, (size_t)qc + 1));
    LY_TRY(ivf_grow(&h->d_avg, &h->avg_cap, (size_t)qc));
    LY_TRY(ivf_grow(&h->d_cnt, &h->cnt_cap, (size_t)qc));
    LY_TRY(ivf_grow(&h->rr.d_keys, &h->rr.keys_cap, (size_t)qc * N));
    LY_TRY(ivf_grow(&h->rr.d_pcnt, &h->rr.pcnt_cap, (size_t)qc));
    if (sort_dev) LY_TRY(ivf_grow(&h->rr.d_out, &h->rr.out_cap, ((size_t)qc * N * 12 + (size_t)qc * 4 + 7) / 8));
    LY_TRY(h->cut.grow(qc, n));
    const bool timed = h->profiling;
    if (timed) {
        for (hipEvent_t& e : h->ev)
            if (!e) LY_HIP(hipEventCreate(&e));
        h->prof.searches += 1;
    }
    auto chunk_done = [&]() -> int {   // the chunk's last launch is enqueued: its times go to the profile
        if (!timed) return LYNSE_OK;
        LY_HIP(hipEventRecord(h->ev[2], st));
        LY_HIP(hipEventSynchronize(h->ev[2]));
        float scan_ms = 0.f, all_ms = 0.f;
        LY_HIP(hipEventElapsedTime(&scan_ms, h->ev[0], h->ev[1]));
        LY_HIP(hipEventElapsedTime(&all_ms, h->ev[0], h->ev[2]));
        h->prof.scan_us += (double)scan_ms * 1000.0;
        h->prof.total_us += (double)all_ms * 1000.0;
        return LYNSE_OK;
    };
    // Everything that queues work: a failure on any path inside drains the stream before the call returns (below), because a queued copy
    // of the caller's words or of the handle's tables must not outlive the call.
    auto run = [&]() -> int {
        // (the caller's words are queued only once nothing before the first launch can fail without being drained)
        if (mask_words) LY_HIP(hipMemcpyAsync(h->d_mask, bitset_words, (size_t)mask_words * 8, hipMemcpyHostToDevice, st));
        uint64_t docs = n, total = h->total_len;   // rule a without a mask: the totals kept from set
        bool have_corpus = !masked;                // under a mask: counted by the first chunk that reaches the device
        for (uint64_t q0 = 0; q0 < nq; q0 += qc) {
            const uint32_t nqc = (uint32_t)std::min<uint64_t>(qc, nq - q0);
            const uint64_t e0 = q_ptr[q0], ns = q_ptr[q0 + nqc] - e0;
            if (ns == 0) {
                nothing(q0, q0 + nqc);
                continue;
            }
            h->slots.resize((size_t)ns);
            h->df.resize((size_t)ns);
            h->slot_ptr.resize((size_t)nqc + 1);
            for (uint32_t i = 0; i <= nqc; ++i) h->slot_ptr[i] = q_ptr[q0 + i] - e0;
            for (uint64_t s = 0; s < ns; ++s) {
                const uint32_t t = q_terms[e0 + s];
                h->slots[s] = TextSlot{h->term_ptr[t], h->term_ptr[t + 1], 0.0f, 0u};
                h->df[s] = h->term_ptr[t + 1] - h->term_ptr[t];   // rule c without a mask
            }
            if (masked) {   // rules a and c under the mask: exact integer counts from the device
                const uint32_t row_blocks = have_corpus ? 0u : (uint32_t)std::min<uint64_t>((n + TEXT_NT - 1) / TEXT_NT, 1024);
                LY_HIP(hipMemcpyAsync(h->d_slots, h->slots.data(), (size_t)ns * sizeof(TextSlot), hipMemcpyHostToDevice, st));
                LY_HIP(hipMemsetAsync(h->d_stats, 0, ((size_t)ns + 2) * 8, st));
                TextStatsArgs sa{};
                sa.post_row = h->d_post_row;
                sa.doc_len = h->d_doc_len;
                sa.n = n;
                sa.slots = h->d_slots;
                sa.n_slots = ns;
                sa.row_blocks = row_blocks;
                sa.mask = h->d_mask;
                sa.mask_words = mask_words;
                sa.corpus = reinterpret_cast<unsigned long long*>(h->d_stats);
                sa.df = reinterpret_cast<unsigned long long*>(h->d_stats) + 2;
                hipLaunchKernelGGL(k_text_stats, dim3((uint32_t)(row_blocks + ns * TEXT_STATS_PARTS)), dim3(TEXT_NT), 0, st, sa);
                if (hipGetLastError() != hipSuccess) return set_error(LYNSE_ERR_DEVICE, "k_text_stats launch failed");
                h->stats.resize((size_t)ns + 2);
                LY_HIP(hipMemcpyAsync(h->stats.data(), h->d_stats, ((size_t)ns + 2) * 8, hipMemcpyDeviceToHost, st));
                LY_TRY(stream_wait(st));
                if (!have_corpus) {
                    docs = h->stats[0];
                    total = h->stats[1];
                    have_corpus = true;
                }
                std::copy(h->stats.begin() + 2, h->stats.end(), h->df.begin());
            }
            if (docs == 0) return nothing(q0, nq), LYNSE_OK;   // rule a: the mask leaves no row (the first chunk with a term finds out; the chunks before it were empty)
            h->avg.resize(nqc);
            uint64_t scan_bytes = 0;
            for (uint32_t i = 0; i < nqc; ++i) {
                const uint64_t s0 = h->slot_ptr[i];
                const uint32_t T = (uint32_t)(h->slot_ptr[i + 1] - s0);
                h->w.resize(T);
                h->cand.resize(T);
                LY_TRY(lynse_hip_text_weights(docs, total, h->df.data() + s0, q_counts + e0 + s0, T, k, &h->avg[i], h->w.data(), h->cand.data()));
                for (uint32_t t = 0; t < T; ++t) {
                    TextSlot& s = h->slots[s0 + t];
                    s.w = h->w[t];
                    s.cand = h->cand[t];
                    if (h->df[s0 + t] == 0) s.p0 = s.p1 = 0;   // rule c: ignored from here on
                    scan_bytes += (s.p1 - s.p0) * 12;
                }
            }
            LY_HIP(hipMemcpyAsync(h->d_slots, h->slots.data(), (size_t)ns * sizeof(TextSlot), hipMemcpyHostToDevice, st));
            LY_HIP(hipMemcpyAsync(h->d_slot_ptr, h->slot_ptr.data(), ((size_t)nqc + 1) * 8, hipMemcpyHostToDevice, st));
            LY_HIP(hipMemcpyAsync(h->d_avg, h->avg.data(), (size_t)nqc * 4, hipMemcpyHostToDevice, st));
            LY_HIP(hipMemsetAsync(h->d_cnt, 0, (size_t)nqc * 4, st));
            TextScanArgs a{};
            a.post_row = h->d_post_row;
            a.post_tf = h->d_post_tf;
            a.doc_len = h->d_doc_len;
            a.n = n;
            a.slots = h->d_slots;
            a.slot_ptr = h->d_slot_ptr;
            a.avg = h->d_avg;
            a.nq = nqc;
            a.mask = masked ? h->d_mask : nullptr;
            a.mask_words = mask_words;
            a.S = h->cut.d_S;
            a.count = h->d_cnt;
            const dim3 grid((uint32_t)((n + TEXT_ROWS - 1) / TEXT_ROWS), nqc);
            if (timed) LY_HIP(hipEventRecord(h->ev[0], st));
            hipLaunchKernelGGL(k_text_scan, grid, dim3(TEXT_NT), 0, st, a);
            if (hipGetLastError() != hipSuccess) return set_error(LYNSE_ERR_DEVICE, "k_text_scan launch failed");
            if (timed) {
                LY_HIP(hipEventRecord(h->ev[1], st));
                h->prof.scan_launches += 1;
                h->prof.scan_rows += n * nqc;
                h->prof.scan_bytes += scan_bytes;
            }
            LY_TRY(range_cut_and_order(h->cut, h->rr, h->d_cnt, h->cnt, h->keys, h->h_out, nqc, n, N, k, M_IP, st, out_rows + q0 * k, out_scores + q0 * k,
                                       out_counts + q0, out_passed ? out_passed + q0 : nullptr, chunk_done));
        }
        return LYNSE_OK;
    };
    const int rc = run();
    if (rc != LYNSE_OK) (void)hipStreamSynchronize(st);
    return rc;
}
