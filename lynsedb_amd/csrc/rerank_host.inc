// rerank_host.inc — the exact rerank stage shared by the quantised indexes (IVF-*-SQ8 in ivf_host.inc; FLAT-*-PQ, FLAT-*-RABITQ and
// FLAT-*-POLARVEC<b> through their one search driver, coded_search in coded_host.inc) and, for the FLAT ones and the range, additive
// and approximate searches, the cut of a score matrix into the pool (ScoreCut below).  Included at the end of lynse_hip.hip, before
// them.  A cheap pool stage leaves a pool of candidate rows per query
// in d_prow / d_pcnt; k_pool_rerank (kernels.h) scores the pool exactly against the original rows and keeps the best k_sel by the
// canonical (distance, row) key.  A pool of up to 16,384 keys whose keys and query fit the LDS is selected on the device, a larger
// one is scored on the device and selected on the host.

template <typename T>
static int ivf_grow(T** p, size_t* cap, size_t need);   // (ivf_host.inc)

// The host selection of one query: the best min(k_sel, P) of its P keys by the canonical (score, row) key, padded to out_k with
// rows ~0 and the worst distance; rows map to row * row_stride + row_offset.  Reorders `keys`; returns the count.
static uint32_t select_pool_keys(uint64_t* keys, uint32_t P, uint32_t k_sel, uint32_t out_k, bool asc, uint64_t* rows, float* dists,
                                 uint64_t row_stride = 1, uint64_t row_offset = 0) {
    const uint32_t cnt = std::min<uint32_t>(k_sel, P);
    std::partial_sort(keys, keys + cnt, keys + P);   // ascending keys = (distance in metric order, row)
    for (uint32_t i = 0; i < out_k; ++i) {
        rows[i] = i < cnt ? (uint64_t)key_row(keys[i]) * row_stride + row_offset : ~0ull;
        dists[i] = i < cnt ? key_score(keys[i], asc) : (asc ? INFINITY : -INFINITY);
    }
    return cnt;
}

// The device buffers of the stage, grown on demand and kept by the owning index (its searches are serialised); no destructor, so
// the owner may be swapped whole: release() frees them.
struct PoolRerank {
    static constexpr size_t LDS_MAX = 160u * 1024u;
    uint64_t* d_prow = nullptr; size_t prow_cap = 0;   // written by the pool stage: [qc][pool] original rows ...
    uint32_t* d_pcnt = nullptr; size_t pcnt_cap = 0;   // ... and [qc] counts
    uint64_t* d_keys = nullptr; size_t keys_cap = 0;   // host selection: the scored keys
    uint64_t* d_out = nullptr; size_t out_cap = 0;     // device selection into host outputs: rows | dists | counts of a chunk, ONE copy back
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};   // profiling: the pool stage begins / the pool stage ends / the rerank ends
    void release() {
        for (void* p : {(void*)d_prow, (void*)d_pcnt, (void*)d_keys, (void*)d_out})
            if (p) (void)hipFree(p);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
        *this = PoolRerank();
    }

    // One search: begin() plans it, then each chunk of queries calls pool_start() before its pool stage and run() after it.
    struct Search {
        PoolRerank& r;
        PoolRerankArgs a{};
        size_t q_lds = 0;
        bool select_dev = false, dev_out = false, timed = false, asc = true;
        uint32_t split = 1;                      // workgroups that score one query's pool (set before begin(): split_small)
        bool split_small = false;                // a caller with few queries and pools of thousands of rows asks for split scoring
        double pool_us = 0.0, rerank_us = 0.0;   // the stage times of this search (timed)
        std::vector<uint64_t> keys, h_rows, h_out;   // host selection; the device selection's outputs on their way to the host
        std::vector<uint32_t> pcnt, h_cnt;
        std::vector<float> h_dists;
        explicit Search(PoolRerank& rr) : r(rr) {}

        // V: n original rows of `ld` floats (D used).  Pools of up to `pool` rows for chunks of up to qc queries; the best k_sel
        // of each pool go out at stride out_k, into device arrays when dev_out.  `who` prefixes the refusal of a query too wide
        // for the LDS.
        int begin(const float* V, uint64_t n, uint32_t ld, uint32_t D, int metric, uint32_t pool, uint32_t k_sel, uint32_t out_k,
                  uint64_t qc, bool dev_out_, bool timed_, const char* who) {
            uint32_t p2 = 2;
            while (p2 < pool) p2 <<= 1;
            q_lds = ((size_t)D + 3) / 4 * 16;
            if (q_lds > LDS_MAX) return set_error(LYNSE_ERR_UNSUPPORTED, std::string(who) + ": the query does not fit in LDS");
            select_dev = pool <= 16384 && (size_t)p2 * 8 + q_lds <= LDS_MAX;
            dev_out = dev_out_;
            timed = timed_;
            asc = metric_ascending(metric);
            LY_TRY(ivf_grow(&r.d_prow, &r.prow_cap, (size_t)qc * pool));
            LY_TRY(ivf_grow(&r.d_pcnt, &r.pcnt_cap, (size_t)qc));
            split = (split_small && select_dev && qc <= 16) ? std::max<uint32_t>(1, std::min<uint32_t>(64, (pool + 63) / 64)) : 1;
            if (!select_dev || split > 1) LY_TRY(ivf_grow(&r.d_keys, &r.keys_cap, (size_t)qc * pool));
            if (select_dev && !dev_out) LY_TRY(ivf_grow(&r.d_out, &r.out_cap, ((size_t)qc * out_k * 12 + (size_t)qc * 4 + 7) / 8));
            a = PoolRerankArgs{V, n, ld, D, nullptr, r.d_prow, r.d_pcnt, pool, p2, metric, k_sel, out_k, nullptr, nullptr, nullptr, nullptr, nullptr};
            LY_TRY(ensure_lds<k_pool_rerank<true>>(LDS_MAX));
            LY_TRY(ensure_lds<k_pool_rerank<false>>(LDS_MAX));
            LY_TRY(ensure_lds<k_pool_select<256>>(LDS_MAX));
            LY_TRY(ensure_lds<k_pool_select<1024>>(LDS_MAX));
            if (timed)
                for (hipEvent_t& e : r.ev)
                    if (!e) LY_HIP(hipEventCreate(&e));
            return LYNSE_OK;
        }

        int mark(int i, hipStream_t st) {
            if (timed) LY_HIP(hipEventRecord(r.ev[i], st));
            return LYNSE_OK;
        }
        int pool_start(hipStream_t st) { return mark(0, st); }

        // The rerank of nqc queries (q: their original queries on the device) on the pool stage's stream; the outputs start at the
        // chunk's first query.  pool_total: the profile's rescored-entry counter, or NULL.  Returns with the results in place.
        int run(const float* q, uint32_t nqc, uint64_t* out_rows, float* out_dists, uint32_t* out_counts, unsigned long long* pool_total,
                hipStream_t st) {
            LY_TRY(mark(1, st));
            PoolRerankArgs x = a;
            x.q = q;
            x.pool_total = pool_total;
            const uint32_t pool = a.pool_ld, out_k = a.out_k;
            if (select_dev) {
                // host outputs: the chunk's rows, distances and counts lie back to back in d_out and come back in one copy (three
                // small copies into pageable memory cost a single query more than its scan)
                const size_t o_dist = (size_t)nqc * out_k * 8, o_cnt = (size_t)nqc * out_k * 12, o_all = o_cnt + (size_t)nqc * 4;
                uint8_t* ob = reinterpret_cast<uint8_t*>(r.d_out);
                x.out_rows = dev_out ? out_rows : r.d_out;
                x.out_dists = dev_out ? out_dists : reinterpret_cast<float*>(ob + o_dist);
                x.out_counts = dev_out ? out_counts : reinterpret_cast<uint32_t*>(ob + o_cnt);
                if (split > 1) {   // scored by `split` workgroups per query, then sorted by one
                    x.keys_out = r.d_keys;
                    hipLaunchKernelGGL(k_pool_rerank<false>, dim3(nqc, split), dim3(256), q_lds, st, x);
                    LY_HIP(hipGetLastError());
                    if (a.p2 >= 2048) hipLaunchKernelGGL(k_pool_select<1024>, dim3(nqc), dim3(1024), (size_t)a.p2 * 8, st, x);
                    else hipLaunchKernelGGL(k_pool_select<256>, dim3(nqc), dim3(256), (size_t)a.p2 * 8, st, x);
                } else {
                    hipLaunchKernelGGL(k_pool_rerank<true>, dim3(nqc), dim3(256), (size_t)a.p2 * 8 + q_lds, st, x);
                }
                LY_HIP(hipGetLastError());
                LY_TRY(mark(2, st));
                if (!dev_out) {
                    h_out.resize((o_all + 7) / 8);
                    LY_HIP(hipMemcpyAsync(h_out.data(), r.d_out, o_all, hipMemcpyDeviceToHost, st));
                }
                LY_TRY(stream_wait(st));
                if (!dev_out) {
                    const uint8_t* hb = reinterpret_cast<const uint8_t*>(h_out.data());
                    memcpy(out_rows, hb, o_dist);
                    memcpy(out_dists, hb + o_dist, o_cnt - o_dist);
                    memcpy(out_counts, hb + o_cnt, o_all - o_cnt);
                }
            } else {   // every pool entry scored on the device, the canonical best k_sel selected on the host
                x.keys_out = r.d_keys;
                hipLaunchKernelGGL(k_pool_rerank<false>, dim3(nqc), dim3(256), q_lds, st, x);
                LY_HIP(hipGetLastError());
                LY_TRY(mark(2, st));
                keys.resize((size_t)nqc * pool);
                pcnt.resize(nqc);
                LY_HIP(hipMemcpyAsync(keys.data(), r.d_keys, keys.size() * 8, hipMemcpyDeviceToHost, st));
                LY_HIP(hipMemcpyAsync(pcnt.data(), r.d_pcnt, (size_t)nqc * 4, hipMemcpyDeviceToHost, st));
                LY_TRY(stream_wait(st));
                uint64_t* rows = out_rows;
                float* dists = out_dists;
                uint32_t* counts = out_counts;
                if (dev_out) {   // selected into host staging, then copied to the device outputs
                    h_rows.resize((size_t)nqc * out_k);
                    h_dists.resize((size_t)nqc * out_k);
                    h_cnt.resize(nqc);
                    rows = h_rows.data();
                    dists = h_dists.data();
                    counts = h_cnt.data();
                }
                const auto t_sel = std::chrono::steady_clock::now();
                for (uint32_t i = 0; i < nqc; ++i)
                    counts[i] = select_pool_keys(keys.data() + (size_t)i * pool, std::min<uint32_t>(pcnt[i], pool), a.k, out_k, asc,
                                                 rows + (size_t)i * out_k, dists + (size_t)i * out_k);
                if (timed) rerank_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_sel).count();
                if (dev_out) {
                    LY_TRY(h2d_done(out_rows, h_rows.data(), h_rows.size() * 8));
                    LY_TRY(h2d_done(out_dists, h_dists.data(), h_dists.size() * 4));
                    LY_TRY(h2d_done(out_counts, h_cnt.data(), h_cnt.size() * 4));
                }
            }
            if (timed) {   // (the stream has drained behind the rerank in both branches)
                float a_ms = 0.f, b_ms = 0.f;
                LY_HIP(hipEventElapsedTime(&a_ms, r.ev[0], r.ev[1]));
                LY_HIP(hipEventElapsedTime(&b_ms, r.ev[1], r.ev[2]));
                pool_us += (double)a_ms * 1000.0;
                rerank_us += (double)b_ms * 1000.0;
            }
            return LYNSE_OK;
        }
    };
};

// The pool stage's second half for the whole-corpus scans (FLAT-*-PQ, FLAT-*-RABITQ): a scan kernel writes the score_ord image of
// every (query, row) to S[nqc][n]; run() leaves the N best rows of each query by the canonical (score, row) key in the rerank's
// pool — the radix selection k_pq_hist / k_pq_find / k_pq_emit (pq.h), or every row when N == n.  Score production stays with the
// caller, so another producer of S (a prefilter) slots in before run().
struct ScoreCut {
    uint32_t *d_S = nullptr, *d_hist = nullptr;
    size_t S_cap = 0, hist_cap = 0;
    PqSel* d_sel = nullptr;
    size_t sel_cap = 0;
    std::vector<PqSel> sel0;
    void release() {
        for (void* p : {(void*)d_S, (void*)d_hist, (void*)d_sel})
            if (p) (void)hipFree(p);
        d_S = d_hist = nullptr;
        d_sel = nullptr;
        S_cap = hist_cap = sel_cap = 0;
    }
    // queries per chunk: the score matrix stays at or under 512 MiB and the pool at or under 256 MiB
    static uint64_t chunk(uint64_t nq, uint64_t n, uint32_t N) {
        return std::max<uint64_t>(1, std::min<uint64_t>({nq, (uint64_t)QCHUNK, (512ull << 20) / (n * 4), (256ull << 20) / ((uint64_t)N * 8)}));
    }
    int grow(uint64_t qc, uint64_t n) {
        LY_TRY(ivf_grow(&d_S, &S_cap, (size_t)qc * n));
        LY_TRY(ivf_grow(&d_sel, &sel_cap, (size_t)qc));
        if (hist_cap < (size_t)qc * PQ_BINS) {
            LY_TRY(ivf_grow(&d_hist, &hist_cap, (size_t)qc * PQ_BINS));
            LY_TRY(memset_done(d_hist, 0, hist_cap * 4));   // k_pq_find clears what it read: zero between searches
        }
        return LYNSE_OK;
    }
    // The selection from the states in sel0 (one per query; a state that starts `done` keeps its prefix: every key whose first
    // bits are <= it is taken), then the emission of the taken keys of each query to out[q * N ..] — the rows, or KEYS: the whole
    // keys — with their number in d_cnt[q].  `select`: some state is not done yet.
    template <bool KEYS>
    int cut(uint32_t nqc, uint64_t n, uint32_t N, bool select, uint64_t* out, uint32_t* d_cnt, hipStream_t st) {
        LY_HIP(hipMemcpyAsync(d_sel, sel0.data(), (size_t)nqc * sizeof(PqSel), hipMemcpyHostToDevice, st));
        const uint32_t rpb = 8192;
        const dim3 hgrid((uint32_t)((n + rpb - 1) / rpb), nqc);
        for (uint32_t pass = 0; select && pass < 6; ++pass) {
            hipLaunchKernelGGL(k_pq_hist, hgrid, dim3(256), 0, st, d_S, n, d_sel, d_hist, rpb);
            LY_HIP(hipGetLastError());
            hipLaunchKernelGGL(k_pq_find, dim3(nqc), dim3(256), 0, st, d_sel, d_hist);
            LY_HIP(hipGetLastError());
        }
        LY_HIP(hipMemsetAsync(d_cnt, 0, (size_t)nqc * 4, st));
        const uint32_t eblocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + PQ_EMIT_TILE - 1) / PQ_EMIT_TILE, 1024));
        hipLaunchKernelGGL(k_pq_emit<KEYS>, dim3(eblocks, nqc), dim3(256), 0, st, d_S, n, d_sel, N, out, d_cnt);
        LY_HIP(hipGetLastError());
        return LYNSE_OK;
    }
    int run(uint32_t nqc, uint64_t n, uint32_t N, PoolRerank& rr, uint32_t num_cu, hipStream_t st) {
        if (N < n) {
            sel0.assign(nqc, PqSel{0ull, 64u, N, 0u, 0u});
            LY_TRY(cut<false>(nqc, n, N, true, rr.d_prow, rr.d_pcnt, st));
        } else {
            const uint32_t blocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(((uint64_t)nqc * n + 255) / 256, (uint64_t)num_cu * 32));
            hipLaunchKernelGGL(k_pq_pool_all, dim3(blocks), dim3(256), 0, st, n, nqc, N, rr.d_prow, rr.d_pcnt);
            LY_HIP(hipGetLastError());
        }
        return LYNSE_OK;
    }
};
