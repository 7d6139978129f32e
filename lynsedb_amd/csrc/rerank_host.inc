// rerank_host.inc — the exact rerank stage shared by the quantised indexes (IVF-*-SQ8 in ivf_host.inc, FLAT-*-PQ in
// pq_host.inc).  Included at the end of lynse_hip.hip, before both.  A cheap pool stage leaves a pool of candidate rows per query
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
    uint64_t* d_orow = nullptr; size_t orow_cap = 0;   // device selection into host outputs: the results before the copy
    float* d_odist = nullptr; size_t odist_cap = 0;
    uint32_t* d_ocnt = nullptr; size_t ocnt_cap = 0;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};   // profiling: the pool stage begins / the pool stage ends / the rerank ends
    void release() {
        for (void* p : {(void*)d_prow, (void*)d_pcnt, (void*)d_keys, (void*)d_orow, (void*)d_odist, (void*)d_ocnt})
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
        double pool_us = 0.0, rerank_us = 0.0;   // the stage times of this search (timed)
        std::vector<uint64_t> keys, h_rows;      // host selection
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
            if (!select_dev) LY_TRY(ivf_grow(&r.d_keys, &r.keys_cap, (size_t)qc * pool));
            if (select_dev && !dev_out) {
                LY_TRY(ivf_grow(&r.d_orow, &r.orow_cap, (size_t)qc * out_k));
                LY_TRY(ivf_grow(&r.d_odist, &r.odist_cap, (size_t)qc * out_k));
                LY_TRY(ivf_grow(&r.d_ocnt, &r.ocnt_cap, (size_t)qc));
            }
            a = PoolRerankArgs{V, n, ld, D, nullptr, r.d_prow, r.d_pcnt, pool, p2, metric, k_sel, out_k, nullptr, nullptr, nullptr, nullptr, nullptr};
            static std::once_flag lds_once;
            static int lds_rc = LYNSE_OK;
            std::call_once(lds_once, []() { lds_rc = set_max_lds(k_pool_rerank<true>, LDS_MAX); if (lds_rc == LYNSE_OK) lds_rc = set_max_lds(k_pool_rerank<false>, LDS_MAX); });
            LY_TRY(lds_rc);
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
                x.out_rows = dev_out ? out_rows : r.d_orow;
                x.out_dists = dev_out ? out_dists : r.d_odist;
                x.out_counts = dev_out ? out_counts : r.d_ocnt;
                hipLaunchKernelGGL(k_pool_rerank<true>, dim3(nqc), dim3(256), (size_t)a.p2 * 8 + q_lds, st, x);
                LY_HIP(hipGetLastError());
                LY_TRY(mark(2, st));
                if (!dev_out) {
                    LY_HIP(hipMemcpyAsync(out_rows, r.d_orow, (size_t)nqc * out_k * 8, hipMemcpyDeviceToHost, st));
                    LY_HIP(hipMemcpyAsync(out_dists, r.d_odist, (size_t)nqc * out_k * 4, hipMemcpyDeviceToHost, st));
                    LY_HIP(hipMemcpyAsync(out_counts, r.d_ocnt, (size_t)nqc * 4, hipMemcpyDeviceToHost, st));
                }
                LY_TRY(stream_wait(st));
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
