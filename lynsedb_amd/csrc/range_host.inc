// range_host.inc — range search on a FLAT handle (Collection::search_range, src/engine.rs:6410-6483).  Included at the end of
// lynse_hip.hip after rabitq_host.inc; kernels in range.h, the cut at max_results is ScoreCut::cut and the order k_pool_select or
// select_pool_keys (rerank_host.inc).  DESIGN.md §16.

// The per-handle scratch of the search (it runs under the exclusive lock).  rr lends its buffers: d_keys takes the emitted keys,
// d_pcnt their number, d_out the sorted rows | distances | counts of a chunk.
struct RangeState {
    float *d_q = nullptr, *d_thr = nullptr;
    uint64_t *d_qw = nullptr, *d_mask = nullptr;
    uint32_t* d_cnt = nullptr;
    size_t q_cap = 0, thr_cap = 0, qw_cap = 0, mask_cap = 0, cnt_cap = 0;
    ScoreCut cut;
    PoolRerank rr;
    std::vector<uint32_t> cnt;
    std::vector<uint64_t> qw, keys, h_out;
    ~RangeState() {
        for (void* p : {(void*)d_q, (void*)d_thr, (void*)d_qw, (void*)d_mask, (void*)d_cnt})
            if (p) (void)hipFree(p);
        cut.release();
        rr.release();
    }
};

static void range_release(lynse_hip_flat* h) {
    delete h->range;
    h->range = nullptr;
}

// What follows a scan that left the score images in cut.d_S and the passer counts in d_cnt (the range search here, the sparse search
// in sparse_host.inc): the counts read back into out_passed / out_counts, the best min(passed, N) keys of each of the nqc queries by the
// canonical (score, row) key written best first at stride out_k and padded with rows ~0 and the worst score.  A query with more
// passers than N goes through the radix selection of its N best keys; any other takes every key below RANGE_FAIL (a state that starts
// done: the first 32 bits <= RANGE_FAIL - 1); a chunk in which nothing passed launches nothing more.  Sorted in LDS (k_pool_select)
// up to 16,384 keys, on the host beyond.  The outputs start at the chunk's first query; `launched` runs once the chunk's last launch
// is enqueued (profiling).
template <typename F>
static int range_cut_and_order(ScoreCut& cut, PoolRerank& rr, const uint32_t* d_cnt, std::vector<uint32_t>& cnt, std::vector<uint64_t>& keys,
                               std::vector<uint64_t>& h_out, uint32_t nqc, uint64_t n, uint32_t N, uint32_t out_k, int metric, hipStream_t st,
                               uint64_t* out_rows, float* out_dists, uint32_t* out_counts, uint64_t* out_passed, F&& launched) {
    const bool asc = metric_ascending(metric), sort_dev = N <= 16384;
    const float worst = asc ? INFINITY : -INFINITY;
    auto pad = [&](uint32_t q, uint32_t from) {
        for (uint32_t i = from; i < out_k; ++i) {
            out_rows[(size_t)q * out_k + i] = ~0ull;
            out_dists[(size_t)q * out_k + i] = worst;
        }
    };
    cnt.resize(nqc);
    LY_HIP(hipMemcpyAsync(cnt.data(), d_cnt, (size_t)nqc * 4, hipMemcpyDeviceToHost, st));
    LY_TRY(stream_wait(st));
    uint32_t most = 0;
    bool select = false;
    cut.sel0.resize(nqc);
    for (uint32_t i = 0; i < nqc; ++i) {
        const uint32_t c = cnt[i];
        if (out_passed) out_passed[i] = c;
        out_counts[i] = std::min(c, N);
        most = std::max(most, std::min(c, N));
        select = select || c > N;
        cut.sel0[i] = c > N ? PqSel{0ull, 64u, N, 0u, 0u} : PqSel{(uint64_t)(RANGE_FAIL - 1u), 32u, 0u, 1u, 0u};
    }
    if (most == 0) {
        for (uint32_t i = 0; i < nqc; ++i) pad(i, 0);
        return launched();
    }
    LY_TRY(cut.cut<true>(nqc, n, N, select, rr.d_keys, rr.d_pcnt, st));
    if (sort_dev) {   // sorted in LDS (k_pool_select), rows | distances | counts of the chunk back in one copy
        uint32_t p2 = 2;
        while (p2 < most) p2 <<= 1;
        const uint32_t ok = most;   // output stride of the chunk on the device: no query emitted more
        const size_t o_dist = (size_t)nqc * ok * 8, o_cnt = (size_t)nqc * ok * 12, o_all = o_cnt + (size_t)nqc * 4;
        uint8_t* ob = reinterpret_cast<uint8_t*>(rr.d_out);
        PoolRerankArgs x{};
        x.pool_cnt = rr.d_pcnt;
        x.pool_ld = N;
        x.p2 = p2;
        x.metric = metric;
        x.k = ok;
        x.out_k = ok;
        x.out_rows = rr.d_out;
        x.out_dists = reinterpret_cast<float*>(ob + o_dist);
        x.out_counts = reinterpret_cast<uint32_t*>(ob + o_cnt);
        x.keys_out = rr.d_keys;
        if (p2 >= 2048) hipLaunchKernelGGL(k_pool_select<1024>, dim3(nqc), dim3(1024), (size_t)p2 * 8, st, x);
        else hipLaunchKernelGGL(k_pool_select<256>, dim3(nqc), dim3(256), (size_t)p2 * 8, st, x);
        LY_HIP(hipGetLastError());
        LY_TRY(launched());
        h_out.resize((o_all + 7) / 8);
        LY_HIP(hipMemcpyAsync(h_out.data(), rr.d_out, o_all, hipMemcpyDeviceToHost, st));
        LY_TRY(stream_wait(st));
        const uint8_t* hb = reinterpret_cast<const uint8_t*>(h_out.data());
        for (uint32_t i = 0; i < nqc; ++i) {   // (k_pool_select padded a shorter result up to `ok`)
            memcpy(out_rows + (size_t)i * out_k, hb + (size_t)i * ok * 8, (size_t)ok * 8);
            memcpy(out_dists + (size_t)i * out_k, hb + o_dist + (size_t)i * ok * 4, (size_t)ok * 4);
            pad(i, ok);
        }
    } else {   // beyond the 16,384 keys of the LDS sort: sorted on the host, as select_pool_keys does for large pools
        LY_TRY(launched());
        keys.resize((size_t)nqc * N);
        LY_HIP(hipMemcpyAsync(keys.data(), rr.d_keys, keys.size() * 8, hipMemcpyDeviceToHost, st));
        LY_TRY(stream_wait(st));
        for (uint32_t i = 0; i < nqc; ++i)
            select_pool_keys(keys.data() + (size_t)i * N, out_counts[i], N, out_k, asc, out_rows + (size_t)i * out_k, out_dists + (size_t)i * out_k);
    }
    return LYNSE_OK;
}

// The LDS tiles of k_range_scan for rows of D floats and chunks of up to qc queries: up to 24 KiB of queries, then rows up to 78 KiB
// in all (two workgroups per CU: one stages its tile while the other scores); a row too wide for that takes the whole LDS.
static int range_plan(uint32_t D, uint64_t qc, uint32_t* TQ, uint32_t* R, uint32_t* stride, size_t* lds) {
    const uint32_t st = (D + 7u) / 8u * 8u + 8u;   // the eight lane groups of a wave on different bank octets (rescore_keys)
    const size_t row_b = (size_t)st * 4, q_b = (size_t)D * 4;
    auto bytes = [&](uint32_t tq, uint32_t r) { return ((size_t)tq * D + 3) / 4 * 16 + (size_t)r * row_b + (size_t)tq * 8; };
    uint32_t tq = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>({(uint64_t)RANGE_MAX_Q, qc, (24u * 1024u) / q_b}));
    size_t budget = 78u * 1024u;
    if (bytes(tq, 8) > budget) budget = PoolRerank::LDS_MAX;
    if (bytes(tq, 1) > budget) tq = 1;
    if (bytes(tq, 1) > budget) return set_error(LYNSE_ERR_UNSUPPORTED, "range search: a query and a row do not fit in LDS");
    const uint32_t r = (uint32_t)std::min<size_t>(RANGE_MAX_ROWS, (budget - bytes(tq, 0)) / row_b);
    *TQ = tq;
    *R = r;
    *stride = st;
    *lds = bytes(tq, r);
    return LYNSE_OK;
}

// pack_binary_query: bit i of word i / 64 = (q[i] > 0.5), LSB first
static void range_pack_queries(const float* q, uint32_t nq, uint32_t D, uint32_t W, uint64_t* out) {
    for (uint32_t i = 0; i < nq; ++i)
        for (uint32_t w = 0; w < W; ++w) {
            uint64_t m = 0;
            for (uint32_t b = 0; b < 64 && w * 64 + b < D; ++b)
                if (q[(size_t)i * D + w * 64 + b] > 0.5f) m |= 1ull << b;
            out[(size_t)i * W + w] = m;
        }
}

// search_range for nq queries, each with its own threshold: the exact scan of every row (the mask's rows when given), the rows
// with d <= threshold (ip: d >= threshold) counted into out_passed, the best min(passed, max_results) of them by the canonical
// (distance, row) key written best first and padded to max_results with rows ~0 and the worst distance.
extern "C" int lynse_hip_flat_search_range_f32(lynse_hip_flat* h, const float* queries, uint64_t nq, const float* thresholds,
                                               uint32_t max_results, int metric, const uint64_t* bitset_words, uint64_t n_words,
                                               uint64_t* out_rows, float* out_dists, uint32_t* out_counts, uint64_t* out_passed) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    if (!metric_valid(metric)) return set_error(LYNSE_ERR_UNKNOWN_METRIC, "Unknown metric id");
    if (nq == 0) return LYNSE_OK;
    if (!out_counts) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    if (max_results == 0) {   // search_range's first early return (:6416-6418): no device is touched
        memset(out_counts, 0, nq * 4);
        if (out_passed) memset(out_passed, 0, nq * 8);
        return LYNSE_OK;
    }
    if (!queries || !thresholds || !out_rows || !out_dists) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    LY_WRITER(h, lk);
    LY_TRY(use_device(h));
    if (h->row_stride != 1 || h->row_offset != 0) return set_error(LYNSE_ERR_UNSUPPORTED, "range search on a row-sharded handle is not supported");
    const bool binary = metric_binary(metric), asc = metric_ascending(metric);
    if (!binary && h->packed_only) return set_error(LYNSE_ERR_UNSUPPORTED, "a packed store answers the binary metrics only");
    const uint64_t n = h->n;
    const uint32_t D = h->dim, W = h->words;
    const float worst = asc ? INFINITY : -INFINITY;
    auto pad = [&](uint64_t q, uint32_t from) {
        for (uint32_t i = from; i < max_results; ++i) {
            out_rows[q * max_results + i] = ~0ull;
            out_dists[q * max_results + i] = worst;
        }
    };
    if (n == 0) {
        for (uint64_t q = 0; q < nq; ++q) {
            out_counts[q] = 0;
            if (out_passed) out_passed[q] = 0;
            pad(q, 0);
        }
        return LYNSE_OK;
    }
    if (binary) LY_TRY(ensure_packed_locked(h));
    if (!h->range) h->range = new RangeState();
    RangeState& p = *h->range;
    const uint32_t N = (uint32_t)std::min<uint64_t>(max_results, n);
    const uint64_t qc = ScoreCut::chunk(nq, n, N);
    uint32_t TQ = 0, R = 0, stride = 0;
    size_t lds = 0;
    if (!binary) {
        LY_TRY(range_plan(D, qc, &TQ, &R, &stride, &lds));
        LY_TRY(ensure_lds<k_range_scan>(PoolRerank::LDS_MAX));
    }
    const bool sort_dev = N <= 16384;
    if (sort_dev) {
        LY_TRY(ensure_lds<k_pool_select<256>>(PoolRerank::LDS_MAX));
        LY_TRY(ensure_lds<k_pool_select<1024>>(PoolRerank::LDS_MAX));
    }
    hipStream_t st = cur(h).stream;
    const uint64_t mask_words = bitset_words ? std::min<uint64_t>(n_words, (n + 63) / 64) : 0;
    if (bitset_words) {
        LY_TRY(ivf_grow(&p.d_mask, &p.mask_cap, (size_t)std::max<uint64_t>(1, mask_words)));
        if (mask_words) LY_HIP(hipMemcpyAsync(p.d_mask, bitset_words, (size_t)mask_words * 8, hipMemcpyHostToDevice, st));
    }
    if (binary) LY_TRY(ivf_grow(&p.d_qw, &p.qw_cap, (size_t)qc * W));
    else LY_TRY(ivf_grow(&p.d_q, &p.q_cap, (size_t)qc * D));
    LY_TRY(ivf_grow(&p.d_thr, &p.thr_cap, (size_t)qc));
    LY_TRY(ivf_grow(&p.d_cnt, &p.cnt_cap, (size_t)qc));
    LY_TRY(ivf_grow(&p.rr.d_keys, &p.rr.keys_cap, (size_t)qc * N));
    LY_TRY(ivf_grow(&p.rr.d_pcnt, &p.rr.pcnt_cap, (size_t)qc));
    if (sort_dev) LY_TRY(ivf_grow(&p.rr.d_out, &p.rr.out_cap, ((size_t)qc * N * 12 + (size_t)qc * 4 + 7) / 8));
    LY_TRY(p.cut.grow(qc, n));
    for (uint64_t q0 = 0; q0 < nq; q0 += qc) {
        const uint32_t nqc = (uint32_t)std::min<uint64_t>(qc, nq - q0);
        LY_HIP(hipMemcpyAsync(p.d_thr, thresholds + q0, (size_t)nqc * 4, hipMemcpyHostToDevice, st));
        LY_HIP(hipMemsetAsync(p.d_cnt, 0, (size_t)nqc * 4, st));
        if (binary) {
            p.qw.resize((size_t)nqc * W);
            range_pack_queries(queries + q0 * D, nqc, D, W, p.qw.data());
            LY_HIP(hipMemcpyAsync(p.d_qw, p.qw.data(), p.qw.size() * 8, hipMemcpyHostToDevice, st));
            RangeBinArgs a{h->packed, W, n, p.d_qw, p.d_thr, nqc, bitset_words ? p.d_mask : nullptr, mask_words, p.cut.d_S, p.d_cnt};
            const dim3 grid((uint32_t)std::min<uint64_t>((n + 31) / 32, (uint64_t)h->num_cu * 8), (nqc + RANGE_MAX_Q - 1) / RANGE_MAX_Q);
            switch (metric) {
            case M_HAMMING: hipLaunchKernelGGL(k_range_scan_bin<0>, grid, dim3(RANGE_NT), 0, st, a); break;
            case M_DICE: hipLaunchKernelGGL(k_range_scan_bin<2>, grid, dim3(RANGE_NT), 0, st, a); break;
            default: hipLaunchKernelGGL(k_range_scan_bin<1>, grid, dim3(RANGE_NT), 0, st, a); break;
            }
        } else {
            LY_HIP(hipMemcpyAsync(p.d_q, queries + q0 * D, (size_t)nqc * D * 4, hipMemcpyHostToDevice, st));
            const bool f16 = is_f16(h);
            RangeScanArgs a{f16 ? (const void*)h->rows_h : (const void*)h->rows, f16 ? h->ld16 : h->ld, D, f16 ? 1 : 0, n, p.d_q, p.d_thr, nqc,
                            metric, bitset_words ? p.d_mask : nullptr, mask_words, R, TQ, stride, p.cut.d_S, p.d_cnt};
            const dim3 grid((uint32_t)std::min<uint64_t>((n + R - 1) / R, (uint64_t)h->num_cu * 4), (nqc + TQ - 1) / TQ);
            hipLaunchKernelGGL(k_range_scan, grid, dim3(RANGE_NT), lds, st, a);
        }
        LY_HIP(hipGetLastError());
        LY_TRY(range_cut_and_order(p.cut, p.rr, p.d_cnt, p.cnt, p.keys, p.h_out, nqc, n, N, max_results, metric, st, out_rows + q0 * max_results,
                                   out_dists + q0 * max_results, out_counts + q0, out_passed ? out_passed + q0 : nullptr, []() { return (int)LYNSE_OK; }));
    }
    return LYNSE_OK;
}
