// additive_host.inc — top-k search under the additive metrics (ids 7-10) on a FLAT handle.  Included at the end of lynse_hip.hip
// after range_host.inc; kernels in additive.h, scratch, cut and order are the range search's (RangeState, ScoreCut::cut<true>,
// k_pool_select or select_pool_keys).  DESIGN.md §17.

// The LDS tiles of k_additive_scan for rows of D floats and chunks of up to qc queries.  First two workgroups per CU (one stages
// its tile while the other scores): up to 32 queries and 64 rows under 78 KiB (up to 8 queries: down to 16 rows); a row too wide
// for 8 queries and 32 rows there takes the whole LDS, queries first down to 8, then rows, then queries again.
static int additive_plan(uint32_t D, uint64_t qc, uint32_t* TQ, uint32_t* R, size_t* lds) {
    const size_t vec_b = (size_t)additive_lane_pitch(D) * 32 + 32;   // body + tail of one vector
    const uint32_t q_want = (uint32_t)std::min<uint64_t>(ADD_MAX_Q, qc <= 8 ? qc : (qc + 7) / 8 * 8);
    auto bytes = [&](uint32_t tq, uint32_t r) { return (size_t)(tq + r) * vec_b; };
    uint32_t tq = q_want, r = ADD_MAX_ROWS;
    size_t budget = 78u * 1024u;
    while (bytes(tq, r) > budget) {
        if (r > 32) r -= 32;
        else if (tq > 8) tq = tq > 16 ? tq - 8 : 8;
        else if (r > 16 && q_want <= 8) r = 16;   // a few queries: HBM decides, two workgroups per CU keep more bytes in flight
        else break;
    }
    if (bytes(tq, r) > budget) {
        budget = PoolRerank::LDS_MAX;
        tq = std::min<uint32_t>(q_want, 16);
        r = 32;
        while (bytes(tq, r) > budget && tq > 8) tq -= 8;
        while (bytes(tq, r) > budget && r > 1) --r;
        while (bytes(tq, r) > budget && tq > 1) --tq;
        if (bytes(tq, r) > budget) return set_error(LYNSE_ERR_UNSUPPORTED, "additive metrics: a query and a row do not fit in LDS");
    }
    *TQ = tq;
    *R = r;
    *lds = bytes(tq, r);
    return LYNSE_OK;
}

template <int M>
static int additive_launch(const AdditiveScanArgs& a, bool one, dim3 grid, size_t lds, hipStream_t st) {
    if (one) {
        LY_TRY((ensure_lds<k_additive_scan<M, 1>>(PoolRerank::LDS_MAX)));
        hipLaunchKernelGGL((k_additive_scan<M, 1>), grid, dim3(ADD_NT), lds, st, a);
    } else {
        LY_TRY((ensure_lds<k_additive_scan<M, 8>>(PoolRerank::LDS_MAX)));
        hipLaunchKernelGGL((k_additive_scan<M, 8>), grid, dim3(ADD_NT), lds, st, a);
    }
    LY_HIP(hipGetLastError());
    return LYNSE_OK;
}

// lynse_hip_flat_search_f32 / _filtered_f32 / _filtered_bitset_f32 for ids 7-10: the exact scan of every row into the score matrix
// (a masked-out row: RANGE_FAIL), the best N = min(k, live rows) keys of each query by the radix selection — or every key below
// RANGE_FAIL when no more than N rows are live; the host knows the live count without a read-back —, sorted in LDS up to 16,384
// keys and on the host beyond.  Output in the layout of lynse_hip_flat_search_f32: stride k, out_counts[q] = N entries valid.
static int additive_search(lynse_hip_flat* h, const float* queries, uint64_t nq, uint32_t k, int metric, bool filtered,
                           const uint64_t* subset, uint64_t n_subset, const uint64_t* bitset_words, uint64_t n_words,
                           uint64_t* out_rows, float* out_dists, uint32_t* out_counts) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    if (nq == 0) return LYNSE_OK;
    if (!queries || !out_counts || (k && (!out_rows || !out_dists))) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    if (filtered && !bitset_words && n_subset && !subset) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "subset is NULL");
    LY_WRITER(h, lk);
    LY_TRY(use_device(h));
    if (h->row_stride != 1 || h->row_offset != 0) return set_error(LYNSE_ERR_UNSUPPORTED, "the additive metrics on a row-sharded handle are not supported");
    if (h->packed_only) return set_error(LYNSE_ERR_UNSUPPORTED, "a packed store answers the binary metrics only");
    if (is_f16(h)) return set_error(LYNSE_ERR_UNSUPPORTED, "top-k under the additive metrics on an F16 shard is not supported (the range search is)");
    const uint64_t n = h->n;
    const uint32_t D = h->dim;
    // the rows searched, as BitSet words: the caller's (bits at or beyond len ignored), or built from the id list (ids >= len skipped,
    // duplicates once)
    if (!h->range) h->range = new RangeState();
    RangeState& p = *h->range;
    const uint64_t* words = nullptr;
    uint64_t mask_words = 0, live = n;
    if (filtered) {
        if (bitset_words) {
            words = bitset_words;
            mask_words = std::min<uint64_t>(n_words, (n + 63) / 64);
        } else {
            p.qw.assign((size_t)((n + 63) / 64), 0ull);
            for (uint64_t i = 0; i < n_subset; ++i)
                if (subset[i] < n) p.qw[(size_t)(subset[i] >> 6)] |= 1ull << (subset[i] & 63u);
            words = p.qw.data();
            mask_words = p.qw.size();
        }
        live = 0;
        for (uint64_t w = 0; w < mask_words; ++w) {
            uint64_t x = words[w];
            if (w == n / 64) x &= (1ull << (n % 64)) - 1ull;   // (the last, partial word: w * 64 + 63 >= n)
            live += (uint64_t)__builtin_popcountll(x);
        }
    }
    if (n == 0 || k == 0 || live == 0) {   // empty results, not an error (flat_mmap.rs:832-835, :498-500)
        memset(out_counts, 0, nq * 4);
        return LYNSE_OK;
    }
    const uint32_t N = (uint32_t)std::min<uint64_t>(k, live);
    const uint64_t qc = ScoreCut::chunk(nq, n, N);
    uint32_t TQ = 0, R = 0;
    size_t lds = 0;
    LY_TRY(additive_plan(D, qc, &TQ, &R, &lds));
    const bool sort_dev = N <= 16384;
    if (sort_dev) {
        LY_TRY(ensure_lds<k_pool_select<256>>(PoolRerank::LDS_MAX));
        LY_TRY(ensure_lds<k_pool_select<1024>>(PoolRerank::LDS_MAX));
    }
    hipStream_t st = cur(h).stream;
    if (filtered) {
        LY_TRY(ivf_grow(&p.d_mask, &p.mask_cap, (size_t)std::max<uint64_t>(1, mask_words)));
        if (mask_words) LY_HIP(hipMemcpyAsync(p.d_mask, words, (size_t)mask_words * 8, hipMemcpyHostToDevice, st));
    }
    LY_TRY(ivf_grow(&p.d_q, &p.q_cap, (size_t)qc * D));
    LY_TRY(ivf_grow(&p.rr.d_keys, &p.rr.keys_cap, (size_t)qc * N));
    LY_TRY(ivf_grow(&p.rr.d_pcnt, &p.rr.pcnt_cap, (size_t)qc));
    if (sort_dev) LY_TRY(ivf_grow(&p.rr.d_out, &p.rr.out_cap, ((size_t)qc * N * 12 + (size_t)qc * 4 + 7) / 8));
    LY_TRY(p.cut.grow(qc, n));
    const bool select = live > N;
    for (uint64_t q0 = 0; q0 < nq; q0 += qc) {
        const uint32_t nqc = (uint32_t)std::min<uint64_t>(qc, nq - q0);
        LY_HIP(hipMemcpyAsync(p.d_q, queries + q0 * D, (size_t)nqc * D * 4, hipMemcpyHostToDevice, st));
        AdditiveScanArgs a{h->rows, h->ld, D, n, p.d_q, nqc, filtered ? p.d_mask : nullptr, mask_words, R, TQ, p.cut.d_S};
        const dim3 grid((uint32_t)std::min<uint64_t>((n + R - 1) / R, (uint64_t)h->num_cu * 4), (nqc + TQ - 1) / TQ);
        switch (metric) {
        case M_L1: LY_TRY(additive_launch<M_L1>(a, nqc == 1, grid, lds, st)); break;
        case M_CHEBYSHEV: LY_TRY(additive_launch<M_CHEBYSHEV>(a, nqc == 1, grid, lds, st)); break;
        case M_CANBERRA: LY_TRY(additive_launch<M_CANBERRA>(a, nqc == 1, grid, lds, st)); break;
        default: LY_TRY(additive_launch<M_BRAY_CURTIS>(a, nqc == 1, grid, lds, st)); break;
        }
        // more live rows than N: the radix selection of the N best keys; else every key below RANGE_FAIL (a state that starts done)
        p.cut.sel0.assign(nqc, select ? PqSel{0ull, 64u, N, 0u, 0u} : PqSel{(uint64_t)(RANGE_FAIL - 1u), 32u, 0u, 1u, 0u});
        LY_TRY(p.cut.cut<true>(nqc, n, N, select, p.rr.d_keys, p.rr.d_pcnt, st));
        if (sort_dev) {   // sorted in LDS (k_pool_select), rows | distances | counts of the chunk back in one copy
            uint32_t p2 = 2;
            while (p2 < N) p2 <<= 1;
            const size_t o_dist = (size_t)nqc * N * 8, o_cnt = (size_t)nqc * N * 12, o_all = o_cnt + (size_t)nqc * 4;
            uint8_t* ob = reinterpret_cast<uint8_t*>(p.rr.d_out);
            PoolRerankArgs x{};
            x.pool_cnt = p.rr.d_pcnt;
            x.pool_ld = N;
            x.p2 = p2;
            x.metric = metric;
            x.k = N;
            x.out_k = N;
            x.out_rows = p.rr.d_out;
            x.out_dists = reinterpret_cast<float*>(ob + o_dist);
            x.out_counts = reinterpret_cast<uint32_t*>(ob + o_cnt);
            x.keys_out = p.rr.d_keys;
            if (p2 >= 2048) hipLaunchKernelGGL(k_pool_select<1024>, dim3(nqc), dim3(1024), (size_t)p2 * 8, st, x);
            else hipLaunchKernelGGL(k_pool_select<256>, dim3(nqc), dim3(256), (size_t)p2 * 8, st, x);
            LY_HIP(hipGetLastError());
            p.h_out.resize((o_all + 7) / 8);
            LY_HIP(hipMemcpyAsync(p.h_out.data(), p.rr.d_out, o_all, hipMemcpyDeviceToHost, st));
            LY_TRY(stream_wait(st));
            const uint8_t* hb = reinterpret_cast<const uint8_t*>(p.h_out.data());
            for (uint32_t i = 0; i < nqc; ++i) {
                memcpy(out_rows + (q0 + i) * k, hb + (size_t)i * N * 8, (size_t)N * 8);
                memcpy(out_dists + (q0 + i) * k, hb + o_dist + (size_t)i * N * 4, (size_t)N * 4);
                out_counts[q0 + i] = N;
            }
        } else {   // beyond the 16,384 keys of the LDS sort: sorted on the host
            p.keys.resize((size_t)nqc * N);
            LY_HIP(hipMemcpyAsync(p.keys.data(), p.rr.d_keys, p.keys.size() * 8, hipMemcpyDeviceToHost, st));
            LY_TRY(stream_wait(st));
            for (uint32_t i = 0; i < nqc; ++i)
                out_counts[q0 + i] = select_pool_keys(p.keys.data() + (size_t)i * N, N, N, N, true, out_rows + (q0 + i) * k, out_dists + (q0 + i) * k);
        }
    }
    return LYNSE_OK;
}
