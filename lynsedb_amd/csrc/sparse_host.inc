// sparse_host.inc — sparse-vector search (Collection::add_sparse_vectors / search_sparse, src/engine.rs:550-718, :4250-4279,
// :4962-5002, :6925-6965): a handle of its own that holds the CSR rows in HBM.  Included at the end of lynse_hip.hip after
// additive_host.inc; the kernel is in sparse.h, the cut and the order are the range search's (range_cut_and_order, range_host.inc).
// DESIGN.md §18.

struct lynse_hip_sparse {
    std::shared_mutex rw;
    int device = 0;
    uint32_t num_cu = 256;
    hipStream_t stream = nullptr;
    uint64_t n = 0, nnz = 0;
    uint64_t* d_indptr = nullptr;   // structure of arrays: the index stream is read without the values
    uint32_t* d_indices = nullptr;
    float* d_values = nullptr;
    size_t indptr_cap = 0, indices_cap = 0, values_cap = 0;
    // the scratch of a search (it runs under the exclusive lock)
    uint32_t *d_tab = nullptr, *d_cnt = nullptr;
    uint64_t* d_mask = nullptr;
    size_t tab_cap = 0, cnt_cap = 0, mask_cap = 0;
    ScoreCut cut;
    PoolRerank rr;
    std::vector<uint32_t> cnt, tab, uni;
    std::vector<uint64_t> keys, h_out;
    bool profiling = false;
    lynse_hip_profile prof{};
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};   // the scan begins / the scan ends / the last launch of the chunk
};

// normalize_sparse_entries (:6925-6943) for n vectors in CSR: a non-finite value is an error, zeros are skipped, the rest merged per
// index in input order (each index from 0.0f, += in f32), merged zeros dropped, ascending by index.
extern "C" int lynse_hip_sparse_normalize(const uint64_t* indptr, const uint32_t* indices, const float* values, uint64_t n,
                                          uint64_t* out_indptr, uint32_t* out_indices, float* out_values) {
    if (!indptr || !out_indptr) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    if (indptr[0] != 0) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "sparse indptr must start at 0");
    for (uint64_t r = 0; r < n; ++r)
        if (indptr[r + 1] < indptr[r]) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "sparse indptr must not decrease");
    if (indptr[n] && (!indices || !values || !out_indices || !out_values)) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    for (uint64_t e = 0; e < indptr[n]; ++e)
        if (!std::isfinite(values[e])) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "sparse vector values must be finite");
    std::vector<uint64_t> ord;
    uint64_t o = 0;
    out_indptr[0] = 0;
    for (uint64_t r = 0; r < n; ++r) {
        ord.clear();
        for (uint64_t e = indptr[r]; e < indptr[r + 1]; ++e)
            if (values[e] != 0.0f) ord.push_back(e);
        std::stable_sort(ord.begin(), ord.end(), [&](uint64_t x, uint64_t y) { return indices[x] < indices[y]; });   // input order within an index
        for (size_t i = 0; i < ord.size();) {
            const uint32_t idx = indices[ord[i]];
            float sum = 0.0f;
            for (; i < ord.size() && indices[ord[i]] == idx; ++i) sum += values[ord[i]];
            if (sum != 0.0f) {
                out_indices[o] = idx;
                out_values[o] = sum;
                ++o;
            }
        }
        out_indptr[r + 1] = o;
    }
    return LYNSE_OK;
}

// the form set_rows and search accept: what normalize_sparse_entries leaves, plus finite sums
static int sparse_validate(const uint64_t* indptr, const uint32_t* indices, const float* values, uint64_t n, const char* what) {
    const std::string w(what);
    if (!indptr) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    if (indptr[0] != 0) return set_error(LYNSE_ERR_INVALID_ARGUMENT, w + ": indptr must start at 0");
    for (uint64_t r = 0; r < n; ++r)
        if (indptr[r + 1] < indptr[r]) return set_error(LYNSE_ERR_INVALID_ARGUMENT, w + ": indptr must not decrease");
    if (indptr[n] && (!indices || !values)) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    for (uint64_t r = 0; r < n; ++r)
        for (uint64_t e = indptr[r]; e < indptr[r + 1]; ++e) {
            if (e > indptr[r] && indices[e] <= indices[e - 1])
                return set_error(LYNSE_ERR_INVALID_ARGUMENT, w + ": indices must be strictly ascending within a vector");
            if (!std::isfinite(values[e])) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "sparse vector values must be finite");
            if (values[e] == 0.0f) return set_error(LYNSE_ERR_INVALID_ARGUMENT, w + ": values must be non-zero (normalise the vector first)");
        }
    return LYNSE_OK;
}

extern "C" int lynse_hip_sparse_create(int device, lynse_hip_sparse** out) {
    if (!out) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    int ndev = 0;
    LY_TRY(lynse_hip_device_count(&ndev));
    if (ndev <= 0) return set_error(LYNSE_ERR_DEVICE, "no HIP device available (this library has no CPU fallback)");
    if (device < 0 || device >= ndev) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "device ordinal out of range");
    LY_HIP(hipSetDevice(device));
    auto* h = new lynse_hip_sparse();
    h->device = device;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) h->num_cu = prop.multiProcessorCount;
    const hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete h;
        return set_error(LYNSE_ERR_DEVICE, std::string("hipStreamCreate: ") + hipGetErrorString(e));
    }
    *out = h;
    return LYNSE_OK;
}

extern "C" int lynse_hip_sparse_destroy(lynse_hip_sparse* h) {
    if (!h) return LYNSE_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (void* p : {(void*)h->d_indptr, (void*)h->d_indices, (void*)h->d_values, (void*)h->d_tab, (void*)h->d_cnt, (void*)h->d_mask})
        if (p) (void)hipFree(p);
    h->cut.release();
    h->rr.release();
    for (hipEvent_t e : h->ev)
        if (e) (void)hipEventDestroy(e);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return LYNSE_OK;
}

// Replaces the whole store (SparseVectorStore::upsert_many rewrites its whole map too).  Everything is checked before any device work.
extern "C" int lynse_hip_sparse_set_rows(lynse_hip_sparse* h, const uint64_t* indptr, const uint32_t* indices, const float* values, uint64_t n) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    if (n >= (1ull << 32)) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "sparse rows: a selection key carries a 32-bit row, n must be below 2^32");
    if (n) LY_TRY(sparse_validate(indptr, indices, values, n, "sparse rows"));
    std::unique_lock<std::shared_mutex> lk(h->rw);
    LY_HIP(hipSetDevice(h->device));
    if (n == 0) {
        h->n = h->nnz = 0;
        return LYNSE_OK;
    }
    const uint64_t nnz = indptr[n];
    h->n = h->nnz = 0;   // (a failed upload leaves an empty store, not a torn one)
    LY_TRY(ivf_grow(&h->d_indptr, &h->indptr_cap, (size_t)n + 1));
    LY_TRY(ivf_grow(&h->d_indices, &h->indices_cap, (size_t)std::max<uint64_t>(1, nnz)));
    LY_TRY(ivf_grow(&h->d_values, &h->values_cap, (size_t)std::max<uint64_t>(1, nnz)));
    LY_TRY(h2d_done(h->d_indptr, indptr, ((size_t)n + 1) * 8));
    if (nnz) {
        LY_TRY(h2d_done(h->d_indices, indices, (size_t)nnz * 4));
        LY_TRY(h2d_done(h->d_values, values, (size_t)nnz * 4));
    }
    h->n = n;
    h->nnz = nnz;
    return LYNSE_OK;
}

extern "C" int lynse_hip_sparse_len(lynse_hip_sparse* h, uint64_t* out_rows, uint64_t* out_nnz) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    std::shared_lock<std::shared_mutex> lk(h->rw);
    if (out_rows) *out_rows = h->n;
    if (out_nnz) *out_nnz = h->nnz;
    return LYNSE_OK;
}

extern "C" uint64_t lynse_hip_sparse_hbm_bytes(lynse_hip_sparse* h) {
    if (!h) return 0;
    std::shared_lock<std::shared_mutex> lk(h->rw);
    return (uint64_t)h->indptr_cap * 8 + (uint64_t)h->indices_cap * 4 + (uint64_t)h->values_cap * 4;
}

extern "C" int lynse_hip_sparse_profile_enable(lynse_hip_sparse* h, int on) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    std::unique_lock<std::shared_mutex> lk(h->rw);
    h->profiling = on != 0;
    return LYNSE_OK;
}

extern "C" int lynse_hip_sparse_profile_get(lynse_hip_sparse* h, lynse_hip_profile* out, int reset) {
    if (!h || !out) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    std::unique_lock<std::shared_mutex> lk(h->rw);
    *out = h->prof;
    if (reset) h->prof = lynse_hip_profile{};
    return LYNSE_OK;
}

// LDS of k_sparse_scan for tiles of tq queries whose largest union holds U indices
static size_t sparse_lds_bytes(uint32_t tq, uint32_t U, uint32_t* H, uint32_t* hbits, uint32_t* tab_words) {
    uint32_t b = 4;
    while ((1ull << b) < 2ull * U) ++b;   // at most half the slots taken
    *hbits = b;
    *H = 1u << b;
    *tab_words = 2u * *H + U * tq + SPARSE_PRE_WORDS;
    return ((size_t)*tab_words + (size_t)tq * SPARSE_ROWS + tq) * 4;
}

// The query tiles of a chunk: the largest TQ <= 16 (halved down to 1) at which every tile's table fits the LDS, and the tables
// themselves in h->tab, one per tile.  A single query of up to SPARSE_MAX_NNZ entries always fits (the caller has checked that).
static int sparse_plan(lynse_hip_sparse* h, const uint64_t* qp, const uint32_t* qi, const float* qv, uint32_t nqc, SparseScanArgs* a, size_t* lds) {
    uint32_t tq = std::min<uint32_t>(SPARSE_MAX_Q, nqc), U = 0, H = 0, hbits = 0, words = 0;
    std::vector<uint32_t>& uni = h->uni;
    auto tile_union = [&](uint32_t t0, uint32_t t1) {   // the ascending distinct indices of queries t0 .. t1 - 1
        uni.assign(qi + qp[t0], qi + qp[t1]);
        std::sort(uni.begin(), uni.end());
        uni.erase(std::unique(uni.begin(), uni.end()), uni.end());
    };
    for (;; tq = (tq + 1) / 2) {
        U = 1;
        for (uint32_t t0 = 0; t0 < nqc; t0 += tq) {
            tile_union(t0, std::min(nqc, t0 + tq));
            U = std::max<uint32_t>(U, (uint32_t)uni.size());
        }
        *lds = sparse_lds_bytes(tq, U, &H, &hbits, &words);
        if (*lds <= PoolRerank::LDS_MAX) break;
        if (tq == 1) return set_error(LYNSE_ERR_UNSUPPORTED, "sparse search: the table of one query does not fit in LDS");
    }
    const uint32_t tiles = (nqc + tq - 1) / tq;
    h->tab.assign((size_t)tiles * words, 0u);
    for (uint32_t t = 0; t < tiles; ++t) {
        const uint32_t t0 = t * tq, t1 = std::min(nqc, t0 + tq);
        tile_union(t0, t1);
        uint32_t* keys = h->tab.data() + (size_t)t * words;
        uint32_t* vidx = keys + H;
        float* vals = reinterpret_cast<float*>(vidx + H);
        uint32_t* pre = vidx + H + (size_t)U * tq;
        for (uint32_t i = 0; i < uni.size(); ++i) {
            uint32_t s = sparse_slot(uni[i], hbits);
            while (vidx[s]) s = (s + 1) & (H - 1);
            keys[s] = uni[i];
            vidx[s] = i + 1;
            const uint32_t b = uni[i] & ((1u << SPARSE_PRE_BITS) - 1u);
            pre[b >> 5] |= 1u << (b & 31u);
        }
        for (uint32_t q = t0; q < t1; ++q)
            for (uint64_t e = qp[q]; e < qp[q + 1]; ++e) {
                const size_t i = (size_t)(std::lower_bound(uni.begin(), uni.end(), qi[e]) - uni.begin());
                vals[i * tq + (q - t0)] = qv[e];
            }
    }
    a->tab_words = words;
    a->H = H;
    a->hbits = hbits;
    a->U = U;
    a->TQ = tq;
    return LYNSE_OK;
}

// SparseVectorStore::search (:660-695) for nq normalised queries in CSR: the rows with score != 0 (of the mask's rows when given)
// counted into out_passed, the best min(passed, k) of them by (score descending, NaN as -inf, row ascending) written best first at
// stride k and padded with rows ~0 and -inf.
extern "C" int lynse_hip_sparse_search(lynse_hip_sparse* h, const uint64_t* q_indptr, const uint32_t* q_indices, const float* q_values,
                                       uint64_t nq, uint32_t k, const uint64_t* bitset_words, uint64_t n_words, uint64_t* out_rows,
                                       float* out_scores, uint32_t* out_counts, uint64_t* out_passed) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    if (nq == 0) return LYNSE_OK;
    if (!out_counts) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    auto nothing = [&]() -> int {
        memset(out_counts, 0, nq * 4);
        if (out_passed) memset(out_passed, 0, nq * 8);
        for (uint64_t i = 0; k && out_rows && out_scores && i < nq * k; ++i) {
            out_rows[i] = ~0ull;
            out_scores[i] = -INFINITY;
        }
        return LYNSE_OK;
    };
    if (k == 0) return nothing();   // (:667-669)
    if (!out_rows || !out_scores) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    if (nq >= (1ull << 32)) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "too many queries");
    LY_TRY(sparse_validate(q_indptr, q_indices, q_values, nq, "sparse queries"));
    for (uint64_t q = 0; q < nq; ++q)
        if (q_indptr[q + 1] - q_indptr[q] > SPARSE_MAX_NNZ)
            return set_error(LYNSE_ERR_UNSUPPORTED, "sparse search: a query of more than 4096 entries does not fit its table in LDS");
    std::unique_lock<std::shared_mutex> lk(h->rw);
    LY_HIP(hipSetDevice(h->device));
    const uint64_t n = h->n;
    if (n == 0 || q_indptr[nq] == 0) return nothing();
    const uint32_t N = (uint32_t)std::min<uint64_t>(k, n);
    const uint64_t qc = ScoreCut::chunk(nq, n, N);
    LY_TRY(ensure_lds<k_sparse_scan>(PoolRerank::LDS_MAX));
    const bool sort_dev = N <= 16384;
    if (sort_dev) {
        LY_TRY(ensure_lds<k_pool_select<256>>(PoolRerank::LDS_MAX));
        LY_TRY(ensure_lds<k_pool_select<1024>>(PoolRerank::LDS_MAX));
    }
    hipStream_t st = h->stream;
    const uint64_t mask_words = bitset_words ? std::min<uint64_t>(n_words, (n + 63) / 64) : 0;
    if (bitset_words) LY_TRY(ivf_grow(&h->d_mask, &h->mask_cap, (size_t)std::max<uint64_t>(1, mask_words)));
    LY_TRY(ivf_grow(&h->d_cnt, &h->cnt_cap, (size_t)qc));
    LY_TRY(ivf_grow(&h->rr.d_keys, &h->rr.keys_cap, (size_t)qc * N));
    LY_TRY(ivf_grow(&h->rr.d_pcnt, &h->rr.pcnt_cap, (size_t)qc));
    if (sort_dev) LY_TRY(ivf_grow(&h->rr.d_out, &h->rr.out_cap, ((size_t)qc * N * 12 + (size_t)qc * 4 + 7) / 8));
    LY_TRY(h->cut.grow(qc, n));
    // (the caller's words are queued only once nothing before the first launch can fail and return with the copy still pending)
    if (mask_words) LY_HIP(hipMemcpyAsync(h->d_mask, bitset_words, (size_t)mask_words * 8, hipMemcpyHostToDevice, st));
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
    for (uint64_t q0 = 0; q0 < nq; q0 += qc) {
        const uint32_t nqc = (uint32_t)std::min<uint64_t>(qc, nq - q0);
        SparseScanArgs a{};
        size_t lds = 0;
        // (the chunk's queries with their own indptr origin: positions are taken relative to q_indptr[q0])
        const uint64_t e0 = q_indptr[q0];
        h->keys.resize((size_t)nqc + 1);
        for (uint32_t i = 0; i <= nqc; ++i) h->keys[i] = q_indptr[q0 + i] - e0;
        int rc = sparse_plan(h, h->keys.data(), q_indices + e0, q_values + e0, nqc, &a, &lds);
        if (rc == LYNSE_OK) rc = ivf_grow(&h->d_tab, &h->tab_cap, h->tab.size());
        if (rc != LYNSE_OK) {   // (the copy of the caller's mask words may still be queued: it must not outlive the call)
            (void)hipStreamSynchronize(st);
            return rc;
        }
        LY_HIP(hipMemcpyAsync(h->d_tab, h->tab.data(), h->tab.size() * 4, hipMemcpyHostToDevice, st));
        LY_HIP(hipMemsetAsync(h->d_cnt, 0, (size_t)nqc * 4, st));
        a.indptr = h->d_indptr;
        a.indices = h->d_indices;
        a.values = h->d_values;
        a.n = n;
        a.tables = h->d_tab;
        a.nq = nqc;
        a.mask = bitset_words ? h->d_mask : nullptr;
        a.mask_words = mask_words;
        a.S = h->cut.d_S;
        a.count = h->d_cnt;
        const uint32_t qtiles = (nqc + a.TQ - 1) / a.TQ;
        const dim3 grid((uint32_t)std::min<uint64_t>((n + SPARSE_ROWS - 1) / SPARSE_ROWS, (uint64_t)h->num_cu * 4), qtiles);
        if (timed) LY_HIP(hipEventRecord(h->ev[0], st));
        hipLaunchKernelGGL(k_sparse_scan, grid, dim3(SPARSE_NT), lds, st, a);
        LY_HIP(hipGetLastError());
        if (timed) {
            LY_HIP(hipEventRecord(h->ev[1], st));
            h->prof.scan_launches += 1;
            h->prof.scan_rows += n * qtiles;
            h->prof.scan_bytes += (h->nnz * 8 + (n + 1) * 8) * qtiles;
        }
        LY_TRY(range_cut_and_order(h->cut, h->rr, h->d_cnt, h->cnt, h->keys, h->h_out, nqc, n, N, k, M_IP, st, out_rows + q0 * k, out_scores + q0 * k,
                                   out_counts + q0, out_passed ? out_passed + q0 : nullptr, chunk_done));
    }
    return LYNSE_OK;
}
