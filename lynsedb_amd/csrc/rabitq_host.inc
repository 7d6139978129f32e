// rabitq_host.inc — FLAT-{IP,L2,COS}-RABITQ on a FLAT handle (RaBitQIndex, src/storage/rabitq_mmap.rs; Collection,
// src/engine.rs:4476, :4552, :5504-5526).  Included at the end of lynse_hip.hip after pq_host.inc (the SmallRng restatement is
// pqrng); kernels in rabitq.h, the pool cut is ScoreCut and the exact rescore PoolRerank (rerank_host.inc).  DESIGN.md §15.

// The index and the per-handle search scratch.  Codes cover the first n rows of the handle: rows appended after a build or a load
// stay outside the index.
struct RbqState {
    uint32_t P = 0, cb = 0, ng = 0;   // padded_dim, code bytes, 16-byte column groups of the device layout
    uint64_t n = 0;
    std::vector<uint64_t> sign;       // ceil(P / 64) sign words
    uint64_t* d_sign = nullptr;
    uint32_t* codes = nullptr;        // device layout (rbq_word_index): ceil(n / 64) * ng * 64 uint4
    float* norms = nullptr;           // [n]
    float *d_q = nullptr, *d_lut = nullptr, *d_total = nullptr;
    size_t q_cap = 0, lut_cap = 0, total_cap = 0;
    ScoreCut cut;
    PoolRerank rr;
    double searches = 0.0, scan_us = 0.0, rescore_us = 0.0;

    void free_index() {
        for (void* p : {(void*)d_sign, (void*)codes, (void*)norms})
            if (p) (void)hipFree(p);
        d_sign = nullptr;
        codes = nullptr;
        norms = nullptr;
        sign.clear();
        P = cb = ng = 0;
        n = 0;
    }
    ~RbqState() {
        free_index();
        for (void* p : {(void*)d_q, (void*)d_lut, (void*)d_total})
            if (p) (void)hipFree(p);
        cut.release();
        rr.release();
    }
};

static void rbq_release(lynse_hip_flat* h) {
    delete h->rbq;
    h->rbq = nullptr;
}

// generate_sign_words (rabitq_mmap.rs:337-340): word w = the w-th next_u64() of SmallRng::seed_from_u64(seed)
extern "C" int lynse_hip_rabitq_sign_words(uint64_t seed, uint64_t count, uint64_t* out) {
    if (count && !out) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    pqrng::Xoshiro256pp rng = pqrng::Xoshiro256pp::seed_from_u64(seed);
    for (uint64_t i = 0; i < count; ++i) out[i] = rng.next();
    return LYNSE_OK;
}

static inline uint32_t rbq_next_pow2(uint32_t d) {
    uint32_t p = 1;
    while (p < d) p <<= 1;
    return p;
}
static inline size_t rbq_code_words(uint64_t n, uint32_t ng) { return (size_t)((n + 63) / 64) * ng * 64 * 4; }

static int rbq_check_handle(const lynse_hip_flat* h) {
    if (h->dtype != LYNSE_DTYPE_F32) return set_error(LYNSE_ERR_UNSUPPORTED, "RaBitQ on an F16 shard is not supported");
    if (h->packed_only) return set_error(LYNSE_ERR_UNSUPPORTED, "RaBitQ is defined for float rows (ip / l2 / cosine)");
    if (h->row_stride != 1 || h->row_offset != 0) return set_error(LYNSE_ERR_UNSUPPORTED, "a RaBitQ index is not row-sharded");
    if (h->dim > (1u << 30) || (size_t)rbq_next_pow2(h->dim) * 4 > PoolRerank::LDS_MAX)
        return set_error(LYNSE_ERR_UNSUPPORTED, "RaBitQ: the padded vector does not fit in LDS");
    return LYNSE_OK;
}

// the rotation kernels keep rb * P floats in LDS: past 64 KiB the limit is raised once per kernel
static int rbq_rotation_lds(size_t bytes) {
    if (bytes <= 64u * 1024u) return LYNSE_OK;
    LY_TRY(ensure_lds<k_rbq_encode>(PoolRerank::LDS_MAX));
    return ensure_lds<k_rbq_query>(PoolRerank::LDS_MAX);
}

// a fresh index of n rows in `out` (device buffers allocated, the codes zeroed, the sign words uploaded)
static int rbq_alloc(RbqState& out, uint32_t dim, uint64_t n, const uint64_t* sign_words, uint32_t n_sign_words) {
    out.P = rbq_next_pow2(dim);
    out.cb = (out.P + 7) / 8;
    out.ng = ((out.cb + 3) / 4 + 3) / 4;
    out.n = n;
    const uint32_t nw = (out.P + 63) / 64;
    out.sign.assign(nw, 0ull);   // a word the file does not hold negates nothing (apply_signs: word_idx < sign_words.len())
    for (uint32_t w = 0; w < nw && w < n_sign_words; ++w) out.sign[w] = sign_words[w];
    LY_HIP(hipMalloc(&out.d_sign, (size_t)nw * 8));
    LY_HIP(hipMalloc(&out.codes, rbq_code_words(n, out.ng) * 4));
    LY_HIP(hipMalloc(&out.norms, (size_t)n * 4));
    LY_TRY(h2d_done(out.d_sign, out.sign.data(), (size_t)nw * 8));
    LY_TRY(memset_done(out.codes, 0, rbq_code_words(n, out.ng) * 4));
    return LYNSE_OK;
}

// install `fresh` as the handle's index, keeping the search scratch
static void rbq_install(lynse_hip_flat* h, RbqState& fresh) {
    if (!h->rbq) h->rbq = new RbqState();
    RbqState& r = *h->rbq;
    r.free_index();
    r.P = fresh.P; r.cb = fresh.cb; r.ng = fresh.ng; r.n = fresh.n;
    r.sign.swap(fresh.sign);
    r.d_sign = fresh.d_sign; r.codes = fresh.codes; r.norms = fresh.norms;
    fresh.d_sign = nullptr; fresh.codes = nullptr; fresh.norms = nullptr;
}

// RaBitQIndex::build (rabitq_mmap.rs:68-156) over the handle's rows
extern "C" int lynse_hip_flat_build_rabitq(lynse_hip_flat* h) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    LY_WRITER(h, lk);
    LY_TRY(use_device(h));
    LY_TRY(rbq_check_handle(h));
    const uint64_t n = h->n;
    if (n == 0) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "need at least one vector");
    if (n > 0xffffffffull) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "a RaBitQ index holds at most 2^32 - 1 rows");
    const uint32_t nw = (rbq_next_pow2(h->dim) + 63) / 64;
    std::vector<uint64_t> sign(nw);
    LY_TRY(lynse_hip_rabitq_sign_words(42, nw, sign.data()));
    RbqState fresh;   // (freed on every failing path)
    LY_TRY(rbq_alloc(fresh, h->dim, n, sign.data(), nw));
    const uint32_t rb = std::max<uint32_t>(1, std::min<uint32_t>(8, 4096u / fresh.P));
    const size_t lds = (size_t)rb * fresh.P * 4;
    LY_TRY(rbq_rotation_lds(lds));
    hipStream_t st = cur(h).stream;
    RbqEncodeArgs a{h->rows, h->ld, h->dim, fresh.P, n, rb, fresh.ng, fresh.d_sign, fresh.codes, fresh.norms};
    hipLaunchKernelGGL(k_rbq_encode, dim3((uint32_t)((n + rb - 1) / rb)), dim3(RBQ_ENC_NT), lds, st, a);
    LY_HIP(hipGetLastError());
    LY_HIP(hipStreamSynchronize(st));
    rbq_install(h, fresh);
    return LYNSE_OK;
}

// RaBitQIndex::load's in-memory half: codes[n][code_bytes] and norms[n] as the file holds them
extern "C" int lynse_hip_flat_load_rabitq(lynse_hip_flat* h, uint32_t dim, const uint64_t* sign_words, uint32_t n_sign_words,
                                          const uint8_t* codes, const float* norms, uint64_t n) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    LY_WRITER(h, lk);
    LY_TRY(use_device(h));
    LY_TRY(rbq_check_handle(h));
    if (dim == 0 || dim != h->dim) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "Invalid RaBitQ dimensions");
    if (n == 0) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "need at least one vector");
    if (n > 0xffffffffull) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "a RaBitQ index holds at most 2^32 - 1 rows");
    if (n > h->n) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "the RaBitQ index covers more rows than the handle holds");
    if (!codes || !norms || (n_sign_words && !sign_words)) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    RbqState fresh;
    LY_TRY(rbq_alloc(fresh, dim, n, sign_words, n_sign_words));
    // [n][code_bytes] -> the device layout, on the host
    std::vector<uint32_t> dev(rbq_code_words(n, fresh.ng), 0u);
    const uint32_t cb = fresh.cb;
    for (uint64_t r = 0; r < n; ++r)
        for (uint32_t b = 0; b < cb; ++b)
            dev[rbq_word_index(r, b >> 2, fresh.ng)] |= (uint32_t)codes[r * cb + b] << (8 * (b & 3u));
    LY_TRY(h2d_done(fresh.codes, dev.data(), dev.size() * 4));
    LY_TRY(h2d_done(fresh.norms, norms, (size_t)n * 4));
    rbq_install(h, fresh);
    return LYNSE_OK;
}

extern "C" int lynse_hip_flat_rabitq_params(lynse_hip_flat* h, uint32_t* dims, uint64_t* n_rbq, uint64_t* sign_words, uint8_t* codes,
                                            float* norms) {
    if (!h || !dims || !n_rbq) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    std::shared_lock<std::shared_mutex> lk(h->rw);
    if (!h->rbq || !h->rbq->codes) {
        dims[0] = dims[1] = dims[2] = 0;
        *n_rbq = 0;
        return LYNSE_OK;
    }
    const RbqState& r = *h->rbq;
    dims[0] = h->dim; dims[1] = r.P; dims[2] = r.cb;
    *n_rbq = r.n;
    LY_TRY(use_device(h));
    if (sign_words) memcpy(sign_words, r.sign.data(), r.sign.size() * 8);
    if (codes) {
        std::vector<uint32_t> dev(rbq_code_words(r.n, r.ng));
        LY_HIP(hipMemcpy(dev.data(), r.codes, dev.size() * 4, hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < r.n; ++i)
            for (uint32_t b = 0; b < r.cb; ++b)
                codes[i * r.cb + b] = (uint8_t)(dev[rbq_word_index(i, b >> 2, r.ng)] >> (8 * (b & 3u)));
    }
    if (norms) LY_HIP(hipMemcpy(norms, r.norms, (size_t)r.n * 4, hipMemcpyDeviceToHost));
    return LYNSE_OK;
}

extern "C" int lynse_hip_flat_drop_rabitq(lynse_hip_flat* h) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    LY_WRITER(h, lk);
    LY_TRY(use_device(h));
    if (h->rbq) h->rbq->free_index();
    return LYNSE_OK;
}

extern "C" int lynse_hip_flat_rabitq_stage_times(lynse_hip_flat* h, double* out3, int reset) {
    if (!h || !out3) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    LY_WRITER(h, lk);
    if (!h->rbq) { out3[0] = out3[1] = out3[2] = 0.0; return LYNSE_OK; }
    out3[0] = h->rbq->searches;
    out3[1] = h->rbq->scan_us;
    out3[2] = h->rbq->rescore_us;
    if (reset) h->rbq->searches = h->rbq->scan_us = h->rbq->rescore_us = 0.0;
    return LYNSE_OK;
}

// RaBitQIndex::search_candidates + rescore_exact_with (rabitq_mmap.rs:177-227): k' = min(k, n_rbq), N = min(k' * oversample, n_rbq)
// rows by the canonical (binary score, row) key, rescored with compute_distance_f32 on the original rows, the best k' by (exact
// distance, row).  Queries go in chunks: score matrix <= 512 MiB, pool <= 256 MiB (ScoreCut::chunk), byte tables <= 256 MiB.
extern "C" int lynse_hip_flat_search_rabitq_f32(lynse_hip_flat* h, const float* queries, uint64_t nq, uint32_t k, int metric,
                                                uint32_t oversample, uint64_t* out_rows, float* out_dists, uint32_t* out_counts) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    LY_TRY(metric_check(metric));
    if (metric_binary(metric)) return set_error(LYNSE_ERR_UNSUPPORTED, "RaBitQ is defined for ip / l2 / cosine");
    if (nq == 0) return LYNSE_OK;
    if (!queries || !out_counts || (k && (!out_rows || !out_dists))) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    LY_WRITER(h, lk);
    LY_TRY(use_device(h));
    LY_TRY(rbq_check_handle(h));
    if (!h->rbq || !h->rbq->codes) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "no RaBitQ index on this handle: build or load one first");
    RbqState& p = *h->rbq;
    const uint64_t n = p.n;
    const uint32_t D = h->dim;
    if (k == 0) { memset(out_counts, 0, nq * 4); return LYNSE_OK; }
    const uint32_t kk = (uint32_t)std::min<uint64_t>(k, n);
    const uint32_t N = (uint32_t)std::min<uint64_t>((uint64_t)kk * oversample, n);
    if (N == 0) { memset(out_counts, 0, nq * 4); return LYNSE_OK; }
    const bool asc = metric_ascending(metric);
    const size_t lut_q = (size_t)p.cb * 256;   // floats of one query's tables
    const uint64_t qc = std::max<uint64_t>(1, std::min<uint64_t>(ScoreCut::chunk(nq, n, N), (256ull << 20) / (lut_q * 4)));
    PoolRerank::Search rr(p.rr);
    rr.split_small = true;   // a pool is 200 k rows: a single query's would be gathered by one CU
    LY_TRY(rr.begin(h->rows, n, h->ld, D, metric, N, kk, k, qc, false, h->profiling.load(), "RaBitQ rescore"));
    LY_TRY(ivf_grow(&p.d_q, &p.q_cap, (size_t)qc * D));
    LY_TRY(ivf_grow(&p.d_lut, &p.lut_cap, (size_t)qc * lut_q));
    LY_TRY(ivf_grow(&p.d_total, &p.total_cap, (size_t)qc));
    LY_TRY(p.cut.grow(qc, n));
    LY_TRY(rbq_rotation_lds((size_t)p.P * 4));
    hipStream_t st = cur(h).stream;
    for (uint64_t q0 = 0; q0 < nq; q0 += qc) {
        const uint32_t nqc = (uint32_t)std::min<uint64_t>(qc, nq - q0);
        LY_HIP(hipMemcpyAsync(p.d_q, queries + q0 * D, (size_t)nqc * D * 4, hipMemcpyHostToDevice, st));
        LY_TRY(rr.pool_start(st));
        // a small batch spreads each query's tables over up to 8 workgroups; one more per query sums total_q
        const uint32_t parts = nqc >= 32 ? 1u : std::max<uint32_t>(1, std::min<uint32_t>(8, p.cb / 16));
        hipLaunchKernelGGL(k_rbq_query, dim3(nqc, parts + 1), dim3(RBQ_Q_NT), (size_t)p.P * 4, st, p.d_q, D, p.P, p.cb, p.d_sign, p.d_lut,
                           p.d_total);
        LY_HIP(hipGetLastError());
        // the scan: QB = 4 queries share a code load when the batch has them; tables in <= 64 KiB of LDS, whole column groups
        const int qb = nqc >= 4 ? 4 : 1;
        const uint32_t mc = p.cb < 16 ? p.cb : std::min<uint32_t>(p.cb, 64u / (uint32_t)qb);
        RbqScanArgs sa{reinterpret_cast<const uint4*>(p.codes), p.norms, n, p.cb, p.ng, mc, (float)p.P, p.d_lut, p.d_total, nqc,
                       asc ? 1 : 0, p.cut.d_S};
        const dim3 sgrid((uint32_t)((n + RBQ_NT * RBQ_R - 1) / (RBQ_NT * RBQ_R)), (nqc + qb - 1) / qb);
        const size_t slds = (size_t)qb * mc * 256 * 4;
        if (qb == 4) hipLaunchKernelGGL(k_rbq_scan<4>, sgrid, dim3(RBQ_NT), slds, st, sa);
        else hipLaunchKernelGGL(k_rbq_scan<1>, sgrid, dim3(RBQ_NT), slds, st, sa);
        LY_HIP(hipGetLastError());
        LY_TRY(p.cut.run(nqc, n, N, p.rr, h->num_cu, st));
        LY_TRY(rr.run(p.d_q, nqc, out_rows + q0 * k, out_dists + q0 * k, out_counts + q0, nullptr, st));
    }
    if (rr.timed) { p.searches += 1; p.scan_us += rr.pool_us; p.rescore_us += rr.rerank_us; }
    return LYNSE_OK;
}
