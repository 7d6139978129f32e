// coded_host.inc — the host frame of the two-pass searches over auxiliary codes on a FLAT handle: FLAT-*-PQ (pq_host.inc),
// FLAT-*-RABITQ (rabitq_host.inc) and FLAT-*-POLARVEC<b> (polarvec_host.inc).  Each scores its codes into a score matrix, ScoreCut cuts
// the matrix to a pool and PoolRerank rescores the pool exactly (rerank_host.inc); what surrounds the codec's own kernels is here, once:
// the owning device pointer, the per-handle search scratch, the search driver, the rotated-code container of RaBitQ and PolarVec, the
// handle checks and the small per-index entry bodies.  Included at the end of lynse_hip.hip, before the three.  DESIGN.md §12, §15, §23.

// An owning device pointer: freed on every exit path unless release() hands it over.
template <typename T>
struct DevBuf {
    T* p = nullptr;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.release()) {}
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (p) (void)hipFree(p);
        p = o.release();
        return *this;
    }
    int alloc(size_t count) {
        LY_HIP(hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T)));
        return LYNSE_OK;
    }
    T* release() {
        T* q = p;
        p = nullptr;
        return q;
    }
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
};

// The search scratch a handle keeps per coded index (its searches are serialised): it outlives the index it serves, so a rebuild or
// a load keeps the buffers.
struct CodedScratch {
    float *d_q = nullptr, *d_lut = nullptr, *d_extra = nullptr;   // a chunk's queries, their tables, one more float per query (RaBitQ's total_q)
    size_t q_cap = 0, lut_cap = 0, extra_cap = 0;
    ScoreCut cut;    // the [chunk][n] score matrix and its radix selection
    PoolRerank rr;   // the pool's rows and counts, the rescore's buffers and timing events
    double searches = 0.0, scan_us = 0.0, rescore_us = 0.0;
    CodedScratch() = default;
    CodedScratch(const CodedScratch&) = delete;
    CodedScratch& operator=(const CodedScratch&) = delete;
    ~CodedScratch() {
        for (void* p : {(void*)d_q, (void*)d_lut, (void*)d_extra})
            if (p) (void)hipFree(p);
        cut.release();
        rr.release();
    }
    void stage_times(double* out3, int reset) {
        out3[0] = searches;
        out3[1] = scan_us;
        out3[2] = rescore_us;
        if (reset) searches = scan_us = rescore_us = 0.0;
    }
};

// ---- the per-index entry bodies: State = {Index ix; CodedScratch s;}, held by the handle through a pointer that is NULL until the
// first build or load ------------------------------------------------------------------------------------------------------------
// install `fresh` as the handle's index, keeping the search scratch
template <typename State, typename Index>
static void coded_install(State*& slot, Index& fresh) {
    if (!slot) slot = new State();
    slot->ix = std::move(fresh);
}

template <typename State>
static int coded_drop(lynse_hip_flat* h, State* lynse_hip_flat::*slot) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    LY_WRITER(h, lk);
    LY_TRY(use_device(h));
    if (h->*slot) (h->*slot)->ix = {};
    return LYNSE_OK;
}

template <typename State>
static int coded_stage_times(State* st, double* out3, int reset) {   // (the writer lock held) an absent index reports zeros
    if (st) st->s.stage_times(out3, reset);
    else out3[0] = out3[1] = out3[2] = 0.0;
    return LYNSE_OK;
}

// what a handle must be to carry a coded index; RaBitQ and PolarVec also keep a padded vector in LDS
static inline uint32_t rbq_next_pow2(uint32_t d) {
    uint32_t p = 1;
    while (p < d) p <<= 1;
    return p;
}
static int coded_check_handle(const lynse_hip_flat* h, const char* who, bool needs_padded_lds) {
    const auto refuse = [who](const char* before, const char* after) { return set_error(LYNSE_ERR_UNSUPPORTED, std::string(before) + who + after); };
    if (h->dtype != LYNSE_DTYPE_F32) return refuse("", " on an F16 shard is not supported");
    if (h->packed_only) return refuse("", " is defined for float rows (ip / l2 / cosine)");
    if (h->row_stride != 1 || h->row_offset != 0) return refuse("a ", " index is not row-sharded");
    if (needs_padded_lds && (h->dim > (1u << 30) || (size_t)rbq_next_pow2(h->dim) * 4 > PoolRerank::LDS_MAX))
        return refuse("", ": the padded vector does not fit in LDS");
    return LYNSE_OK;
}

// ---- the rotated codes of RaBitQ (1 bit per dimension) and PolarVec (`bits`): the dimension padded to a power of two, the sign words
// of the rotation on both sides, the codes in the device layout of rbq_word_index (rabitq.h) --------------------------------------
struct RotCodes {
    uint32_t P = 0, cb = 0, ng = 0;   // padded_dim, code bytes, 16-byte column groups of the device layout
    uint64_t n = 0;
    std::vector<uint64_t> sign;       // ceil(P / 64) sign words
    DevBuf<uint64_t> d_sign;
    DevBuf<uint32_t> codes;           // ceil(n / 64) * ng * 64 uint4
    size_t words() const { return (size_t)((n + 63) / 64) * ng * 64 * 4; }

    // a fresh index of n rows: device buffers allocated, the codes zeroed, the sign words uploaded
    int alloc(uint32_t dim, uint32_t bits, uint64_t n_rows, const uint64_t* sign_words, uint32_t n_sign_words) {
        P = rbq_next_pow2(dim);
        cb = (uint32_t)(((uint64_t)P * bits + 7) / 8);
        ng = ((cb + 3) / 4 + 3) / 4;
        n = n_rows;
        const uint32_t nw = (P + 63) / 64;
        sign.assign(nw, 0ull);   // a word the caller does not hold negates nothing (apply_signs: word_idx < sign_words.len())
        for (uint32_t w = 0; w < nw && w < n_sign_words; ++w) sign[w] = sign_words[w];
        LY_TRY(d_sign.alloc(nw));
        LY_TRY(codes.alloc(words()));
        LY_TRY(h2d_done(d_sign.p, sign.data(), (size_t)nw * 8));
        return memset_done(codes.p, 0, words() * 4);
    }
    // host_codes [n][cb], as the index files hold them, <-> the device layout; the conversion runs on the host
    int upload(const uint8_t* host_codes) {
        std::vector<uint32_t> dev(words(), 0u);
        for (uint64_t r = 0; r < n; ++r)
            for (uint32_t b = 0; b < cb; ++b) dev[rbq_word_index(r, b >> 2, ng)] |= (uint32_t)host_codes[r * cb + b] << (8 * (b & 3u));
        return h2d_done(codes.p, dev.data(), dev.size() * 4);
    }
    int download(uint8_t* host_codes) const {
        std::vector<uint32_t> dev(words());
        LY_HIP(hipMemcpy(dev.data(), codes.p, dev.size() * 4, hipMemcpyDeviceToHost));
        for (uint64_t r = 0; r < n; ++r)
            for (uint32_t b = 0; b < cb; ++b) host_codes[r * cb + b] = (uint8_t)(dev[rbq_word_index(r, b >> 2, ng)] >> (8 * (b & 3u)));
        return LYNSE_OK;
    }
};

// ---- the search ------------------------------------------------------------------------------------------------------------------
// What a codec tells the driver about its index: the rows it covers, its name in messages, the floats of one query's table(s), whether
// a chunk's tables are capped at 256 MiB, whether a small batch's pools are scored by several workgroups each (PoolRerank's
// split_small), whether the kernels want CodedScratch::d_extra.
struct CodedShape {
    const char* who;
    uint64_t n;
    size_t lut_q;
    bool cap_tables, split_small, extra;
};

// search_candidates + rescore_exact of the three indexes: k' = min(k, n), N = min(k' * oversample, n) rows by the canonical (code
// score, row) key, rescored with compute_distance_f32 on the original rows, the best k' by (exact distance, row).  Queries go in
// chunks: score matrix <= 512 MiB, pool <= 256 MiB (ScoreCut::chunk) and, where capped, tables <= 256 MiB.  score(st, nqc, asc)
// launches the codec's table and scan kernels for the nqc queries in s.d_q and leaves the score images in s.cut.d_S.  The caller
// holds the writer lock and has checked its arguments, the handle and the index.
template <typename Score>
static int coded_search(lynse_hip_flat* h, CodedScratch& s, const CodedShape& c, const float* queries, uint64_t nq, uint32_t k, int metric,
                        uint32_t oversample, uint64_t* out_rows, float* out_dists, uint32_t* out_counts, Score score) {
    const uint64_t n = c.n;
    const uint32_t D = h->dim;
    const uint32_t kk = (uint32_t)std::min<uint64_t>(k, n);
    const uint32_t N = (uint32_t)std::min<uint64_t>((uint64_t)kk * oversample, n);
    if (N == 0) { memset(out_counts, 0, nq * 4); return LYNSE_OK; }   // (k == 0 among them)
    const bool asc = metric_ascending(metric);
    uint64_t qc = ScoreCut::chunk(nq, n, N);
    if (c.cap_tables) qc = std::max<uint64_t>(1, std::min<uint64_t>(qc, (256ull << 20) / (c.lut_q * 4)));
    PoolRerank::Search rr(s.rr);
    rr.split_small = c.split_small;   // pools of thousands of rows: a single query's would be gathered by one CU
    LY_TRY(rr.begin(h->rows, n, h->ld, D, metric, N, kk, k, qc, false, h->profiling.load(), (std::string(c.who) + " rescore").c_str()));
    LY_TRY(ivf_grow(&s.d_q, &s.q_cap, (size_t)qc * D));
    LY_TRY(ivf_grow(&s.d_lut, &s.lut_cap, (size_t)qc * c.lut_q));
    if (c.extra) LY_TRY(ivf_grow(&s.d_extra, &s.extra_cap, (size_t)qc));
    LY_TRY(s.cut.grow(qc, n));
    hipStream_t st = cur(h).stream;
    for (uint64_t q0 = 0; q0 < nq; q0 += qc) {
        const uint32_t nqc = (uint32_t)std::min<uint64_t>(qc, nq - q0);
        LY_HIP(hipMemcpyAsync(s.d_q, queries + q0 * D, (size_t)nqc * D * 4, hipMemcpyHostToDevice, st));
        LY_TRY(rr.pool_start(st));
        LY_TRY(score(st, nqc, asc));
        LY_TRY(s.cut.run(nqc, n, N, s.rr, h->num_cu, st));   // the N best (score, row) keys -> pool rows
        LY_TRY(rr.run(s.d_q, nqc, out_rows + q0 * k, out_dists + q0 * k, out_counts + q0, nullptr, st));
    }
    if (rr.timed) { s.searches += 1; s.scan_us += rr.pool_us; s.rescore_us += rr.rerank_us; }
    return LYNSE_OK;
}
