// polarvec_host.inc — FLAT-{IP,L2,COS}-POLARVEC<b> on a FLAT handle (PolarVecIndex, src/storage/polarvec_mmap.rs; Collection,
// src/engine.rs:2559-2567, :4593-4602, :5514-5515).  Included at the end of lynse_hip.hip after rabitq_host.inc, whose sign words, code
// layout helpers and handle checks it shares; kernels in polarvec.h, the pool cut is ScoreCut and the exact rescore PoolRerank
// (rerank_host.inc).  DESIGN.md §23.

// The index and the per-handle search scratch.  Codes cover the first n rows of the handle: rows appended after a build or a load
// stay outside the index.
struct PlvState {
    uint32_t P = 0, bits = 0, cb = 0, ng = 0;   // padded_dim, bits per dimension, code bytes, 16-byte column groups of the device layout
    uint64_t n = 0;
    std::vector<uint64_t> sign;                 // ceil(P / 64) sign words
    uint64_t* d_sign = nullptr;
    float *dim_mins = nullptr, *dim_scales = nullptr;   // [P]
    uint32_t* codes = nullptr;                  // device layout (rbq_word_index): ceil(n / 64) * ng * 64 uint4
    float *residual_sq = nullptr, *inv_norms = nullptr;   // [n]; the first only when built for L2, the second only for cosine
    float *d_q = nullptr, *d_lut = nullptr;
    size_t q_cap = 0, lut_cap = 0;
    ScoreCut cut;
    PoolRerank rr;
    double searches = 0.0, scan_us = 0.0, rescore_us = 0.0;

    void free_index() {
        for (void* p : {(void*)d_sign, (void*)dim_mins, (void*)dim_scales, (void*)codes, (void*)residual_sq, (void*)inv_norms})
            if (p) (void)hipFree(p);
        d_sign = nullptr;
        dim_mins = dim_scales = residual_sq = inv_norms = nullptr;
        codes = nullptr;
        sign.clear();
        P = bits = cb = ng = 0;
        n = 0;
    }
    ~PlvState() {
        free_index();
        for (void* p : {(void*)d_q, (void*)d_lut})
            if (p) (void)hipFree(p);
        cut.release();
        rr.release();
    }
};

static void plv_release(lynse_hip_flat* h) {
    delete h->plv;
    h->plv = nullptr;
}

static int plv_check_handle(const lynse_hip_flat* h) {
    if (h->dtype != LYNSE_DTYPE_F32) return set_error(LYNSE_ERR_UNSUPPORTED, "PolarVec on an F16 shard is not supported");
    if (h->packed_only) return set_error(LYNSE_ERR_UNSUPPORTED, "PolarVec is defined for float rows (ip / l2 / cosine)");
    if (h->row_stride != 1 || h->row_offset != 0) return set_error(LYNSE_ERR_UNSUPPORTED, "a PolarVec index is not row-sharded");
    if (h->dim > (1u << 30) || (size_t)rbq_next_pow2(h->dim) * 4 > PoolRerank::LDS_MAX)
        return set_error(LYNSE_ERR_UNSUPPORTED, "PolarVec: the padded vector does not fit in LDS");
    return LYNSE_OK;
}
static int plv_check_metric(int metric) {
    LY_TRY(metric_check(metric));
    if (metric != M_IP && metric != M_L2 && metric != M_COS) return set_error(LYNSE_ERR_UNSUPPORTED, "PolarVec is defined for ip / l2 / cosine");
    return LYNSE_OK;
}

// the rotation kernels keep rb * P floats in LDS: past 64 KiB the limit is raised once per kernel
static int plv_rotation_lds(size_t bytes) {
    if (bytes <= 64u * 1024u) return LYNSE_OK;
    LY_TRY(ensure_lds<k_plv_minmax>(PoolRerank::LDS_MAX));
    LY_TRY(ensure_lds<k_plv_encode>(PoolRerank::LDS_MAX));
    return ensure_lds<k_plv_query>(PoolRerank::LDS_MAX);
}

// a fresh index of n rows in `out` (device buffers allocated, the codes zeroed, the sign words uploaded)
static int plv_alloc(PlvState& out, uint32_t dim, uint32_t bits, uint64_t n, const uint64_t* sign_words, uint32_t n_sign_words,
                     bool residual, bool inv_norms) {
    out.P = rbq_next_pow2(dim);
    out.bits = bits;
    out.cb = (uint32_t)(((uint64_t)out.P * bits + 7) / 8);
    out.ng = ((out.cb + 3) / 4 + 3) / 4;
    out.n = n;
    const uint32_t nw = (out.P + 63) / 64;
    out.sign.assign(nw, 0ull);   // a word the caller does not hold negates nothing (apply_signs: sign_words.get(word_idx).unwrap_or(0))
    for (uint32_t w = 0; w < nw && w < n_sign_words; ++w) out.sign[w] = sign_words[w];
    LY_HIP(hipMalloc(&out.d_sign, (size_t)nw * 8));
    LY_HIP(hipMalloc(&out.dim_mins, (size_t)out.P * 4));
    LY_HIP(hipMalloc(&out.dim_scales, (size_t)out.P * 4));
    LY_HIP(hipMalloc(&out.codes, rbq_code_words(n, out.ng) * 4));
    if (residual) LY_HIP(hipMalloc(&out.residual_sq, (size_t)n * 4));
    if (inv_norms) LY_HIP(hipMalloc(&out.inv_norms, (size_t)n * 4));
    LY_TRY(h2d_done(out.d_sign, out.sign.data(), (size_t)nw * 8));
    LY_TRY(memset_done(out.codes, 0, rbq_code_words(n, out.ng) * 4));
    return LYNSE_OK;
}

// install `fresh` as the handle's index, keeping the search scratch
static void plv_install(lynse_hip_flat* h, PlvState& fresh) {
    if (!h->plv) h->plv = new PlvState();
    PlvState& r = *h->plv;
    r.free_index();
    r.P = fresh.P; r.bits = fresh.bits; r.cb = fresh.cb; r.ng = fresh.ng; r.n = fresh.n;
    r.sign.swap(fresh.sign);
    r.d_sign = fresh.d_sign; r.dim_mins = fresh.dim_mins; r.dim_scales = fresh.dim_scales; r.codes = fresh.codes;
    r.residual_sq = fresh.residual_sq; r.inv_norms = fresh.inv_norms;
    fresh.d_sign = nullptr; fresh.dim_mins = fresh.dim_scales = fresh.residual_sq = fresh.inv_norms = nullptr; fresh.codes = nullptr;
}

// PolarVecIndex::build_for_metric (polarvec_mmap.rs:118-264) over the handle's rows
extern "C" int lynse_hip_flat_build_polarvec(lynse_hip_flat* h, uint32_t bits, int metric) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    LY_TRY(plv_check_metric(metric));
    if (bits < 1 || bits > 8) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "bits must be in [1, 8]");
    LY_WRITER(h, lk);
    LY_TRY(use_device(h));
    LY_TRY(plv_check_handle(h));
    const uint64_t n = h->n;
    if (n == 0) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "need at least one vector");
    if (n > 0xffffffffull) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "a PolarVec index holds at most 2^32 - 1 rows");
    const uint32_t nw = (rbq_next_pow2(h->dim) + 63) / 64;
    std::vector<uint64_t> sign(nw);
    LY_TRY(lynse_hip_rabitq_sign_words(42, nw, sign.data()));
    PlvState fresh;   // (freed on every failing path)
    LY_TRY(plv_alloc(fresh, h->dim, bits, n, sign.data(), nw, metric == M_L2, metric == M_COS));
    const uint32_t P = fresh.P;
    const uint32_t rb = std::max<uint32_t>(1, std::min<uint32_t>(8, 4096u / P));
    const size_t lds = (size_t)rb * P * 4;
    LY_TRY(plv_rotation_lds(lds));
    hipStream_t st = cur(h).stream;
    // the fit: up to 50,000 sample rows at a fixed stride; the partials of all blocks stay at or under 16 MiB
    const uint64_t n_sample = std::min<uint64_t>(n, 50000), stride = n <= 50000 ? 1 : n / n_sample;
    const uint64_t groups = (n_sample + rb - 1) / rb;
    const uint64_t max_blocks = std::max<uint64_t>(64, (2ull << 20) / P);
    const uint64_t per = (groups + max_blocks - 1) / max_blocks * rb;
    const uint32_t blocks = (uint32_t)((n_sample + per - 1) / per);
    float* part = nullptr;
    LY_HIP(hipMalloc(&part, (size_t)blocks * P * 8));
    PlvMinmaxArgs ma{h->rows, h->ld, h->dim, P, n_sample, stride, per, rb, fresh.d_sign, part, part + (size_t)blocks * P};
    hipLaunchKernelGGL(k_plv_minmax, dim3(blocks), dim3(PLV_FIT_NT), lds, st, ma);
    hipLaunchKernelGGL(k_plv_fit, dim3((P + PLV_FIT_NT - 1) / PLV_FIT_NT), dim3(PLV_FIT_NT), 0, st, part, part + (size_t)blocks * P, blocks, P,
                       (float)((1u << bits) - 1u), fresh.dim_mins, fresh.dim_scales);
    PlvEncodeArgs ea{h->rows, h->ld, h->dim, P, bits, n, rb, fresh.ng, fresh.d_sign, fresh.dim_mins, fresh.dim_scales,
                     fresh.codes, fresh.residual_sq, fresh.inv_norms};
    hipLaunchKernelGGL(k_plv_encode, dim3((uint32_t)((n + rb - 1) / rb)), dim3(RBQ_ENC_NT), lds, st, ea);
    const hipError_t launched = hipGetLastError(), done = hipStreamSynchronize(st);
    (void)hipFree(part);
    LY_HIP(launched);
    LY_HIP(done);
    plv_install(h, fresh);
    return LYNSE_OK;
}

// PolarVecIndex::load's in-memory half: the arrays as polarvec_index.bin (version 5) holds them; a NULL correction array is absent
extern "C" int lynse_hip_flat_load_polarvec(lynse_hip_flat* h, uint32_t dim, uint32_t bits, const uint64_t* sign_words, uint32_t n_sign_words,
                                            const float* dim_mins, const float* dim_scales, const uint8_t* codes, const float* residual_sq,
                                            const float* inv_v_hat_norms, uint64_t n) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    LY_WRITER(h, lk);
    LY_TRY(use_device(h));
    LY_TRY(plv_check_handle(h));
    if (dim == 0 || dim != h->dim) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "Invalid PolarVec index dimensions");
    if (bits < 1 || bits > 8) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "bits must be in [1, 8]");
    if (n == 0) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "need at least one vector");
    if (n > 0xffffffffull) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "a PolarVec index holds at most 2^32 - 1 rows");
    if (n > h->n) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "the PolarVec index covers more rows than the handle holds");
    if (!codes || !dim_mins || !dim_scales || (n_sign_words && !sign_words)) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    PlvState fresh;
    LY_TRY(plv_alloc(fresh, dim, bits, n, sign_words, n_sign_words, residual_sq != nullptr, inv_v_hat_norms != nullptr));
    // [n][bytes_per_vec] -> the device layout, on the host
    std::vector<uint32_t> dev(rbq_code_words(n, fresh.ng), 0u);
    const uint32_t cb = fresh.cb;
    for (uint64_t r = 0; r < n; ++r)
        for (uint32_t b = 0; b < cb; ++b)
            dev[rbq_word_index(r, b >> 2, fresh.ng)] |= (uint32_t)codes[r * cb + b] << (8 * (b & 3u));
    LY_TRY(h2d_done(fresh.codes, dev.data(), dev.size() * 4));
    LY_TRY(h2d_done(fresh.dim_mins, dim_mins, (size_t)fresh.P * 4));
    LY_TRY(h2d_done(fresh.dim_scales, dim_scales, (size_t)fresh.P * 4));
    if (residual_sq) LY_TRY(h2d_done(fresh.residual_sq, residual_sq, (size_t)n * 4));
    if (inv_v_hat_norms) LY_TRY(h2d_done(fresh.inv_norms, inv_v_hat_norms, (size_t)n * 4));
    plv_install(h, fresh);
    return LYNSE_OK;
}

extern "C" int lynse_hip_flat_polarvec_params(lynse_hip_flat* h, uint32_t* dims, uint64_t* n_plv, uint64_t* sign_words, float* dim_mins,
                                              float* dim_scales, uint8_t* codes, float* residual_sq, float* inv_v_hat_norms) {
    if (!h || !dims || !n_plv) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    std::shared_lock<std::shared_mutex> lk(h->rw);
    if (!h->plv || !h->plv->codes) {
        dims[0] = dims[1] = dims[2] = dims[3] = dims[4] = 0;
        *n_plv = 0;
        return LYNSE_OK;
    }
    const PlvState& r = *h->plv;
    dims[0] = h->dim; dims[1] = r.P; dims[2] = r.bits; dims[3] = r.cb;
    dims[4] = (r.residual_sq ? 1u : 0u) | (r.inv_norms ? 2u : 0u);
    *n_plv = r.n;
    LY_TRY(use_device(h));
    if (sign_words) memcpy(sign_words, r.sign.data(), r.sign.size() * 8);
    if (dim_mins) LY_HIP(hipMemcpy(dim_mins, r.dim_mins, (size_t)r.P * 4, hipMemcpyDeviceToHost));
    if (dim_scales) LY_HIP(hipMemcpy(dim_scales, r.dim_scales, (size_t)r.P * 4, hipMemcpyDeviceToHost));
    if (codes) {
        std::vector<uint32_t> dev(rbq_code_words(r.n, r.ng));
        LY_HIP(hipMemcpy(dev.data(), r.codes, dev.size() * 4, hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < r.n; ++i)
            for (uint32_t b = 0; b < r.cb; ++b)
                codes[i * r.cb + b] = (uint8_t)(dev[rbq_word_index(i, b >> 2, r.ng)] >> (8 * (b & 3u)));
    }
    if (residual_sq && r.residual_sq) LY_HIP(hipMemcpy(residual_sq, r.residual_sq, (size_t)r.n * 4, hipMemcpyDeviceToHost));
    if (inv_v_hat_norms && r.inv_norms) LY_HIP(hipMemcpy(inv_v_hat_norms, r.inv_norms, (size_t)r.n * 4, hipMemcpyDeviceToHost));
    return LYNSE_OK;
}

extern "C" int lynse_hip_flat_drop_polarvec(lynse_hip_flat* h) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    LY_WRITER(h, lk);
    LY_TRY(use_device(h));
    if (h->plv) h->plv->free_index();
    return LYNSE_OK;
}

extern "C" int lynse_hip_flat_polarvec_stage_times(lynse_hip_flat* h, double* out3, int reset) {
    if (!h || !out3) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    LY_WRITER(h, lk);
    if (!h->plv) { out3[0] = out3[1] = out3[2] = 0.0; return LYNSE_OK; }
    out3[0] = h->plv->searches;
    out3[1] = h->plv->scan_us;
    out3[2] = h->plv->rescore_us;
    if (reset) h->plv->searches = h->plv->scan_us = h->plv->rescore_us = 0.0;
    return LYNSE_OK;
}

template <int CLS>
static void plv_launch_scan(int qb, dim3 grid, size_t lds, hipStream_t st, const PlvScanArgs& sa) {
    if (qb == 4) hipLaunchKernelGGL((k_plv_scan<CLS, 4>), grid, dim3(PLV_NT), lds, st, sa);
    else hipLaunchKernelGGL((k_plv_scan<CLS, 1>), grid, dim3(PLV_NT), lds, st, sa);
}

// PolarVecIndex::search_candidates + rescore_exact_with (polarvec_mmap.rs:285-371): k' = min(k, n_plv), N = min(k' * oversample, n_plv)
// rows by the canonical (table score, row) key, rescored with compute_distance_f32 on the original rows, the best k' by (exact
// distance, row).  Queries go in chunks: score matrix <= 512 MiB, pool <= 256 MiB (ScoreCut::chunk), tables <= 256 MiB.
extern "C" int lynse_hip_flat_search_polarvec_f32(lynse_hip_flat* h, const float* queries, uint64_t nq, uint32_t k, int metric,
                                                  uint32_t oversample, uint64_t* out_rows, float* out_dists, uint32_t* out_counts) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    LY_TRY(plv_check_metric(metric));
    if (nq == 0) return LYNSE_OK;
    if (!queries || !out_counts || (k && (!out_rows || !out_dists))) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    LY_WRITER(h, lk);
    LY_TRY(use_device(h));
    LY_TRY(plv_check_handle(h));
    if (!h->plv || !h->plv->codes) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "no PolarVec index on this handle: build or load one first");
    PlvState& p = *h->plv;
    const uint64_t n = p.n;
    const uint32_t D = h->dim;
    if (k == 0) { memset(out_counts, 0, nq * 4); return LYNSE_OK; }
    const uint32_t kk = (uint32_t)std::min<uint64_t>(k, n);
    const uint32_t N = (uint32_t)std::min<uint64_t>((uint64_t)kk * oversample, n);
    if (N == 0) { memset(out_counts, 0, nq * 4); return LYNSE_OK; }
    const bool asc = metric_ascending(metric);
    const size_t lut_q = (size_t)p.P << p.bits;   // floats of one query's table
    const uint64_t qc = std::max<uint64_t>(1, std::min<uint64_t>(ScoreCut::chunk(nq, n, N), (256ull << 20) / (lut_q * 4)));
    PoolRerank::Search rr(p.rr);
    rr.split_small = true;   // a pool is 20 k rows: a single query's would be gathered by one CU
    LY_TRY(rr.begin(h->rows, n, h->ld, D, metric, N, kk, k, qc, false, h->profiling.load(), "PolarVec rescore"));
    LY_TRY(ivf_grow(&p.d_q, &p.q_cap, (size_t)qc * D));
    LY_TRY(ivf_grow(&p.d_lut, &p.lut_cap, (size_t)qc * lut_q));
    LY_TRY(p.cut.grow(qc, n));
    LY_TRY(plv_rotation_lds((size_t)p.P * 4));
    // the scan's class and its unit: bytes of code and table entries (polarvec.h)
    const int cls = p.bits == 8 ? PLV_BYTE : (p.bits == 4 ? PLV_B4 : (p.bits == 3 ? PLV_B3 : PLV_GEN));
    const uint32_t ub = cls == PLV_B3 ? 48u : (cls == PLV_GEN ? 16u * p.bits : 16u);
    const uint32_t ue = cls == PLV_BYTE ? 4096u : (cls == PLV_B4 ? 512u : (128u << p.bits));
    const uint32_t units = (p.cb + ub - 1) / ub;
    hipStream_t st = cur(h).stream;
    for (uint64_t q0 = 0; q0 < nq; q0 += qc) {
        const uint32_t nqc = (uint32_t)std::min<uint64_t>(qc, nq - q0);
        LY_HIP(hipMemcpyAsync(p.d_q, queries + q0 * D, (size_t)nqc * D * 4, hipMemcpyHostToDevice, st));
        LY_TRY(rr.pool_start(st));
        // a small batch spreads each query's table over up to 16 workgroups
        const uint32_t parts = nqc >= 32 ? 1u : (uint32_t)std::max<size_t>(1, std::min<size_t>(16, lut_q / 4096));
        hipLaunchKernelGGL(k_plv_query, dim3(nqc, parts), dim3(RBQ_Q_NT), (size_t)p.P * 4, st, p.d_q, D, p.P, p.bits, metric, p.d_sign,
                           p.dim_mins, p.dim_scales, p.d_lut);
        LY_HIP(hipGetLastError());
        // the scan: QB = 4 queries share a code load when the batch has them and four unit tables fit 64 KiB of LDS
        const int qb = nqc >= 4 && (size_t)ue * 16 <= 64u * 1024u ? 4 : 1;
        const uint32_t cu = std::max<uint32_t>(1, std::min<uint32_t>(units, (64u * 1024u) / (ue * 4u * (uint32_t)qb)));
        PlvScanArgs sa{reinterpret_cast<const uint4*>(p.codes), n, p.P, p.bits, p.cb, p.ng, cu, ub, ue, p.d_lut, nqc, asc ? 1 : 0,
                       metric == M_L2 ? p.residual_sq : nullptr, metric == M_COS ? p.inv_norms : nullptr, p.cut.d_S};
        const dim3 sgrid((uint32_t)((n + PLV_NT * PLV_R - 1) / (PLV_NT * PLV_R)), (nqc + qb - 1) / qb);
        const size_t slds = (size_t)qb * cu * ue * 4;
        switch (cls) {
        case PLV_BYTE: plv_launch_scan<PLV_BYTE>(qb, sgrid, slds, st, sa); break;
        case PLV_B4: plv_launch_scan<PLV_B4>(qb, sgrid, slds, st, sa); break;
        case PLV_B3: plv_launch_scan<PLV_B3>(qb, sgrid, slds, st, sa); break;
        default: plv_launch_scan<PLV_GEN>(qb, sgrid, slds, st, sa); break;
        }
        LY_HIP(hipGetLastError());
        LY_TRY(p.cut.run(nqc, n, N, p.rr, h->num_cu, st));
        LY_TRY(rr.run(p.d_q, nqc, out_rows + q0 * k, out_dists + q0 * k, out_counts + q0, nullptr, st));
    }
    if (rr.timed) { p.searches += 1; p.scan_us += rr.pool_us; p.rescore_us += rr.rerank_us; }
    return LYNSE_OK;
}
