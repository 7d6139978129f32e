// polarvec_host.inc — FLAT-{IP,L2,COS}-POLARVEC<b> on a FLAT handle (PolarVecIndex, src/storage/polarvec_mmap.rs; Collection,
// src/engine.rs:2559-2567, :4593-4602, :5514-5515): the grid fit and encode launches, the table and scan launches with their scan-class
// arithmetic.  Included at the end of lynse_hip.hip after coded_host.inc, which holds the frame it shares with PQ and RaBitQ (RotCodes,
// CodedScratch, the handle check, the search driver around ScoreCut and PoolRerank), and after rabitq_host.inc, whose sign words it
// draws; kernels in polarvec.h.  The last of the three: coded_release is at its end.  DESIGN.md §23.

// The index: b-bit codes of the first n rows of the handle on a per-dimension grid.  Rows appended after a build or a load stay outside it.
struct PlvIndex : RotCodes {
    uint32_t bits = 0;                       // per dimension
    DevBuf<float> dim_mins, dim_scales;      // [P]
    DevBuf<float> residual_sq, inv_norms;    // [n]; the first only when built for L2, the second only for cosine
};
struct PlvState {
    PlvIndex ix;
    CodedScratch s;   // (coded_host.inc)
};

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

static int plv_alloc(PlvIndex& out, uint32_t dim, uint32_t bits, uint64_t n, const uint64_t* sign_words, uint32_t n_sign_words, bool residual,
                     bool inv_norms) {
    LY_TRY(out.alloc(dim, bits, n, sign_words, n_sign_words));
    out.bits = bits;
    LY_TRY(out.dim_mins.alloc(out.P));
    LY_TRY(out.dim_scales.alloc(out.P));
    if (residual) LY_TRY(out.residual_sq.alloc(n));
    if (inv_norms) LY_TRY(out.inv_norms.alloc(n));
    return LYNSE_OK;
}

// PolarVecIndex::build_for_metric (polarvec_mmap.rs:118-264) over the handle's rows
extern "C" int lynse_hip_flat_build_polarvec(lynse_hip_flat* h, uint32_t bits, int metric) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    LY_TRY(plv_check_metric(metric));
    if (bits < 1 || bits > 8) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "bits must be in [1, 8]");
    LY_WRITER(h, lk);
    LY_TRY(use_device(h));
    LY_TRY(coded_check_handle(h, "PolarVec", true));
    const uint64_t n = h->n;
    if (n == 0) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "need at least one vector");
    if (n > 0xffffffffull) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "a PolarVec index holds at most 2^32 - 1 rows");
    const uint32_t nw = (rbq_next_pow2(h->dim) + 63) / 64;
    std::vector<uint64_t> sign(nw);
    LY_TRY(lynse_hip_rabitq_sign_words(42, nw, sign.data()));
    PlvIndex fresh;   // (freed on every failing path)
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
    DevBuf<float> part;
    LY_TRY(part.alloc((size_t)blocks * P * 2));
    PlvMinmaxArgs ma{h->rows, h->ld, h->dim, P, n_sample, stride, per, rb, fresh.d_sign.p, part.p, part.p + (size_t)blocks * P};
    hipLaunchKernelGGL(k_plv_minmax, dim3(blocks), dim3(PLV_FIT_NT), lds, st, ma);
    hipLaunchKernelGGL(k_plv_fit, dim3((P + PLV_FIT_NT - 1) / PLV_FIT_NT), dim3(PLV_FIT_NT), 0, st, part.p, part.p + (size_t)blocks * P, blocks, P,
                       (float)((1u << bits) - 1u), fresh.dim_mins.p, fresh.dim_scales.p);
    PlvEncodeArgs ea{h->rows, h->ld, h->dim, P, bits, n, rb, fresh.ng, fresh.d_sign.p, fresh.dim_mins.p, fresh.dim_scales.p,
                     fresh.codes.p, fresh.residual_sq.p, fresh.inv_norms.p};
    hipLaunchKernelGGL(k_plv_encode, dim3((uint32_t)((n + rb - 1) / rb)), dim3(RBQ_ENC_NT), lds, st, ea);
    const hipError_t launched = hipGetLastError(), done = hipStreamSynchronize(st);   // (the stream drained before any buffer goes)
    LY_HIP(launched);
    LY_HIP(done);
    coded_install(h->plv, fresh);
    return LYNSE_OK;
}

// PolarVecIndex::load's in-memory half: the arrays as polarvec_index.bin (version 5) holds them; a NULL correction array is absent
extern "C" int lynse_hip_flat_load_polarvec(lynse_hip_flat* h, uint32_t dim, uint32_t bits, const uint64_t* sign_words, uint32_t n_sign_words,
                                            const float* dim_mins, const float* dim_scales, const uint8_t* codes, const float* residual_sq,
                                            const float* inv_v_hat_norms, uint64_t n) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    LY_WRITER(h, lk);
    LY_TRY(use_device(h));
    LY_TRY(coded_check_handle(h, "PolarVec", true));
    if (dim == 0 || dim != h->dim) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "Invalid PolarVec index dimensions");
    if (bits < 1 || bits > 8) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "bits must be in [1, 8]");
    if (n == 0) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "need at least one vector");
    if (n > 0xffffffffull) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "a PolarVec index holds at most 2^32 - 1 rows");
    if (n > h->n) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "the PolarVec index covers more rows than the handle holds");
    if (!codes || !dim_mins || !dim_scales || (n_sign_words && !sign_words)) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    PlvIndex fresh;
    LY_TRY(plv_alloc(fresh, dim, bits, n, sign_words, n_sign_words, residual_sq != nullptr, inv_v_hat_norms != nullptr));
    LY_TRY(fresh.upload(codes));
    LY_TRY(h2d_done(fresh.dim_mins.p, dim_mins, (size_t)fresh.P * 4));
    LY_TRY(h2d_done(fresh.dim_scales.p, dim_scales, (size_t)fresh.P * 4));
    if (residual_sq) LY_TRY(h2d_done(fresh.residual_sq.p, residual_sq, (size_t)n * 4));
    if (inv_v_hat_norms) LY_TRY(h2d_done(fresh.inv_norms.p, inv_v_hat_norms, (size_t)n * 4));
    coded_install(h->plv, fresh);
    return LYNSE_OK;
}

extern "C" int lynse_hip_flat_polarvec_params(lynse_hip_flat* h, uint32_t* dims, uint64_t* n_plv, uint64_t* sign_words, float* dim_mins,
                                              float* dim_scales, uint8_t* codes, float* residual_sq, float* inv_v_hat_norms) {
    if (!h || !dims || !n_plv) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    std::shared_lock<std::shared_mutex> lk(h->rw);
    if (!h->plv || !h->plv->ix.codes.p) {
        dims[0] = dims[1] = dims[2] = dims[3] = dims[4] = 0;
        *n_plv = 0;
        return LYNSE_OK;
    }
    const PlvIndex& r = h->plv->ix;
    dims[0] = h->dim; dims[1] = r.P; dims[2] = r.bits; dims[3] = r.cb;
    dims[4] = (r.residual_sq.p ? 1u : 0u) | (r.inv_norms.p ? 2u : 0u);
    *n_plv = r.n;
    LY_TRY(use_device(h));
    if (sign_words) memcpy(sign_words, r.sign.data(), r.sign.size() * 8);
    if (dim_mins) LY_HIP(hipMemcpy(dim_mins, r.dim_mins.p, (size_t)r.P * 4, hipMemcpyDeviceToHost));
    if (dim_scales) LY_HIP(hipMemcpy(dim_scales, r.dim_scales.p, (size_t)r.P * 4, hipMemcpyDeviceToHost));
    if (codes) LY_TRY(r.download(codes));
    if (residual_sq && r.residual_sq.p) LY_HIP(hipMemcpy(residual_sq, r.residual_sq.p, (size_t)r.n * 4, hipMemcpyDeviceToHost));
    if (inv_v_hat_norms && r.inv_norms.p) LY_HIP(hipMemcpy(inv_v_hat_norms, r.inv_norms.p, (size_t)r.n * 4, hipMemcpyDeviceToHost));
    return LYNSE_OK;
}

extern "C" int lynse_hip_flat_drop_polarvec(lynse_hip_flat* h) { return coded_drop(h, &lynse_hip_flat::plv); }

extern "C" int lynse_hip_flat_polarvec_stage_times(lynse_hip_flat* h, double* out3, int reset) {
    if (!h || !out3) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    LY_WRITER(h, lk);
    return coded_stage_times(h->plv, out3, reset);
}

template <int CLS>
static void plv_launch_scan(int qb, dim3 grid, size_t lds, hipStream_t st, const PlvScanArgs& sa) {
    if (qb == 4) hipLaunchKernelGGL((k_plv_scan<CLS, 4>), grid, dim3(PLV_NT), lds, st, sa);
    else hipLaunchKernelGGL((k_plv_scan<CLS, 1>), grid, dim3(PLV_NT), lds, st, sa);
}

// PolarVecIndex::search_candidates + rescore_exact_with (polarvec_mmap.rs:285-371) through coded_search, by the table score; a chunk's
// tables stay at or under 256 MiB, and a pool is 20 k rows, so a small batch's rescore is split.
extern "C" int lynse_hip_flat_search_polarvec_f32(lynse_hip_flat* h, const float* queries, uint64_t nq, uint32_t k, int metric,
                                                  uint32_t oversample, uint64_t* out_rows, float* out_dists, uint32_t* out_counts) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    LY_TRY(plv_check_metric(metric));
    if (nq == 0) return LYNSE_OK;
    if (!queries || !out_counts || (k && (!out_rows || !out_dists))) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    LY_WRITER(h, lk);
    LY_TRY(use_device(h));
    LY_TRY(coded_check_handle(h, "PolarVec", true));
    if (!h->plv || !h->plv->ix.codes.p) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "no PolarVec index on this handle: build or load one first");
    const PlvIndex& p = h->plv->ix;
    CodedScratch& s = h->plv->s;
    LY_TRY(plv_rotation_lds((size_t)p.P * 4));
    const size_t lut_q = (size_t)p.P << p.bits;   // floats of one query's table
    // the scan's class and its unit: bytes of code and table entries (polarvec.h)
    const int cls = p.bits == 8 ? PLV_BYTE : (p.bits == 4 ? PLV_B4 : (p.bits == 3 ? PLV_B3 : PLV_GEN));
    const uint32_t ub = cls == PLV_B3 ? 48u : (cls == PLV_GEN ? 16u * p.bits : 16u);
    const uint32_t ue = cls == PLV_BYTE ? 4096u : (cls == PLV_B4 ? 512u : (128u << p.bits));
    const uint32_t units = (p.cb + ub - 1) / ub;
    const auto score = [&](hipStream_t st, uint32_t nqc, bool asc) -> int {
        // a small batch spreads each query's table over up to 16 workgroups
        const uint32_t parts = nqc >= 32 ? 1u : (uint32_t)std::max<size_t>(1, std::min<size_t>(16, lut_q / 4096));
        hipLaunchKernelGGL(k_plv_query, dim3(nqc, parts), dim3(RBQ_Q_NT), (size_t)p.P * 4, st, s.d_q, h->dim, p.P, p.bits, metric, p.d_sign.p,
                           p.dim_mins.p, p.dim_scales.p, s.d_lut);
        LY_HIP(hipGetLastError());
        // the scan: QB = 4 queries share a code load when the batch has them and four unit tables fit 64 KiB of LDS
        const int qb = nqc >= 4 && (size_t)ue * 16 <= 64u * 1024u ? 4 : 1;
        const uint32_t cu = std::max<uint32_t>(1, std::min<uint32_t>(units, (64u * 1024u) / (ue * 4u * (uint32_t)qb)));
        PlvScanArgs sa{reinterpret_cast<const uint4*>(p.codes.p), p.n, p.P, p.bits, p.cb, p.ng, cu, ub, ue, s.d_lut, nqc, asc ? 1 : 0,
                       metric == M_L2 ? p.residual_sq.p : nullptr, metric == M_COS ? p.inv_norms.p : nullptr, s.cut.d_S};
        const dim3 sgrid((uint32_t)((p.n + PLV_NT * PLV_R - 1) / (PLV_NT * PLV_R)), (nqc + qb - 1) / qb);
        const size_t slds = (size_t)qb * cu * ue * 4;
        switch (cls) {
        case PLV_BYTE: plv_launch_scan<PLV_BYTE>(qb, sgrid, slds, st, sa); break;
        case PLV_B4: plv_launch_scan<PLV_B4>(qb, sgrid, slds, st, sa); break;
        case PLV_B3: plv_launch_scan<PLV_B3>(qb, sgrid, slds, st, sa); break;
        default: plv_launch_scan<PLV_GEN>(qb, sgrid, slds, st, sa); break;
        }
        LY_HIP(hipGetLastError());
        return LYNSE_OK;
    };
    return coded_search(h, s, {"PolarVec", p.n, lut_q, true, true, false}, queries, nq, k, metric, oversample, out_rows, out_dists, out_counts,
                        score);
}

// every coded index and its scratch, for the handle's destructor and a row mutation (declared in lynse_hip.hip)
static void coded_release(lynse_hip_flat* h) {
    delete h->pq;
    delete h->rbq;
    delete h->plv;
    h->pq = nullptr;
    h->rbq = nullptr;
    h->plv = nullptr;
}
