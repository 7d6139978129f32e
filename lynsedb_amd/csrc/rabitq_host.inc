// rabitq_host.inc — FLAT-{IP,L2,COS}-RABITQ on a FLAT handle (RaBitQIndex, src/storage/rabitq_mmap.rs; Collection,
// src/engine.rs:4476, :4552, :5504-5526): the sign words, the encode launch, the byte-table and scan launches.  Included at the end of
// lynse_hip.hip after coded_host.inc, which holds the frame it shares with PQ and PolarVec (RotCodes, CodedScratch, the handle check,
// the search driver around ScoreCut and PoolRerank), and after pq_host.inc (the SmallRng restatement is pqrng); kernels in rabitq.h.
// DESIGN.md §15.

// The index: 1-bit codes and the norms of the first n rows of the handle.  Rows appended after a build or a load stay outside it.
struct RbqIndex : RotCodes {
    DevBuf<float> norms;   // [n]
};
struct RbqState {
    RbqIndex ix;
    CodedScratch s;   // (coded_host.inc; d_extra is total_q)
};

// generate_sign_words (rabitq_mmap.rs:337-340): word w = the w-th next_u64() of SmallRng::seed_from_u64(seed)
extern "C" int lynse_hip_rabitq_sign_words(uint64_t seed, uint64_t count, uint64_t* out) {
    if (count && !out) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    pqrng::Xoshiro256pp rng = pqrng::Xoshiro256pp::seed_from_u64(seed);
    for (uint64_t i = 0; i < count; ++i) out[i] = rng.next();
    return LYNSE_OK;
}

// the rotation kernels keep rb * P floats in LDS: past 64 KiB the limit is raised once per kernel
static int rbq_rotation_lds(size_t bytes) {
    if (bytes <= 64u * 1024u) return LYNSE_OK;
    LY_TRY(ensure_lds<k_rbq_encode>(PoolRerank::LDS_MAX));
    return ensure_lds<k_rbq_query>(PoolRerank::LDS_MAX);
}

static int rbq_alloc(RbqIndex& out, uint32_t dim, uint64_t n, const uint64_t* sign_words, uint32_t n_sign_words) {
    LY_TRY(out.alloc(dim, 1, n, sign_words, n_sign_words));
    return out.norms.alloc(n);
}

// RaBitQIndex::build (rabitq_mmap.rs:68-156) over the handle's rows
extern "C" int lynse_hip_flat_build_rabitq(lynse_hip_flat* h) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    LY_WRITER(h, lk);
    LY_TRY(use_device(h));
    LY_TRY(coded_check_handle(h, "RaBitQ", true));
    const uint64_t n = h->n;
    if (n == 0) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "need at least one vector");
    if (n > 0xffffffffull) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "a RaBitQ index holds at most 2^32 - 1 rows");
    const uint32_t nw = (rbq_next_pow2(h->dim) + 63) / 64;
    std::vector<uint64_t> sign(nw);
    LY_TRY(lynse_hip_rabitq_sign_words(42, nw, sign.data()));
    RbqIndex fresh;   // (freed on every failing path)
    LY_TRY(rbq_alloc(fresh, h->dim, n, sign.data(), nw));
    const uint32_t rb = std::max<uint32_t>(1, std::min<uint32_t>(8, 4096u / fresh.P));
    const size_t lds = (size_t)rb * fresh.P * 4;
    LY_TRY(rbq_rotation_lds(lds));
    hipStream_t st = cur(h).stream;
    RbqEncodeArgs a{h->rows, h->ld, h->dim, fresh.P, n, rb, fresh.ng, fresh.d_sign.p, fresh.codes.p, fresh.norms.p};
    hipLaunchKernelGGL(k_rbq_encode, dim3((uint32_t)((n + rb - 1) / rb)), dim3(RBQ_ENC_NT), lds, st, a);
    LY_HIP(hipGetLastError());
    LY_HIP(hipStreamSynchronize(st));
    coded_install(h->rbq, fresh);
    return LYNSE_OK;
}

// RaBitQIndex::load's in-memory half: codes[n][code_bytes] and norms[n] as the file holds them
extern "C" int lynse_hip_flat_load_rabitq(lynse_hip_flat* h, uint32_t dim, const uint64_t* sign_words, uint32_t n_sign_words,
                                          const uint8_t* codes, const float* norms, uint64_t n) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    LY_WRITER(h, lk);
    LY_TRY(use_device(h));
    LY_TRY(coded_check_handle(h, "RaBitQ", true));
    if (dim == 0 || dim != h->dim) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "Invalid RaBitQ dimensions");
    if (n == 0) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "need at least one vector");
    if (n > 0xffffffffull) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "a RaBitQ index holds at most 2^32 - 1 rows");
    if (n > h->n) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "the RaBitQ index covers more rows than the handle holds");
    if (!codes || !norms || (n_sign_words && !sign_words)) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    RbqIndex fresh;
    LY_TRY(rbq_alloc(fresh, dim, n, sign_words, n_sign_words));
    LY_TRY(fresh.upload(codes));
    LY_TRY(h2d_done(fresh.norms.p, norms, (size_t)n * 4));
    coded_install(h->rbq, fresh);
    return LYNSE_OK;
}

extern "C" int lynse_hip_flat_rabitq_params(lynse_hip_flat* h, uint32_t* dims, uint64_t* n_rbq, uint64_t* sign_words, uint8_t* codes,
                                            float* norms) {
    if (!h || !dims || !n_rbq) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    std::shared_lock<std::shared_mutex> lk(h->rw);
    if (!h->rbq || !h->rbq->ix.codes.p) {
        dims[0] = dims[1] = dims[2] = 0;
        *n_rbq = 0;
        return LYNSE_OK;
    }
    const RbqIndex& r = h->rbq->ix;
    dims[0] = h->dim; dims[1] = r.P; dims[2] = r.cb;
    *n_rbq = r.n;
    LY_TRY(use_device(h));
    if (sign_words) memcpy(sign_words, r.sign.data(), r.sign.size() * 8);
    if (codes) LY_TRY(r.download(codes));
    if (norms) LY_HIP(hipMemcpy(norms, r.norms.p, (size_t)r.n * 4, hipMemcpyDeviceToHost));
    return LYNSE_OK;
}

extern "C" int lynse_hip_flat_drop_rabitq(lynse_hip_flat* h) { return coded_drop(h, &lynse_hip_flat::rbq); }

extern "C" int lynse_hip_flat_rabitq_stage_times(lynse_hip_flat* h, double* out3, int reset) {
    if (!h || !out3) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    LY_WRITER(h, lk);
    return coded_stage_times(h->rbq, out3, reset);
}

// RaBitQIndex::search_candidates + rescore_exact_with (rabitq_mmap.rs:177-227) through coded_search, by the binary score; a chunk's byte
// tables stay at or under 256 MiB, and a pool is 200 k rows, so a small batch's rescore is split.
extern "C" int lynse_hip_flat_search_rabitq_f32(lynse_hip_flat* h, const float* queries, uint64_t nq, uint32_t k, int metric,
                                                uint32_t oversample, uint64_t* out_rows, float* out_dists, uint32_t* out_counts) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    LY_TRY(metric_check(metric));
    if (metric_binary(metric)) return set_error(LYNSE_ERR_UNSUPPORTED, "RaBitQ is defined for ip / l2 / cosine");
    if (nq == 0) return LYNSE_OK;
    if (!queries || !out_counts || (k && (!out_rows || !out_dists))) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    LY_WRITER(h, lk);
    LY_TRY(use_device(h));
    LY_TRY(coded_check_handle(h, "RaBitQ", true));
    if (!h->rbq || !h->rbq->ix.codes.p) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "no RaBitQ index on this handle: build or load one first");
    const RbqIndex& p = h->rbq->ix;
    CodedScratch& s = h->rbq->s;
    LY_TRY(rbq_rotation_lds((size_t)p.P * 4));
    const auto score = [&](hipStream_t st, uint32_t nqc, bool asc) -> int {
        // a small batch spreads each query's tables over up to 8 workgroups; one more per query sums total_q
        const uint32_t parts = nqc >= 32 ? 1u : std::max<uint32_t>(1, std::min<uint32_t>(8, p.cb / 16));
        hipLaunchKernelGGL(k_rbq_query, dim3(nqc, parts + 1), dim3(RBQ_Q_NT), (size_t)p.P * 4, st, s.d_q, h->dim, p.P, p.cb, p.d_sign.p, s.d_lut,
                           s.d_extra);
        LY_HIP(hipGetLastError());
        // the scan: QB = 4 queries share a code load when the batch has them; tables in <= 64 KiB of LDS, whole column groups
        const int qb = nqc >= 4 ? 4 : 1;
        const uint32_t mc = p.cb < 16 ? p.cb : std::min<uint32_t>(p.cb, 64u / (uint32_t)qb);
        RbqScanArgs sa{reinterpret_cast<const uint4*>(p.codes.p), p.norms.p, p.n, p.cb, p.ng, mc, (float)p.P, s.d_lut, s.d_extra, nqc,
                       asc ? 1 : 0, s.cut.d_S};
        const dim3 sgrid((uint32_t)((p.n + RBQ_NT * RBQ_R - 1) / (RBQ_NT * RBQ_R)), (nqc + qb - 1) / qb);
        const size_t slds = (size_t)qb * mc * 256 * 4;
        if (qb == 4) hipLaunchKernelGGL(k_rbq_scan<4>, sgrid, dim3(RBQ_NT), slds, st, sa);
        else hipLaunchKernelGGL(k_rbq_scan<1>, sgrid, dim3(RBQ_NT), slds, st, sa);
        LY_HIP(hipGetLastError());
        return LYNSE_OK;
    };
    return coded_search(h, s, {"RaBitQ", p.n, (size_t)p.cb * 256, true, true, true}, queries, nq, k, metric, oversample, out_rows, out_dists,
                        out_counts, score);
}
