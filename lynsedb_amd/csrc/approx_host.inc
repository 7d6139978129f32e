// approx_host.inc — the approximate flat search on a FLAT handle (lynse_hip_flat_search_approx_f32), its eps helpers and its size
// policy.  Included at the end of lynse_hip.hip after additive_host.inc; kernels in approx.h; scratch, cut and order are the range
// search's (RangeState, ScoreCut::cut, k_pool_select or select_pool_keys).  The APPROXIMATE FLAT SEARCH block of include/lynse_hip.h
// states the contract, DESIGN.md §27 the reasoning.

// ---- eps -------------------------------------------------------------------------------------------------------------------------
extern "C" float lynse_hip_normalize_eps(float eps) {   // approx_search.rs:113-119
    if (std::isfinite(eps) && eps > 0.0f) return eps > 1e-8f ? eps : 1e-8f;
    return 1e-4f;
}

extern "C" void lynse_hip_round_distances_to_eps(float* d, size_t n, float eps) {   // approx_search.rs:123-143
    if (!d || !(eps > 0.0f)) return;
    for (size_t i = 0; i < n; ++i) {
        const float v = d[i];
        if (!std::isfinite(v)) continue;
        const float scaled = v / eps;
        if (!std::isfinite(scaled)) continue;
        const float rounded = roundf(scaled) * eps;   // Rust's f32::round: half away from zero
        if (std::isfinite(rounded)) d[i] = rounded;
    }
}

// ---- the size policy (host only) -------------------------------------------------------------------------------------------------
static int approx_eps_band(float eps) {   // 0: <= 1e-6, 1: <= 1e-5, 2: <= 1e-4, 3: <= 1e-3, 4: <= 1e-2, 5: above
    const float edge[5] = {1e-6f, 1e-5f, 1e-4f, 1e-3f, 1e-2f};
    int b = 0;
    while (b < 5 && !(eps <= edge[b])) ++b;
    return b;
}
static uint64_t approx_mul_sat(uint64_t a, uint64_t b) { return b && a > UINT64_MAX / b ? UINT64_MAX : a * b; }
static uint64_t approx_pool(uint64_t k, uint64_t n, const uint64_t per_k, const uint64_t div, uint64_t cap) {
    uint64_t p = std::max(approx_mul_sat(k, per_k), n / div);
    p = std::max(p, k + 128);
    return std::min(std::min(p, n), cap);
}
extern "C" uint64_t lynse_hip_approx_ip_order_pool(uint64_t k, uint64_t n, float eps) {   // flat_mmap.rs:3739-3771
    static const uint64_t per_k[6] = {1000, 750, 500, 250, 120, 60}, div[6] = {100, 133, 200, 400, 800, 1600};
    const int b = approx_eps_band(eps);
    return approx_pool(k, n, per_k[b], div[b], std::max<uint64_t>(20000, std::min(k, n)));
}
extern "C" uint64_t lynse_hip_approx_hybrid_ip_pool(uint64_t k, uint64_t n, float eps) {   // :3930-3962
    static const uint64_t per_k[6] = {8000, 6000, 5000, 3000, 2000, 1000}, div[6] = {20, 20, 20, 40, 80, 160};
    const int b = approx_eps_band(eps);
    return approx_pool(k, n, per_k[b], div[b], 100000);
}
extern "C" uint64_t lynse_hip_approx_hybrid_pool(uint64_t k, uint64_t n, float eps) {   // :4024-4056
    static const uint64_t per_k[6] = {4000, 3000, 2000, 1000, 500, 250}, div[6] = {50, 50, 50, 100, 200, 400};
    const int b = approx_eps_band(eps);
    return approx_pool(k, n, per_k[b], div[b], 100000);
}
static uint32_t approx_sample(uint32_t dim, float ratio) {
    if (dim <= 32) return dim;
    const uint32_t s = (uint32_t)roundf((float)dim * ratio);
    return std::min(std::max<uint32_t>(s, 32), dim);
}
extern "C" uint32_t lynse_hip_approx_hybrid_ip_sample_dims(uint32_t dim, float eps) {   // :3911-3927
    static const float ratio[6] = {0.75f, 0.625f, 0.5f, 0.375f, 0.25f, 0.25f};
    return approx_sample(dim, ratio[approx_eps_band(eps)]);
}
extern "C" uint32_t lynse_hip_approx_hybrid_sample_dims(uint32_t dim, float eps) {   // :4003-4021
    static const float ratio[6] = {0.875f, 0.75f, 0.625f, 0.5f, 0.375f, 0.25f};
    return approx_sample(dim, ratio[approx_eps_band(eps)]);
}
// sampled_dim_blocks (:4468-4496): up to three contiguous blocks — head, middle, tail; returns their number
extern "C" uint32_t lynse_hip_approx_sampled_dim_blocks(uint32_t dim, uint32_t sample, uint32_t* out_start, uint32_t* out_len) {
    sample = std::min(sample, dim);
    if (sample == 0 || !out_start || !out_len) return 0;
    if (sample == dim) { out_start[0] = 0; out_len[0] = dim; return 1; }
    const uint32_t nb = std::min<uint32_t>(sample, 3);
    if (nb <= 1) { out_start[0] = (dim - sample) / 2; out_len[0] = sample; return 1; }
    uint32_t remaining = sample;
    for (uint32_t i = 0; i < nb; ++i) {
        const uint32_t left = nb - i, len = (remaining + left - 1) / left;
        remaining -= len;
        const uint64_t max_start = dim > len ? dim - len : 0;
        out_start[i] = (uint32_t)(((uint64_t)i * max_start + (nb - 1) / 2) / (nb - 1));
        out_len[i] = len;
    }
    return nb;
}

// ---- the derived copies ----------------------------------------------------------------------------------------------------------
// Row sums, squared norms and inverse norms of rows [0, n), and the two sum orders cut from the sums.  Valid only while n == h->n:
// an append moves h->n, and everything that rewrites rows goes through reset_derived_locked (mutate_host.inc) or empties the shard
// (lynse_hip_top_k_search), which release the state — the keys the other derived copies (n_stats, n16, CodeSet::n) go by.
struct ApproxState {
    float *row_sum = nullptr, *norm2 = nullptr, *inv_norm = nullptr;
    unsigned long long* d_fin = nullptr;
    uint64_t n = 0, finite = 0;   // rows covered (0: nothing built) / rows with a finite sum
    struct Order { uint64_t* rows = nullptr; uint32_t* d_cnt = nullptr; uint64_t n = 0; uint32_t pool = 0; } order[2];   // [0] sum desc, [1] sum asc
    float* d_q = nullptr;
    ~ApproxState() {
        for (void* p : {(void*)row_sum, (void*)norm2, (void*)inv_norm, (void*)d_fin, (void*)order[0].rows, (void*)order[0].d_cnt,
                        (void*)order[1].rows, (void*)order[1].d_cnt, (void*)d_q})
            if (p) (void)hipFree(p);
    }
};

static void approx_release(lynse_hip_flat* h) {
    delete h->approx;
    h->approx = nullptr;
}

static int approx_ensure_stats(lynse_hip_flat* h, hipStream_t st) {
    if (h->approx && h->approx->n == h->n) return LYNSE_OK;
    approx_release(h);
    h->approx = new ApproxState();   // (n == 0 until the pass is done: a failure below leaves nothing that counts as built)
    ApproxState* s = h->approx;
    const uint64_t n = h->n;
    LY_HIP(hipMalloc(&s->row_sum, (size_t)n * 4));
    LY_HIP(hipMalloc(&s->norm2, (size_t)n * 4));
    LY_HIP(hipMalloc(&s->inv_norm, (size_t)n * 4));
    LY_HIP(hipMalloc(&s->d_fin, 8));
    LY_HIP(hipMemsetAsync(s->d_fin, 0, 8, st));
    ApproxStatsArgs a{h->rows, h->ld, h->dim, n, s->row_sum, s->norm2, s->inv_norm, s->d_fin};
    const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + 31) / 32, (uint64_t)h->num_cu * 16));
    hipLaunchKernelGGL(k_approx_rowstats, dim3(grid), dim3(APX_NT), 0, st, a);
    LY_HIP(hipGetLastError());
    unsigned long long fin = 0;
    LY_HIP(hipMemcpyAsync(&fin, s->d_fin, 8, hipMemcpyDeviceToHost, st));
    LY_TRY(stream_wait(st));
    s->finite = fin;
    s->n = n;
    return LYNSE_OK;
}

// the single-row IP form on the host (the query with itself): two 8-lane accumulators over chunks of 16, one more chunk of 8, the
// pairwise horizontal sum, the tail multiplied and added
static float approx_ip_single_host(const float* a, const float* b, uint32_t D) {
    float acc0[8] = {0}, acc1[8] = {0};
    const uint32_t chunks = D / 8, dbl = chunks / 2;
    for (uint32_t i = 0; i < dbl; ++i)
        for (int g = 0; g < 8; ++g) {
            acc0[g] = fmaf(a[i * 16 + g], b[i * 16 + g], acc0[g]);
            acc1[g] = fmaf(a[i * 16 + 8 + g], b[i * 16 + 8 + g], acc1[g]);
        }
    if (chunks % 2)
        for (int g = 0; g < 8; ++g) acc0[g] = fmaf(a[dbl * 16 + g], b[dbl * 16 + g], acc0[g]);
    float t[8];
    for (int g = 0; g < 8; ++g) t[g] = acc0[g] + acc1[g];
    float sum = ((t[0] + t[4]) + (t[1] + t[5])) + ((t[2] + t[6]) + (t[3] + t[7]));
    for (uint32_t i = chunks * 8; i < D; ++i) sum = sum + a[i] * b[i];
    return sum;
}

template <int FORM>
static int approx_coarse_launch(const ApproxCoarseArgs& a, uint32_t q_floats, uint32_t num_cu, hipStream_t st) {
    LY_TRY(ensure_lds<k_approx_coarse<FORM>>(PoolRerank::LDS_MAX));
    const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((a.n + 31) / 32, (uint64_t)num_cu * 32));
    hipLaunchKernelGGL(k_approx_coarse<FORM>, dim3(grid), dim3(APX_NT), (size_t)q_floats * 4, st, a);
    LY_HIP(hipGetLastError());
    return LYNSE_OK;
}

// The keys in p.rr.d_keys (their number in p.rr.d_pcnt, at most `ld`) ordered by the canonical key: the best k_sel go out.  Sorted in LDS
// up to 16,384 keys (k_pool_select), on the host beyond.
static int approx_order_keys(RangeState& p, uint32_t ld, uint32_t k_sel, int metric, hipStream_t st, uint64_t* out_rows, float* out_dists,
                             uint32_t* out_count) {
    const bool asc = metric_ascending(metric);
    if (ld <= 16384) {
        uint32_t p2 = 2;
        while (p2 < ld) p2 <<= 1;
        LY_TRY(ensure_lds<k_pool_select<256>>(PoolRerank::LDS_MAX));
        LY_TRY(ensure_lds<k_pool_select<1024>>(PoolRerank::LDS_MAX));
        LY_TRY(ivf_grow(&p.rr.d_out, &p.rr.out_cap, ((size_t)k_sel * 12 + 4 + 7) / 8));
        const size_t o_dist = (size_t)k_sel * 8, o_cnt = (size_t)k_sel * 12, o_all = o_cnt + 4;
        uint8_t* ob = reinterpret_cast<uint8_t*>(p.rr.d_out);
        PoolRerankArgs x{};
        x.pool_cnt = p.rr.d_pcnt;
        x.pool_ld = ld;
        x.p2 = p2;
        x.metric = metric;
        x.k = k_sel;
        x.out_k = k_sel;
        x.out_rows = p.rr.d_out;
        x.out_dists = reinterpret_cast<float*>(ob + o_dist);
        x.out_counts = reinterpret_cast<uint32_t*>(ob + o_cnt);
        x.keys_out = p.rr.d_keys;
        if (p2 >= 2048) hipLaunchKernelGGL(k_pool_select<1024>, dim3(1), dim3(1024), (size_t)p2 * 8, st, x);
        else hipLaunchKernelGGL(k_pool_select<256>, dim3(1), dim3(256), (size_t)p2 * 8, st, x);
        LY_HIP(hipGetLastError());
        p.h_out.resize((o_all + 7) / 8);
        LY_HIP(hipMemcpyAsync(p.h_out.data(), p.rr.d_out, o_all, hipMemcpyDeviceToHost, st));
        LY_TRY(stream_wait(st));
        const uint8_t* hb = reinterpret_cast<const uint8_t*>(p.h_out.data());
        memcpy(out_count, hb + o_cnt, 4);
        memcpy(out_rows, hb, (size_t)k_sel * 8);
        memcpy(out_dists, hb + o_dist, (size_t)k_sel * 4);
    } else {
        uint32_t cnt = 0;
        p.keys.resize(ld);
        LY_HIP(hipMemcpyAsync(p.keys.data(), p.rr.d_keys, (size_t)ld * 8, hipMemcpyDeviceToHost, st));
        LY_HIP(hipMemcpyAsync(&cnt, p.rr.d_pcnt, 4, hipMemcpyDeviceToHost, st));
        LY_TRY(stream_wait(st));
        *out_count = select_pool_keys(p.keys.data(), std::min(cnt, ld), k_sel, k_sel, asc, out_rows, out_dists);
    }
    return LYNSE_OK;
}

// What ran, for out_info
enum { APX_IP_NONE = 0, APX_IP_SUM_DESC = 1, APX_IP_SUM_ASC = 2, APX_IP_HYBRID = 3 };

// The part under the handle's lock.  *exact: the answer is the exact search's (path 2 under an additive metric, or a fall-back of
// paths 3 / 4) — the caller runs it once the lock is gone.
static int approx_search_locked(lynse_hip_flat* h, const float* query, uint32_t k_in, int metric, float eps, uint64_t* out_rows,
                                float* out_dists, uint32_t* out_count, lynse_hip_approx_info* info, bool* exact) {
    LY_WRITER(h, lk);
    LY_TRY(use_device(h));
    if (h->row_stride != 1 || h->row_offset != 0) return set_error(LYNSE_ERR_UNSUPPORTED, "the approximate search on a row-mapped handle is not supported");
    if (h->packed_only) return set_error(LYNSE_ERR_UNSUPPORTED, "a packed store answers the binary metrics only");
    if (is_f16(h)) return set_error(LYNSE_ERR_UNSUPPORTED, "the approximate search on an F16 shard is not supported");
    const uint64_t n = h->n;
    const uint32_t D = h->dim;
    *out_count = 0;
    if (n == 0 || k_in == 0) return LYNSE_OK;
    if ((size_t)D * 4 > PoolRerank::LDS_MAX) return set_error(LYNSE_ERR_UNSUPPORTED, "approximate search: the query does not fit in LDS");
    const uint32_t k = (uint32_t)std::min<uint64_t>(k_in, n);
    const bool big = D > 16 && n > 65536;
    hipStream_t st = cur(h).stream;
    int ip_form = h->ip_form;
    if (ip_form == LYNSE_IPFORM_AUTO) ip_form = n < 4096 ? LYNSE_IPFORM_SINGLE : LYNSE_IPFORM_BATCH8;

    // ---- the plan ----
    int form = -1;              // the coarse kernel; -1: none (a sum order)
    bool pooled = false;        // a pool is cut and rescored (paths 3 / 4); else the best k are cut from the score vector
    uint32_t pool = 0, sample = 0;
    ApproxBlocks blk{1, {0, 0, 0}, {D, 0, 0}};
    int order = -1;
    if (metric == M_IP && big) {
        info->path = 3;
        bool nonneg = true, nonpos = true;
        for (uint32_t i = 0; i < D; ++i) { nonneg = nonneg && query[i] >= 0.0f; nonpos = nonpos && query[i] <= 0.0f; }
        pooled = true;
        if (nonneg || nonpos) {
            order = nonneg ? 0 : 1;
            info->ip_case = nonneg ? APX_IP_SUM_DESC : APX_IP_SUM_ASC;
            pool = (uint32_t)lynse_hip_approx_ip_order_pool(k, n, eps);
        } else {
            info->ip_case = APX_IP_HYBRID;
            sample = lynse_hip_approx_hybrid_ip_sample_dims(D, eps);
            pool = (uint32_t)lynse_hip_approx_hybrid_ip_pool(k, n, eps);
            form = AF_IP;
        }
    } else if (metric == M_L2 || metric == M_COS) {
        info->path = 1;
        form = metric == M_L2 ? AF_L2EXP : AF_COSEXP;
    } else if (big) {   // an additive metric
        info->path = 4;
        pooled = true;
        sample = lynse_hip_approx_hybrid_sample_dims(D, eps);
        pool = (uint32_t)lynse_hip_approx_hybrid_pool(k, n, eps);
        form = metric == M_L1 ? AF_L1 : metric == M_CHEBYSHEV ? AF_CHEBYSHEV : metric == M_CANBERRA ? AF_CANBERRA : AF_BRAY_CURTIS;
    } else {
        info->path = 2;
        if (metric != M_IP) { *exact = true; return LYNSE_OK; }   // every row in its AVX2 form: the exact scan itself
        form = AF_IP;
        ip_form = LYNSE_IPFORM_SINGLE;   // exact_distance: simd::inner_product_f32 whatever n is
    }
    info->pool = pool;
    info->sample_dims = sample;
    if (pooled && order < 0) {
        if (sample >= D || pool >= n) { info->fell_back = 1; *exact = true; return LYNSE_OK; }
        blk.nb = lynse_hip_approx_sampled_dim_blocks(D, sample, blk.start, blk.len);
    }

    if (!h->range) h->range = new RangeState();
    RangeState& p = *h->range;
    float q_norm2 = 0.0f, q_inv = 0.0f;
    if (info->path == 1) {
        q_norm2 = approx_ip_single_host(query, query, D);
        q_inv = q_norm2 > 1e-30f ? 1.0f / sqrtf(q_norm2) : 0.0f;
        if (metric == M_COS && q_inv <= 0.0f) {   // norm_cached_cosine_topk: the first k rows at 1.0
            for (uint32_t i = 0; i < k; ++i) { out_rows[i] = i; out_dists[i] = 1.0f; }
            *out_count = k;
            return LYNSE_OK;
        }
    }
    if (info->path == 1 || order >= 0) LY_TRY(approx_ensure_stats(h, st));
    if (!h->approx) h->approx = new ApproxState();
    ApproxState& s = *h->approx;
    if (!s.d_q) LY_HIP(hipMalloc(&s.d_q, (size_t)D * 4));
    LY_HIP(hipMemcpyAsync(s.d_q, query, (size_t)D * 4, hipMemcpyHostToDevice, st));
    LY_TRY(p.cut.grow(1, n));
    LY_TRY(ivf_grow(&p.rr.d_pcnt, &p.rr.pcnt_cap, (size_t)1));

    if (form >= 0) {
        uint32_t q_floats = 0;
        for (uint32_t b = 0; b < blk.nb; ++b) q_floats += blk.len[b];
        ApproxCoarseArgs a{h->rows, h->ld, D, n, s.d_q, blk, ip_form, (float)D / (float)std::max<uint32_t>(q_floats, 1), q_norm2, q_inv,
                           s.norm2, s.inv_norm, p.cut.d_S};
        switch (form) {
        case AF_IP: LY_TRY(approx_coarse_launch<AF_IP>(a, q_floats, h->num_cu, st)); break;
        case AF_L2EXP: LY_TRY(approx_coarse_launch<AF_L2EXP>(a, q_floats, h->num_cu, st)); break;
        case AF_COSEXP: LY_TRY(approx_coarse_launch<AF_COSEXP>(a, q_floats, h->num_cu, st)); break;
        case AF_L1: LY_TRY(approx_coarse_launch<AF_L1>(a, q_floats, h->num_cu, st)); break;
        case AF_CHEBYSHEV: LY_TRY(approx_coarse_launch<AF_CHEBYSHEV>(a, q_floats, h->num_cu, st)); break;
        case AF_CANBERRA: LY_TRY(approx_coarse_launch<AF_CANBERRA>(a, q_floats, h->num_cu, st)); break;
        default: LY_TRY(approx_coarse_launch<AF_BRAY_CURTIS>(a, q_floats, h->num_cu, st)); break;
        }
    }

    if (!pooled) {   // paths 1 and 2: the best k straight from the score vector
        LY_TRY(ivf_grow(&p.rr.d_keys, &p.rr.keys_cap, (size_t)k));
        p.cut.sel0.assign(1, n > k ? PqSel{0ull, 64u, k, 0u, 0u} : PqSel{(uint64_t)(RANGE_FAIL - 1u), 32u, 0u, 1u, 0u});
        LY_TRY(p.cut.cut<true>(1, n, k, n > k, p.rr.d_keys, p.rr.d_pcnt, st));
        return approx_order_keys(p, k, k, metric, st, out_rows, out_dists, out_count);
    }

    // paths 3 and 4: the pool — a cached sum order, or the cut of the coarse scores — rescored exactly
    LY_TRY(ivf_grow(&p.rr.d_prow, &p.rr.prow_cap, (size_t)pool));
    LY_TRY(ivf_grow(&p.rr.d_keys, &p.rr.keys_cap, (size_t)pool));
    const uint64_t* pool_rows = p.rr.d_prow;
    const uint32_t* pool_cnt = p.rr.d_pcnt;
    if (order >= 0) {
        ApproxState::Order& o = s.order[order];
        if (o.n != n || o.pool != pool) {   // cut once per (n, pool)
            if (o.rows) (void)hipFree(o.rows);
            o.rows = nullptr;
            o.n = 0;
            LY_HIP(hipMalloc(&o.rows, (size_t)pool * 8));
            if (!o.d_cnt) LY_HIP(hipMalloc(&o.d_cnt, 4));
            const uint32_t blocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, (uint64_t)h->num_cu * 32));
            hipLaunchKernelGGL(k_approx_sum_keys, dim3(blocks), dim3(256), 0, st, s.row_sum, n, order == 0 ? 1 : 0, p.cut.d_S);
            LY_HIP(hipGetLastError());
            const bool select = s.finite > pool;
            p.cut.sel0.assign(1, select ? PqSel{0ull, 64u, pool, 0u, 0u} : PqSel{(uint64_t)(RANGE_FAIL - 1u), 32u, 0u, 1u, 0u});
            LY_TRY(p.cut.cut<false>(1, n, pool, select, o.rows, o.d_cnt, st));
            LY_TRY(stream_wait(st));
            o.n = n;
            o.pool = pool;
        }
        pool_rows = o.rows;
        pool_cnt = o.d_cnt;
    } else {
        p.cut.sel0.assign(1, PqSel{0ull, 64u, pool, 0u, 0u});
        LY_TRY(p.cut.cut<false>(1, n, pool, true, p.rr.d_prow, p.rr.d_pcnt, st));
    }
    ApproxRescoreArgs ra{h->rows, h->ld, D, n, s.d_q, pool_rows, pool_cnt, pool, metric, p.rr.d_keys};
    LY_TRY(ensure_lds<k_approx_rescore>(PoolRerank::LDS_MAX));
    hipLaunchKernelGGL(k_approx_rescore, dim3(std::max<uint32_t>(1, std::min<uint32_t>((pool + 31) / 32, (uint32_t)h->num_cu * 8))), dim3(APX_NT),
                       (size_t)D * 4, st, ra);
    LY_HIP(hipGetLastError());
    if (pool_cnt != p.rr.d_pcnt) LY_HIP(hipMemcpyAsync(p.rr.d_pcnt, pool_cnt, 4, hipMemcpyDeviceToDevice, st));
    return approx_order_keys(p, pool, k, metric, st, out_rows, out_dists, out_count);
}

extern "C" int lynse_hip_flat_search_approx_f32(lynse_hip_flat* h, const float* query, uint32_t k, int metric, float eps, uint64_t* out_rows,
                                                float* out_dists, uint32_t* out_count, lynse_hip_approx_info* out_info) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    if (!query || !out_count || (k && (!out_rows || !out_dists))) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!metric_valid(metric)) return set_error(LYNSE_ERR_UNKNOWN_METRIC, "Unknown metric id");
    if (metric_binary(metric)) return set_error(LYNSE_ERR_UNSUPPORTED, "the approximate search serves ip, l2, cosine, l1, chebyshev, canberra and bray_curtis");
    lynse_hip_approx_info info{};
    bool exact = false;
    LY_TRY(approx_search_locked(h, query, k, metric, lynse_hip_normalize_eps(eps), out_rows, out_dists, out_count, &info, &exact));
    if (out_info) *out_info = info;
    if (exact) return lynse_hip_flat_search_f32(h, query, 1, k, metric, out_rows, out_dists, out_count);
    return LYNSE_OK;
}
