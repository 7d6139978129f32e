// pq_host.inc — FLAT-{IP,L2,COS}-PQ on a FLAT handle (PQIndex, src/storage/pq_mmap.rs; Collection, src/engine.rs:4559-4600,
// :5504-5526): the SmallRng restatement, the device training and encoding, the ADC table and scan launches.  Included at the end of
// lynse_hip.hip after coded_host.inc, which holds the frame it shares with RaBitQ and PolarVec (DevBuf, CodedScratch, the handle check,
// the search driver around ScoreCut and PoolRerank); kernels in pq.h.  DESIGN.md §12.

// The quantiser.  Codes cover the first n rows of the handle: rows appended after a build or a load stay outside the index (the
// reference neither re-encodes nor drops them on flush).
struct PqIndex {
    uint32_t M = 0, K = 0, ss = 0;
    uint64_t n = 0;
    DevBuf<float> cb;        // [M][K][ss] f32 codebooks
    DevBuf<uint8_t> codes;   // [n][M] u8 codes
};
struct PqState {
    PqIndex ix;
    CodedScratch s;   // (coded_host.inc)
};

// ---- SmallRng (rand 0.8.5 on 64-bit: Xoshiro256PlusPlus) and random_init_centroids' draws --------------------------------
namespace pqrng {
static inline uint64_t rotl(uint64_t x, int k) { return (x << k) | (x >> (64 - k)); }
static inline uint64_t splitmix(uint64_t& state) {   // SeedableRng::seed_from_u64's generator (rand_core 0.6)
    state += 0x9e3779b97f4a7c15ull;
    uint64_t z = state;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
struct Xoshiro256pp {
    uint64_t s[4];
    static Xoshiro256pp seed_from_u64(uint64_t seed) {
        Xoshiro256pp r;
        uint64_t st = seed;
        for (auto& w : r.s) w = splitmix(st);
        if (!(r.s[0] | r.s[1] | r.s[2] | r.s[3])) return seed_from_u64(0);   // from_seed: an all-zero seed re-seeds from 0
        return r;
    }
    uint64_t next() {
        const uint64_t result = rotl(s[0] + s[3], 23) + s[0];
        const uint64_t t = s[1] << 17;
        s[2] ^= s[0];
        s[3] ^= s[1];
        s[1] ^= s[2];
        s[0] ^= s[3];
        s[2] ^= t;
        s[3] = rotl(s[3], 45);
        return result;
    }
    // gen_range(0..n), n >= 1 (UniformInt::sample_single: widening multiply, rejection zone = (n << lzcnt(n)) - 1)
    uint64_t below(uint64_t n) {
        const uint64_t zone = (n << __builtin_clzll(n)) - 1;
        for (;;) {
            const unsigned __int128 p = (unsigned __int128)next() * n;
            if ((uint64_t)p <= zone) return (uint64_t)(p >> 64);
        }
    }
};
// random_init_centroids (pq_mmap.rs:665-689): distinct indices, at most 10 k attempts; returns how many were chosen
static uint32_t init_indices(uint64_t seed, uint64_t n, uint32_t k, uint32_t* idx) {
    Xoshiro256pp rng = Xoshiro256pp::seed_from_u64(seed);
    std::vector<uint64_t> seen;
    seen.reserve(k);
    uint32_t c = 0;
    uint64_t attempts = 0;
    while (c < k && attempts < (uint64_t)k * 10) {
        const uint64_t i = rng.below(n);
        if (std::find(seen.begin(), seen.end(), i) == seen.end()) {
            seen.push_back(i);
            idx[c++] = (uint32_t)i;
        }
        ++attempts;
    }
    return c;
}
}  // namespace pqrng

extern "C" int lynse_hip_pq_xoshiro_stream(const uint64_t* state4, uint64_t count, uint64_t* out) {
    if (!state4 || (count && !out)) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    pqrng::Xoshiro256pp r;
    for (int i = 0; i < 4; ++i) r.s[i] = state4[i];
    for (uint64_t i = 0; i < count; ++i) out[i] = r.next();
    return LYNSE_OK;
}

extern "C" int lynse_hip_pq_splitmix_stream(uint64_t seed, uint64_t count, uint64_t* out) {
    if (count && !out) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    uint64_t st = seed;
    for (uint64_t i = 0; i < count; ++i) out[i] = pqrng::splitmix(st);
    return LYNSE_OK;
}

extern "C" int lynse_hip_pq_init_indices(uint64_t seed, uint64_t n, uint32_t k, uint32_t* idx, uint32_t* chosen) {
    if (!chosen || (k && !idx)) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n == 0 && k) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "need at least one vector");
    *chosen = k ? pqrng::init_indices(seed, n, k, idx) : 0u;
    return LYNSE_OK;
}

// ---- build / load ------------------------------------------------------------------------------------------------------------
// encode (pq_mmap.rs:696-735): codes[i][m] = argmin over the K codewords of l2_squared_f32, first strictly smaller wins
static int pq_launch_assign(PqAssignArgs a, uint64_t n_rows, hipStream_t st) {
    const size_t lds = (size_t)a.K * a.ss * 4;
    a.cb_lds = lds <= 64u * 1024u;
    const dim3 grid((uint32_t)((n_rows + 255) / 256), a.M);
    const size_t sh = a.cb_lds ? lds : 0;
    if (a.ss <= 8) hipLaunchKernelGGL(k_pq_assign<8>, grid, dim3(256), sh, st, a);
    else if (a.ss <= 16) hipLaunchKernelGGL(k_pq_assign<16>, grid, dim3(256), sh, st, a);
    else if (a.ss <= 32) hipLaunchKernelGGL(k_pq_assign<32>, grid, dim3(256), sh, st, a);
    else if (a.ss <= 64) hipLaunchKernelGGL(k_pq_assign<64>, grid, dim3(256), sh, st, a);
    else if (a.ss <= 128) hipLaunchKernelGGL(k_pq_assign<128>, grid, dim3(256), sh, st, a);
    else hipLaunchKernelGGL(k_pq_assign<0>, grid, dim3(256), sh, st, a);
    LY_HIP(hipGetLastError());
    return LYNSE_OK;
}

// a fresh index with its two device arrays
static int pq_alloc(PqIndex& out, uint32_t M, uint32_t K, uint32_t ss, uint64_t n) {
    out.M = M; out.K = K; out.ss = ss; out.n = n;
    LY_TRY(out.cb.alloc((size_t)M * K * ss));
    if (out.codes.alloc((size_t)n * M) != LYNSE_OK) return set_error(LYNSE_ERR_OUT_OF_MEMORY, "hipMalloc(PQ codes)");
    return LYNSE_OK;
}

// PQIndex::build_with_clusters (pq_mmap.rs:73-149) over the handle's rows, the writer lock held
static int pq_build_locked(lynse_hip_flat* h, uint32_t M, uint32_t n_clusters) {
    const uint64_t n = h->n;
    const uint32_t D = h->dim;
    if (n == 0) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "need at least one vector");
    if (M == 0 || D % M != 0) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "dim must be divisible by n_subspaces");
    const uint32_t ss = D / M;
    const uint32_t K = (uint32_t)std::min<uint64_t>(std::min<uint32_t>(std::max<uint32_t>(n_clusters, 1), 256), n);
    const uint64_t train_n = std::min<uint64_t>(n, 50000);
    const uint64_t stride = train_n < n ? std::max<uint64_t>(n / train_n, 1) : 1;
    const uint32_t iters = K <= 64 ? 6 : 15;
    hipStream_t st = cur(h).stream;
    DevBuf<float> T, raw;   // scratch of the build
    DevBuf<uint32_t> idx, chosen, asg, active, changed, count;
    LY_TRY(T.alloc((size_t)train_n * D));
    LY_TRY(raw.alloc((size_t)M * K * ss));
    LY_TRY(idx.alloc((size_t)M * K));
    LY_TRY(chosen.alloc(M));
    LY_TRY(asg.alloc((size_t)M * train_n));
    LY_TRY(active.alloc(M));
    LY_TRY(changed.alloc(M));
    LY_TRY(count.alloc((size_t)M * K));
    PqIndex fresh;   // (freed on every failing path)
    LY_TRY(pq_alloc(fresh, M, K, ss, n));
    float* cb = fresh.cb.p;
    const uint32_t gather_blocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((train_n * D + 255) / 256, (uint64_t)h->num_cu * 32));
    hipLaunchKernelGGL(k_pq_gather, dim3(gather_blocks), dim3(256), 0, st, h->rows, h->ld, D, stride, train_n, T.p);
    if (hipGetLastError() != hipSuccess) return set_error(LYNSE_ERR_DEVICE, "k_pq_gather launch");
    // the K draws of each subspace (seed m) on the host
    std::vector<uint32_t> h_idx((size_t)M * K, 0u), h_chosen(M), h_active(M, 1u), h_changed(M);
    for (uint32_t m = 0; m < M; ++m) h_chosen[m] = pqrng::init_indices(m, train_n, K, h_idx.data() + (size_t)m * K);
    auto run = [&]() -> int {
        LY_HIP(hipMemcpyAsync(idx.p, h_idx.data(), h_idx.size() * 4, hipMemcpyHostToDevice, st));
        LY_HIP(hipMemcpyAsync(chosen.p, h_chosen.data(), (size_t)M * 4, hipMemcpyHostToDevice, st));
        LY_HIP(hipMemcpyAsync(active.p, h_active.data(), (size_t)M * 4, hipMemcpyHostToDevice, st));
        LY_HIP(hipMemsetAsync(asg.p, 0, (size_t)M * train_n * 4, st));
        hipLaunchKernelGGL(k_pq_init, dim3(M), dim3(64), 0, st, T.p, D, ss, K, idx.p, chosen.p, cb);
        LY_HIP(hipGetLastError());
        for (uint32_t it = 0; it < iters; ++it) {
            LY_HIP(hipMemsetAsync(changed.p, 0, (size_t)M * 4, st));
            PqAssignArgs a{T.p, D, train_n, M, ss, K, cb, 0, active.p, asg.p, changed.p, nullptr};
            LY_TRY(pq_launch_assign(a, train_n, st));
            LY_HIP(hipMemcpyAsync(h_changed.data(), changed.p, (size_t)M * 4, hipMemcpyDeviceToHost, st));
            LY_HIP(hipStreamSynchronize(st));
            bool any = false;
            for (uint32_t m = 0; m < M; ++m) {   // no assignment moved: this subspace stops BEFORE the update
                h_active[m] = h_active[m] && h_changed[m];
                any = any || h_active[m];
            }
            if (!any) break;
            LY_HIP(hipMemcpyAsync(active.p, h_active.data(), (size_t)M * 4, hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(k_pq_update, dim3(K, M), dim3(64), 0, st, T.p, D, train_n, ss, K, active.p, asg.p, raw.p, cb, count.p);
            LY_HIP(hipGetLastError());
            hipLaunchKernelGGL(k_pq_empty, dim3(M), dim3(64), 0, st, ss, K, active.p, raw.p, cb, count.p);
            LY_HIP(hipGetLastError());
        }
        PqAssignArgs e{h->rows, h->ld, n, M, ss, K, cb, 0, nullptr, nullptr, nullptr, fresh.codes.p};
        LY_TRY(pq_launch_assign(e, n, st));
        LY_HIP(hipStreamSynchronize(st));
        return LYNSE_OK;
    };
    const int rc = run();
    if (rc != LYNSE_OK) {
        (void)hipStreamSynchronize(st);   // (the buffers go with this frame)
        return rc;
    }
    coded_install(h->pq, fresh);
    return LYNSE_OK;
}

extern "C" int lynse_hip_flat_build_pq(lynse_hip_flat* h, uint32_t n_subspaces, uint32_t n_clusters) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    LY_WRITER(h, lk);
    LY_TRY(use_device(h));
    LY_TRY(coded_check_handle(h, "PQ", false));
    return pq_build_locked(h, n_subspaces, n_clusters);
}

extern "C" int lynse_hip_flat_load_pq(lynse_hip_flat* h, uint32_t M, uint32_t K, const float* codebooks, const uint8_t* codes, uint64_t n) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    LY_WRITER(h, lk);
    LY_TRY(use_device(h));
    LY_TRY(coded_check_handle(h, "PQ", false));
    // PQIndex::load's checks (pq_mmap.rs:481-494, :526-531)
    if (M == 0 || K == 0 || K > 256 || h->dim % M != 0 || n > 0xffffffffull)
        return set_error(LYNSE_ERR_INVALID_ARGUMENT, "Invalid PQ index dimensions");
    if (n == 0) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "need at least one vector");
    if (n > h->n) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "the PQ index covers more rows than the handle holds");
    if (!codebooks || !codes) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    for (uint64_t i = 0; i < n * M; ++i)
        if (codes[i] >= K) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "PQ index contains an out-of-range code");
    const uint32_t ss = h->dim / M;
    PqIndex fresh;
    LY_TRY(pq_alloc(fresh, M, K, ss, n));
    if (h2d_done(fresh.cb.p, codebooks, (size_t)M * K * ss * 4) != LYNSE_OK || h2d_done(fresh.codes.p, codes, (size_t)n * M) != LYNSE_OK)
        return LYNSE_ERR_DEVICE;
    coded_install(h->pq, fresh);
    return LYNSE_OK;
}

extern "C" int lynse_hip_flat_pq_params(lynse_hip_flat* h, uint32_t* mks, uint64_t* n_pq, float* codebooks, uint8_t* codes) {
    if (!h || !mks || !n_pq) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    std::shared_lock<std::shared_mutex> lk(h->rw);
    if (!h->pq || !h->pq->ix.cb.p) {
        mks[0] = mks[1] = mks[2] = 0;
        *n_pq = 0;
        return LYNSE_OK;
    }
    const PqIndex& p = h->pq->ix;
    mks[0] = p.M; mks[1] = p.K; mks[2] = p.ss;
    *n_pq = p.n;
    LY_TRY(use_device(h));
    if (codebooks) LY_HIP(hipMemcpy(codebooks, p.cb.p, (size_t)p.M * p.K * p.ss * 4, hipMemcpyDeviceToHost));
    if (codes) LY_HIP(hipMemcpy(codes, p.codes.p, (size_t)p.n * p.M, hipMemcpyDeviceToHost));
    return LYNSE_OK;
}

extern "C" int lynse_hip_flat_drop_pq(lynse_hip_flat* h) { return coded_drop(h, &lynse_hip_flat::pq); }

extern "C" int lynse_hip_flat_pq_stage_times(lynse_hip_flat* h, double* out3, int reset) {
    if (!h || !out3) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    LY_WRITER(h, lk);
    return coded_stage_times(h->pq, out3, reset);
}

// ---- search --------------------------------------------------------------------------------------------------------------------
// PQIndex::search_candidates + rescore_exact_candidates (pq_mmap.rs:176-240, vector_store.rs:611-638) through coded_search, by the ADC
// score; the tables of a chunk are not capped.
extern "C" int lynse_hip_flat_search_pq_f32(lynse_hip_flat* h, const float* queries, uint64_t nq, uint32_t k, int metric, uint32_t oversample,
                                            uint64_t* out_rows, float* out_dists, uint32_t* out_counts) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    LY_TRY(metric_check(metric));
    if (metric_binary(metric)) return set_error(LYNSE_ERR_UNSUPPORTED, "PQ is defined for ip / l2 / cosine");
    if (nq == 0) return LYNSE_OK;
    if (!queries || !out_counts || (k && (!out_rows || !out_dists))) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    LY_WRITER(h, lk);
    LY_TRY(use_device(h));
    LY_TRY(coded_check_handle(h, "PQ", false));
    if (!h->pq || !h->pq->ix.cb.p) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "no PQ index on this handle: build or load one first");
    const PqIndex& p = h->pq->ix;
    CodedScratch& s = h->pq->s;
    const auto score = [&](hipStream_t st, uint32_t nqc, bool asc) -> int {
        const uint64_t lut_threads = (uint64_t)nqc * p.M * p.K;
        hipLaunchKernelGGL(k_pq_lut, dim3((uint32_t)((lut_threads + 255) / 256)), dim3(256), 0, st, s.d_q, nqc, h->dim, p.M, p.ss, p.K, p.cb.p,
                           metric == M_IP ? 1 : 0, s.d_lut);
        LY_HIP(hipGetLastError());
        // the ADC scan: QB = 4 queries share a code load when the batch has them; tables in <= 64 KiB of LDS
        const int qb = nqc >= 4 ? 4 : 1;
        const uint32_t mc = std::max<uint32_t>(1, std::min<uint32_t>(p.M, 16384u / ((uint32_t)qb * p.K)));
        PqAdcArgs aa{p.codes.p, p.n, p.M, p.K, mc, s.d_lut, nqc, asc ? 1 : 0, s.cut.d_S};
        const dim3 agrid((uint32_t)((p.n + PQ_NT * PQ_R - 1) / (PQ_NT * PQ_R)), (nqc + qb - 1) / qb);
        const size_t alds = (size_t)qb * mc * p.K * 4;
        if (qb == 4) hipLaunchKernelGGL(k_pq_adc<4>, agrid, dim3(PQ_NT), alds, st, aa);
        else hipLaunchKernelGGL(k_pq_adc<1>, agrid, dim3(PQ_NT), alds, st, aa);
        LY_HIP(hipGetLastError());
        return LYNSE_OK;
    };
    return coded_search(h, s, {"PQ", p.n, (size_t)p.M * p.K, false, false, false}, queries, nq, k, metric, oversample, out_rows, out_dists,
                        out_counts, score);
}
