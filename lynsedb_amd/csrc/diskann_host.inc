// diskann_host.inc — DISKANN-{L2,COS} on a FLAT handle (DiskANNIndex, src/index/diskann.rs, in memory and at full precision).
// Included from lynse_hip.hip after graph_host.inc, whose lock, handle check, clock, list normaliser and search driver it shares with
// hnsw_host.inc; kernels in diskann.h.  The rule block of
// include/lynse_hip.h states the contract, DESIGN.md §21 the reasoning.  The graph shares the handle's rows: it holds ids only.

struct DiskannState {
    int metric = -1;
    uint32_t r = 0, l = 0, entry = 0;
    float alpha = 0.0f;
    uint64_t n = 0;                       // the graph covers the first n rows of the handle
    uint32_t* d_adj = nullptr;            // [n][r]
    GraphSearchScratch search;            // with the searches timed with profiling on
    // the last build (microseconds of host time; the three stages only when it ran with profiling on, which synchronises them)
    double b_search_us = 0.0, b_prune_us = 0.0, b_commit_us = 0.0, b_draws_us = 0.0, b_total_us = 0.0;

    bool built() const { return d_adj != nullptr; }
    void free_index() {
        if (d_adj) (void)hipFree(d_adj);
        d_adj = nullptr;
        metric = -1;
        r = l = entry = 0;
        alpha = 0.0f;
        n = 0;
    }
    ~DiskannState() { free_index(); }
};

static void diskann_release(lynse_hip_flat* h) {
    delete h->diskann;
    h->diskann = nullptr;
}

constexpr uint32_t DISKANN_R_MAX = 64, DISKANN_L_MAX = 4096, DISKANN_L_BUILD_CAP = 128, DISKANN_BUILD_ANCHORS = 32, DISKANN_QUERY_ANCHORS = 8;

// rules 1-4, the part that does not depend on the rows: refs / cands (the prefixes of shuffles A and B), the order before the entry
// is swapped to its front, and the initial graph [n][r]
struct VamanaDraws { std::vector<uint32_t> refs, cands, order, adj0; };
static void vamana_draws(uint64_t seed, uint64_t n, uint32_t r, VamanaDraws& out) {
    pqrng::Xoshiro256pp rng = pqrng::Xoshiro256pp::seed_from_u64(seed);
    auto draw = [&](uint64_t b) { return (uint32_t)(((rng.next() >> 32) * b) >> 32); };
    auto shuffled = [&]() {
        std::vector<uint32_t> v(n);
        for (uint64_t i = 0; i < n; ++i) v[i] = (uint32_t)i;
        for (uint64_t i = n; i-- > 1;) std::swap(v[i], v[draw(i + 1)]);
        return v;
    };
    out.adj0.assign((size_t)n * r, GRAPH_PAD);
    if (n <= 1) {   // no word is consumed
        out.refs.assign(n, 0); out.cands.assign(n, 0); out.order.assign(n, 0);
        return;
    }
    out.refs = shuffled();
    out.refs.resize(std::min<uint64_t>(32, n));
    out.cands = shuffled();
    out.cands.resize(std::min<uint64_t>(64, n));
    const uint32_t deg = (uint32_t)std::min<uint64_t>(r, n - 1);
    for (uint64_t i = 0; i < n; ++i) {
        uint32_t* row = &out.adj0[(size_t)i * r];
        for (uint32_t c = 0; c < deg;) {
            const uint32_t j = draw(n);
            if (j != i && std::find(row, row + c, j) == row + c) row[c++] = j;
        }
    }
    out.order = shuffled();
}

extern "C" int lynse_hip_vamana_draws(uint64_t seed, uint64_t n, uint32_t r, uint32_t* refs, uint32_t* cands, uint32_t* order, uint32_t* adj0) {
    if (n && (!refs || !cands || !order || !adj0)) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    if (r < 1 || r > DISKANN_R_MAX) return set_error(LYNSE_ERR_UNSUPPORTED, "DiskANN: r must be between 1 and 64");
    if (n >= 0xffffffffull) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "a DiskANN index holds fewer than 2^32 - 1 rows");
    VamanaDraws d;
    vamana_draws(seed, n, r, d);
    if (n) {
        memcpy(refs, d.refs.data(), d.refs.size() * 4);
        memcpy(cands, d.cands.data(), d.cands.size() * 4);
        memcpy(order, d.order.data(), d.order.size() * 4);
        memcpy(adj0, d.adj0.data(), d.adj0.size() * 4);
    }
    return LYNSE_OK;
}

static int diskann_check_metric(int metric) {
    LY_TRY(metric_check(metric));
    if (metric != M_L2 && metric != M_COS) return set_error(LYNSE_ERR_UNSUPPORTED, "DiskANN is built for l2 / cosine");
    return LYNSE_OK;
}
static int diskann_check_params(uint32_t r, uint32_t l) {
    if (r < 1 || r > DISKANN_R_MAX) return set_error(LYNSE_ERR_UNSUPPORTED, "DiskANN: r must be between 1 and 64");
    if (l < 1 || l > DISKANN_L_MAX) return set_error(LYNSE_ERR_UNSUPPORTED, "DiskANN: l must be between 1 and 4096");
    return LYNSE_OK;
}
static size_t diskann_prune_lds(uint32_t cap, uint32_t D) { return (size_t)cap * 16 + (size_t)D * 8; }   // two key arrays, the rows of p and b

static int diskann_install(lynse_hip_flat* h, uint32_t* d_adj, int metric, uint32_t r, uint32_t l, float alpha, uint64_t n, uint32_t entry) {
    if (!h->diskann) h->diskann = new DiskannState();
    DiskannState& s = *h->diskann;
    s.free_index();
    s.d_adj = d_adj; s.metric = metric; s.r = r; s.l = l; s.alpha = alpha; s.n = n; s.entry = entry;
    return LYNSE_OK;
}

extern "C" int lynse_hip_flat_build_diskann(lynse_hip_flat* h, int metric, uint32_t r, uint32_t l, float alpha, uint32_t max_degree, uint64_t seed,
                                            uint64_t max_batches) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    LY_TRY(diskann_check_metric(metric));
    LY_TRY(diskann_check_params(r, l));
    if (!(alpha >= 1.0f) || !(alpha < LY_INF)) return set_error(LYNSE_ERR_UNSUPPORTED, "DiskANN: alpha must be a finite value >= 1.0");
    (void)max_degree;   // max(max_degree, r) bounds the stored degree min(r, max_degree) = r
    l = std::max(l, r);
    std::unique_lock<std::shared_mutex> lk;
    LY_TRY(graph_lock(h, lk));
    LY_TRY(use_device(h));
    LY_TRY(graph_check_handle(h));
    const uint64_t n = h->n;
    const uint32_t D = h->dim;
    if (n == 0) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "need at least one vector");
    if (n >= 0xffffffffull) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "a DiskANN index holds fewer than 2^32 - 1 rows");
    const uint32_t Lb = std::max(std::min(l, DISKANN_L_BUILD_CAP), r), ef_b = (uint32_t)std::min<uint64_t>(Lb, n);
    const uint32_t cap = r + VAMANA_BATCH;   // the longest list a commit prunes; a forward prune sees at most Lb + r <= 128 + 64
    const size_t s_lds = GraphSearchLds::bytes(ef_b, vamana_c_cap(ef_b), D), p_lds = diskann_prune_lds(cap, D);
    if (std::max(s_lds, p_lds) > PoolRerank::LDS_MAX) return set_error(LYNSE_ERR_UNSUPPORTED, "DiskANN: the vector does not fit in LDS");
    const double t_begin = graph_now_us();
    VamanaDraws dr;
    vamana_draws(seed, n, r, dr);
    const double draws_us = graph_now_us() - t_begin;
    hipStream_t st = cur(h).stream;
    const uint32_t vis_words = (uint32_t)((n + 31) / 32);
    const uint32_t Bmax = (uint32_t)std::min<uint64_t>(VAMANA_BATCH, n);
    uint32_t P = 2;
    while (P < Bmax * r) P <<= 1;
    uint32_t *d_adj = nullptr, *d_order = nullptr, *d_small = nullptr, *d_vis = nullptr, *d_beam_n = nullptr, *d_scored = nullptr, *d_status = nullptr;
    uint64_t *d_beam = nullptr, *d_ckeys = nullptr;
    float* d_pairs = nullptr;
    GraphFree fr;
    fr.ps = {(void**)&d_adj, (void**)&d_order, (void**)&d_small, (void**)&d_vis, (void**)&d_beam_n, (void**)&d_scored, (void**)&d_status,
             (void**)&d_beam, (void**)&d_ckeys, (void**)&d_pairs};
    LY_HIP(hipMalloc(&d_adj, std::max<size_t>((size_t)n * r, 1) * 4));
    LY_TRY(h2d_done(d_adj, dr.adj0.data(), (size_t)n * r * 4));
    LY_HIP(hipMalloc(&d_status, 4));
    LY_TRY(memset_done(d_status, 0, 4));
    // rule 2: the entry point
    uint32_t entry = 0;
    if (n > 1) {
        const uint32_t nr = (uint32_t)dr.refs.size(), nc = (uint32_t)dr.cands.size();
        LY_HIP(hipMalloc(&d_small, (size_t)(nr + nc) * 4));
        LY_HIP(hipMalloc(&d_pairs, (size_t)nr * nc * 4));
        LY_TRY(h2d_done(d_small, dr.refs.data(), (size_t)nr * 4));
        LY_TRY(h2d_done(d_small + nr, dr.cands.data(), (size_t)nc * 4));
        LY_TRY(launch_lds<k_vamana_pairs>(dim3(nc), dim3(64), (size_t)D * 4, st, (const float*)h->rows, h->ld, D, metric, (const uint32_t*)(d_small + nr),
                                          (const uint32_t*)d_small, nr, d_pairs));
        LY_HIP(hipStreamSynchronize(st));
        std::vector<float> pairs((size_t)nr * nc);
        LY_HIP(hipMemcpy(pairs.data(), d_pairs, pairs.size() * 4, hipMemcpyDeviceToHost));
        entry = dr.cands[0];
        float best_sum = LY_INF;
        for (uint32_t c = 0; c < nc; ++c) {
            float sum = 0.0f;
            for (uint32_t j = 0; j < nr; ++j) sum += pairs[(size_t)c * nr + j];
            if (sum < best_sum) { best_sum = sum; entry = dr.cands[c]; }
        }
    }
    // rule 4: the order, the entry first
    {
        auto pos = std::find(dr.order.begin(), dr.order.end(), entry);
        if (pos != dr.order.end()) std::swap(dr.order[0], *pos);
    }
    LY_HIP(hipMalloc(&d_order, (size_t)n * 4));
    LY_TRY(h2d_done(d_order, dr.order.data(), (size_t)n * 4));
    LY_HIP(hipMalloc(&d_vis, (size_t)Bmax * vis_words * 4));
    LY_HIP(hipMalloc(&d_beam, (size_t)Bmax * ef_b * 8));
    LY_HIP(hipMalloc(&d_beam_n, (size_t)Bmax * 4));
    LY_HIP(hipMalloc(&d_scored, (size_t)Bmax * 4));
    LY_HIP(hipMalloc(&d_ckeys, (size_t)P * 8));
    // rule 5: a batch is four launches and a clear on one stream; the host waits once, at the end (per stage with profiling on)
    const bool timed = h->profiling.load();
    double st_us[3] = {0.0, 0.0, 0.0};
    const int passes = alpha > 1.0f + 1.1920929e-7f ? 2 : 1;   // (f32::EPSILON)
    uint64_t batches = 0;
    bool stop = false;
    for (int pass = 0; pass < passes && !stop; ++pass) {
        const float al = pass == 0 ? 1.0f : alpha;
        for (uint64_t b0 = 0; b0 < n && !stop; b0 += VAMANA_BATCH) {
            const uint32_t B = (uint32_t)std::min<uint64_t>(VAMANA_BATCH, n - b0);
            double t0 = timed ? graph_now_us() : 0.0;
            LY_HIP(hipMemsetAsync(d_vis, 0, (size_t)B * vis_words * 4, st));
            VamanaSearchArgs sa{};
            sa.V = h->rows; sa.ld = h->ld; sa.D = D; sa.metric = metric; sa.Q = nullptr; sa.qids = d_order + b0; sa.k = 0; sa.ef = ef_b; sa.r = r;
            sa.anchors = DISKANN_BUILD_ANCHORS; sa.entry = entry; sa.n = n; sa.adj = d_adj; sa.vis = d_vis; sa.vis_words = vis_words;
            sa.out_beam = d_beam; sa.out_beam_n = d_beam_n; sa.out_scored = d_scored; sa.status = d_status;
            LY_TRY(launch_lds<k_vamana_search>(dim3(B), dim3(64), s_lds, st, sa));
            if (timed) { LY_HIP(hipStreamSynchronize(st)); const double t1 = graph_now_us(); st_us[0] += t1 - t0; t0 = t1; }
            VamanaPruneArgs pa{};
            pa.V = h->rows; pa.ld = h->ld; pa.D = D; pa.metric = metric; pa.r = r; pa.cap = cap; pa.alpha = al; pa.adj = d_adj; pa.items = d_order + b0;
            pa.beam = d_beam; pa.beam_n = d_beam_n; pa.beam_stride = ef_b;
            LY_TRY(launch_lds<k_vamana_prune>(dim3(B), dim3(64), p_lds, st, pa));
            if (timed) { LY_HIP(hipStreamSynchronize(st)); const double t1 = graph_now_us(); st_us[1] += t1 - t0; t0 = t1; }
            uint32_t Pb = 2;
            while (Pb < B * r) Pb <<= 1;
            VamanaCommitArgs ca{};
            ca.adj = d_adj; ca.r = r; ca.B = B; ca.P = Pb; ca.items = d_order + b0; ca.ckeys = d_ckeys;
            LY_TRY(launch_lds<k_vamana_commit>(dim3(1), dim3(1024), (size_t)Pb * 8, st, ca));
            pa.ckeys = d_ckeys; pa.n_ckeys = Pb; pa.beam = nullptr; pa.beam_n = nullptr;
            LY_TRY(launch_lds<k_vamana_prune>(dim3(Pb), dim3(64), p_lds, st, pa));   // every slot: a wave that heads no over-long run exits at once
            if (timed) { LY_HIP(hipStreamSynchronize(st)); st_us[2] += graph_now_us() - t0; }
            stop = ++batches == max_batches;
        }
    }
    LY_HIP(hipStreamSynchronize(st));
    uint32_t status = 0;
    LY_HIP(hipMemcpy(&status, d_status, 4, hipMemcpyDeviceToHost));
    if (status) return set_error(LYNSE_ERR_INTERNAL, "DiskANN: the candidate set outgrew its 2 ef + 41 slots");
    LY_TRY(diskann_install(h, d_adj, metric, r, l, alpha, n, entry));
    d_adj = nullptr;
    DiskannState& s = *h->diskann;
    s.b_search_us = st_us[0]; s.b_prune_us = st_us[1]; s.b_commit_us = st_us[2]; s.b_draws_us = draws_us; s.b_total_us = graph_now_us() - t_begin;
    return LYNSE_OK;
}

// A graph as diskann_params exports it.  Pads inside a list and a neighbour named twice are dropped (first place kept): neither
// changes a search — the second visit of a node is skipped.
extern "C" int lynse_hip_flat_load_diskann(lynse_hip_flat* h, int metric, uint32_t r, uint32_t l, const uint32_t* adj, uint64_t n,
                                           uint32_t entry) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    LY_TRY(diskann_check_metric(metric));
    LY_TRY(diskann_check_params(r, l));
    l = std::max(l, r);
    std::unique_lock<std::shared_mutex> lk;
    LY_TRY(graph_lock(h, lk));
    LY_TRY(use_device(h));
    LY_TRY(graph_check_handle(h));
    if (n == 0) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "need at least one vector");
    if (n >= 0xffffffffull) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "a DiskANN index holds fewer than 2^32 - 1 rows");
    if (n > h->n) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "the DiskANN index covers more rows than the handle holds");
    if (!adj) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    if (entry >= n) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "DiskANN: the entry point is beyond the rows of the graph");
    if (GraphSearchLds::bytes(1, vamana_c_cap(1), h->dim) > PoolRerank::LDS_MAX) return set_error(LYNSE_ERR_UNSUPPORTED, "DiskANN: the vector does not fit in LDS");
    std::vector<uint32_t> lists((size_t)n * r, GRAPH_PAD);
    for (uint64_t i = 0; i < n; ++i)
        LY_TRY(graph_take_list(adj + (size_t)i * r, r, n, "DiskANN: a neighbour beyond the rows of the graph", &lists[(size_t)i * r]));
    uint32_t* d_adj = nullptr;
    LY_HIP(hipMalloc(&d_adj, lists.size() * 4));
    const int rc = h2d_done(d_adj, lists.data(), lists.size() * 4);
    if (rc != LYNSE_OK) { (void)hipFree(d_adj); return rc; }
    return diskann_install(h, d_adj, metric, r, l, 0.0f, n, entry);   // (alpha belongs to a build: a loaded graph reports 0)
}

// info = {metric, r, l, entry}, all 0 (and alpha, n_diskann 0) without an index
extern "C" int lynse_hip_flat_diskann_params(lynse_hip_flat* h, uint32_t* info, float* alpha, uint64_t* n_diskann, uint32_t* adj) {
    if (!h || !info || !alpha || !n_diskann) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    std::shared_lock<std::shared_mutex> lk(h->rw);
    if (!h->diskann || !h->diskann->built()) {
        for (int i = 0; i < 4; ++i) info[i] = 0;
        *alpha = 0.0f;
        *n_diskann = 0;
        return LYNSE_OK;
    }
    const DiskannState& s = *h->diskann;
    info[0] = (uint32_t)s.metric; info[1] = s.r; info[2] = s.l; info[3] = s.entry;
    *alpha = s.alpha;
    *n_diskann = s.n;
    LY_TRY(use_device(h));
    if (adj) LY_HIP(hipMemcpy(adj, s.d_adj, (size_t)s.n * s.r * 4, hipMemcpyDeviceToHost));
    return LYNSE_OK;
}

extern "C" int lynse_hip_flat_drop_diskann(lynse_hip_flat* h) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    LY_WRITER(h, lk);
    LY_TRY(use_device(h));
    if (h->diskann) h->diskann->free_index();
    return LYNSE_OK;
}

// out8 = the last build: {search, prune, commit} microseconds (a build with profiling on waits after every stage and times it on the
// host clock; otherwise 0), host random draws, the whole build; then with profiling on: searches timed, their kernel microseconds
// (HIP events) and the distances they scored
extern "C" int lynse_hip_flat_diskann_stage_times(lynse_hip_flat* h, double* out8, int reset) {
    if (!h || !out8) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    LY_WRITER(h, lk);
    if (!h->diskann) { for (int i = 0; i < 8; ++i) out8[i] = 0.0; return LYNSE_OK; }
    DiskannState& s = *h->diskann;
    out8[0] = s.b_search_us; out8[1] = s.b_prune_us; out8[2] = s.b_commit_us; out8[3] = s.b_draws_us; out8[4] = s.b_total_us;
    out8[5] = s.search.searches; out8[6] = s.search.search_us; out8[7] = s.search.scored;
    if (reset) s.search.searches = s.search.search_us = s.search.scored = 0.0;
    return LYNSE_OK;
}

// rule 8; graph_search (graph_host.inc) runs the queries in chunks
extern "C" int lynse_hip_flat_search_diskann_f32(lynse_hip_flat* h, const float* queries, uint64_t nq, uint32_t k, int metric, uint32_t ef_query,
                                                 uint64_t* out_rows, float* out_dists, uint32_t* out_counts) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    LY_TRY(diskann_check_metric(metric));
    if (nq == 0) return LYNSE_OK;
    if (!queries || !out_counts || (k && (!out_rows || !out_dists))) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    std::unique_lock<std::shared_mutex> lk;
    LY_TRY(graph_lock(h, lk));
    LY_TRY(use_device(h));
    LY_TRY(graph_check_handle(h));
    if (!h->diskann || !h->diskann->built()) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "no DiskANN index on this handle: build or load one first");
    DiskannState& s = *h->diskann;
    if (metric != s.metric) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "the DiskANN index was built for another metric");
    if (ef_query > DISKANN_L_MAX) return set_error(LYNSE_ERR_UNSUPPORTED, "DiskANN: ef must be between 1 and 4096");
    if (k == 0) { memset(out_counts, 0, nq * 4); return LYNSE_OK; }
    const uint32_t ef = (uint32_t)std::min<uint64_t>(std::max<uint64_t>({(uint64_t)ef_query, (uint64_t)s.l, 10ull * k}), s.n);
    const size_t lds = GraphSearchLds::bytes(ef, vamana_c_cap(ef), h->dim);
    if (lds > PoolRerank::LDS_MAX) return set_error(LYNSE_ERR_UNSUPPORTED, "DiskANN: the beam (24 bytes per ef, ef >= 10 k) and the query do not fit in LDS");
    return graph_search(h, s.search, s.n, lds, "DiskANN: the candidate set outgrew its 2 ef + 41 slots", queries, nq, k, out_rows, out_dists, out_counts,
                        [&](const GraphSearchChunk& c) {
        VamanaSearchArgs a{};
        a.V = h->rows; a.ld = h->ld; a.D = h->dim; a.metric = metric; a.Q = c.Q; a.k = k; a.ef = ef; a.r = s.r; a.anchors = DISKANN_QUERY_ANCHORS;
        a.entry = s.entry; a.n = s.n; a.adj = s.d_adj; a.vis = c.vis; a.vis_words = c.vis_words; a.out_rows = c.out_rows; a.out_dists = c.out_dists;
        a.out_counts = c.out_counts; a.out_scored = c.out_scored; a.status = c.status;
        return launch_lds<k_vamana_search>(dim3(c.nqc), dim3(64), c.lds, c.st, a);
    });
}
