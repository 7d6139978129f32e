// hnsw_host.inc — HNSW-{IP,L2,COS} on a FLAT handle (HNSWIndex, src/index/hnsw.rs; Collection, src/engine.rs:4606-4655, :4743-4745).
// Included at the end of lynse_hip.hip after rabitq_host.inc (the SmallRng restatement is pqrng) and graph_host.inc, whose lock, handle
// check, clock, list normaliser and search driver it shares with diskann_host.inc; kernels in hnsw.h.  The rule block of
// include/lynse_hip.h states the contract, DESIGN.md §19 the reasoning.  The graph shares the handle's rows: it holds ids only.

// What a build keeps of one level for lynse_hip_flat_hnsw_extend (rule 7), in host memory: the members S_l, their forward lists with
// the graph distances (what rule 4 is a function of) and one threshold each.  New rows have the highest row numbers, so an extend
// appends to every array and the item index of an old member never moves.
struct HnswLevelKeep {
    std::vector<uint32_t> items;   // S_l ascending; empty at level 0, where item t is row t
    std::vector<uint32_t> fid;     // [|S_l|][cap] F_l(i) in selection order, GRAPH_PAD after the last
    std::vector<float> fd;         // d(i, fid)
    std::vector<float> thr;        // [|S_l|] the raw score of the last of the ef_construction + 1 entries the exact search returned; NaN = short
};

struct HnswState {
    int metric = -1;
    uint32_t m = 0, ef_search = 0, entry = 0, top_level = 0;
    uint64_t n = 0;                       // the graph covers the first n rows of the handle
    std::vector<uint32_t> levels;         // [n]
    std::vector<uint32_t> upper_node, upper_level;   // ascending (node, level), levels >= 1
    uint32_t *d_adj0 = nullptr, *d_upper_off = nullptr, *d_upper_adj = nullptr;
    // a built graph (not a loaded one) can be extended: the parameters of rule 1-3 and the levels' forward lists
    bool extendable = false;
    uint32_t ef_construction = 0;
    int32_t max_level = -1;
    uint64_t seed = 0;
    std::vector<HnswLevelKeep> keep;      // [top_level + 1]
    double ext[12] = {0.0};               // lynse_hip_flat_hnsw_extend_stats
    GraphSearchScratch search;            // with the searches timed with profiling on
    // the last build, microseconds of host time around synchronised stages
    double cand_us = 0.0, select_us = 0.0, reverse_us = 0.0;

    bool built() const { return d_adj0 != nullptr; }
    void free_device() {
        for (void* p : {(void*)d_adj0, (void*)d_upper_off, (void*)d_upper_adj})
            if (p) (void)hipFree(p);
        d_adj0 = d_upper_off = d_upper_adj = nullptr;
    }
    void drop_keep() {
        extendable = false;
        ef_construction = 0; max_level = -1; seed = 0;
        std::vector<HnswLevelKeep>().swap(keep);
    }
    void free_index() {
        free_device();
        drop_keep();
        levels.clear(); upper_node.clear(); upper_level.clear();
        metric = -1;
        m = ef_search = entry = top_level = 0;
        n = 0;
    }
    ~HnswState() { free_index(); }
};

static void hnsw_release(lynse_hip_flat* h) {
    delete h->hnsw;
    h->hnsw = nullptr;
}

constexpr uint32_t HNSW_M_MIN = 2, HNSW_M_MAX = 32, HNSW_EF_MAX = 4096, HNSW_LEVEL_MAX = 52;   // t * m < 2^53 with m >= 2 ends at 52

// rule 1: level i from the i-th next_u64 of SmallRng::seed_from_u64(seed), integers only; max_level < 0 = no cap
static void hnsw_levels(uint64_t seed, uint32_t m, int32_t max_level, uint64_t n, uint32_t* out) {
    pqrng::Xoshiro256pp rng = pqrng::Xoshiro256pp::seed_from_u64(seed);
    for (uint64_t i = 0; i < n; ++i) {
        uint64_t t = std::max<uint64_t>(rng.next() >> 11, 1);
        uint32_t level = 0;
        while ((max_level < 0 || level < (uint32_t)max_level) && t * m < (1ull << 53)) { t *= m; ++level; }
        out[i] = level;
    }
}

extern "C" int lynse_hip_hnsw_levels(uint64_t seed, uint32_t m, int32_t max_level, uint64_t n, uint32_t* out) {
    if (n && !out) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    if (m < HNSW_M_MIN || m > HNSW_M_MAX) return set_error(LYNSE_ERR_UNSUPPORTED, "HNSW: m must be between 2 and 32");
    hnsw_levels(seed, m, max_level, n, out);
    return LYNSE_OK;
}

static int hnsw_check_metric(int metric) {
    LY_TRY(metric_check(metric));
    if (metric_binary(metric)) return set_error(LYNSE_ERR_UNSUPPORTED, "HNSW is defined for ip / l2 / cosine");
    return LYNSE_OK;
}
static int hnsw_check_params(uint32_t m, uint32_t ef_construction, uint32_t ef_search) {
    if (m < HNSW_M_MIN || m > HNSW_M_MAX) return set_error(LYNSE_ERR_UNSUPPORTED, "HNSW: m must be between 2 and 32");
    if (ef_construction < 1 || ef_construction > HNSW_EF_MAX) return set_error(LYNSE_ERR_UNSUPPORTED, "HNSW: ef_construction must be between 1 and 4096");
    if (ef_search < 1 || ef_search > HNSW_EF_MAX) return set_error(LYNSE_ERR_UNSUPPORTED, "HNSW: ef_search must be between 1 and 4096");
    return LYNSE_OK;
}
// A graph on the host: adj0[n][2 m], upper lists in ascending (node, level) order.  Installing uploads it.
struct HnswGraph {
    uint32_t m = 0, entry = 0, top_level = 0;
    uint64_t n = 0;
    std::vector<uint32_t> levels, adj0, upper_off, upper_node, upper_level, upper_adj;
    void shape(uint32_t mm, const uint32_t* lv, uint64_t nn) {
        m = mm; n = nn;
        levels.assign(lv, lv + nn);
        upper_off.assign(nn, GRAPH_PAD);
        uint64_t nu = 0;
        top_level = 0;
        for (uint64_t i = 0; i < nn; ++i) {
            if (lv[i]) upper_off[i] = (uint32_t)nu;
            for (uint32_t l = 1; l <= lv[i]; ++l) { upper_node.push_back((uint32_t)i); upper_level.push_back(l); }
            nu += lv[i];
            top_level = std::max(top_level, lv[i]);
        }
        for (uint64_t i = 0; i < nn; ++i)
            if (lv[i] == top_level) { entry = (uint32_t)i; break; }   // the first row of the highest level (hnsw.rs:967-975)
        adj0.assign((size_t)nn * 2 * mm, GRAPH_PAD);
        upper_adj.assign((size_t)nu * mm, GRAPH_PAD);
    }
    uint32_t* list(uint32_t node, uint32_t level) {
        return level == 0 ? &adj0[(size_t)node * 2 * m] : &upper_adj[((size_t)upper_off[node] + level - 1) * m];
    }
};

// Uploads first and replaces the earlier graph only then: a failed install leaves it as it was.  The forward lists a build kept are
// the caller's: a load drops them (keep_forward false), build and extend put theirs in place afterwards.
static int hnsw_install(lynse_hip_flat* h, HnswGraph& gph, int metric, uint32_t ef_search, bool keep_forward) {
    if (!h->hnsw) h->hnsw = new HnswState();
    HnswState& s = *h->hnsw;
    uint32_t *d_adj0 = nullptr, *d_off = nullptr, *d_up = nullptr;
    auto fail = [&](int rc) {
        for (void* p : {(void*)d_adj0, (void*)d_off, (void*)d_up})
            if (p) (void)hipFree(p);
        return rc;
    };
    auto up = [&](uint32_t** d, const std::vector<uint32_t>& v) -> int {
        LY_HIP(hipMalloc(d, std::max<size_t>(v.size(), 1) * 4));
        if (!v.empty()) LY_TRY(h2d_done(*d, v.data(), v.size() * 4));
        return LYNSE_OK;
    };
    int rc = up(&d_adj0, gph.adj0);
    if (rc == LYNSE_OK) rc = up(&d_off, gph.upper_off);
    if (rc == LYNSE_OK) rc = up(&d_up, gph.upper_adj);
    if (rc != LYNSE_OK) return fail(rc);
    s.free_device();
    if (!keep_forward) s.drop_keep();
    s.metric = metric; s.m = gph.m; s.ef_search = ef_search; s.entry = gph.entry; s.top_level = gph.top_level; s.n = gph.n;
    s.levels.swap(gph.levels); s.upper_node.swap(gph.upper_node); s.upper_level.swap(gph.upper_level);
    s.d_adj0 = d_adj0; s.d_upper_off = d_off; s.d_upper_adj = d_up;
    return LYNSE_OK;
}

// One level while it is built or extended: its members, and the stages build and extend share.
struct HnswLevelJob {
    lynse_hip_flat* h;
    int metric;
    uint32_t level, m, ef_construction;
    uint64_t n;                          // rows the graph covers once the job is done
    const uint32_t* items;               // S_l ascending (NULL at level 0: item t is row t)
    uint32_t ns;                         // |S_l|
    std::vector<uint64_t> words;         // the BitSet of S_l above level 0
    std::vector<uint32_t> item_of;       // node -> item above level 0
    double* times3;                      // candidate lists, selection, reverse edges (microseconds)

    uint32_t cap() const { return level == 0 ? 2 * m : m; }
    uint32_t node(uint32_t t) const { return items ? items[t] : t; }
    uint32_t item(uint32_t nd) const { return items ? item_of[nd] : nd; }
    void index_members() {
        if (!items) return;
        words.assign((n + 63) / 64, 0ull);
        item_of.assign(n, GRAPH_PAD);
        for (uint32_t t = 0; t < ns; ++t) {
            words[items[t] >> 6] |= 1ull << (items[t] & 63u);
            item_of[items[t]] = t;
        }
    }
};

// Rules 2-3 for the members `q_nodes` of the level: their exact candidate lists over S_l, then the heuristic.  fid / fd: [nq][cap],
// thr: [nq] (rule 7), all on the host.
static int hnsw_level_forward(const HnswLevelJob& jb, const uint32_t* q_nodes, uint32_t nq, uint32_t* fid, float* fd, float* thr) {
    lynse_hip_flat* h = jb.h;
    const uint32_t cap = jb.cap(), D = h->dim, ask = jb.ef_construction + 1, level = jb.level;
    if (nq == 0) return LYNSE_OK;
    hipStream_t st = cur(h).stream;
    uint32_t* d_items = nullptr;
    float *d_q = nullptr, *d_cd = nullptr, *d_fd = nullptr, *d_thr = nullptr;
    uint64_t* d_cr = nullptr;
    uint32_t *d_cc = nullptr, *d_fid = nullptr;
    GraphFree fr;
    fr.ps = {(void**)&d_items, (void**)&d_q, (void**)&d_cd, (void**)&d_fd, (void**)&d_thr, (void**)&d_cr, (void**)&d_cc, (void**)&d_fid};
    LY_HIP(hipMalloc(&d_items, (size_t)nq * 4));
    LY_TRY(h2d_done(d_items, q_nodes, (size_t)nq * 4));
    // queries per pass: the candidate lists of a pass stay under 256 MiB, its queries under 128 MiB
    const uint64_t qc = std::max<uint64_t>(1, std::min<uint64_t>({(uint64_t)nq, (256ull << 20) / ((uint64_t)ask * 12), (128ull << 20) / ((uint64_t)D * 4)}));
    LY_HIP(hipMalloc(&d_q, (size_t)qc * D * 4));
    LY_HIP(hipMalloc(&d_cr, (size_t)qc * ask * 8));
    LY_HIP(hipMalloc(&d_cd, (size_t)qc * ask * 4));
    LY_HIP(hipMalloc(&d_cc, (size_t)qc * 4));
    LY_HIP(hipMalloc(&d_fid, (size_t)nq * cap * 4));
    LY_HIP(hipMalloc(&d_fd, (size_t)nq * cap * 4));
    LY_HIP(hipMalloc(&d_thr, (size_t)nq * 4));
    const size_t sel_lds = 512 + (size_t)D * 4;
    for (uint64_t q0 = 0; q0 < nq; q0 += qc) {
        const uint64_t nqc = std::min<uint64_t>(qc, nq - q0);
        double t0 = graph_now_us();
        hipLaunchKernelGGL(k_hnsw_gather, dim3((uint32_t)std::min<uint64_t>((nqc * D + 255) / 256, (uint64_t)h->num_cu * 32)), dim3(256), 0, st,
                           h->rows, h->ld, D, d_items + q0, 0u, nqc, d_q);
        LY_HIP(hipGetLastError());
        LY_HIP(hipStreamSynchronize(st));
        // rule 2: the exact searches of the handle, single-row kernels (the caller pinned the SINGLE ip form), canonical (d, row) order
        LY_TRY(search_impl(h, d_q, false, nqc, ask, jb.metric, d_cr, d_cd, d_cc, true, nullptr, nullptr, level > 0 ? (uint64_t)jb.ns : 0, level > 0,
                           level > 0 ? jb.words.data() : nullptr, jb.words.size(), true));
        LY_HIP(hipStreamSynchronize(st));
        double t1 = graph_now_us();
        jb.times3[0] += t1 - t0;
        // rule 3: the forward lists
        HnswSelectArgs sa{};
        sa.V = h->rows; sa.ld = h->ld; sa.D = D; sa.metric = jb.metric; sa.cap = cap;
        sa.item_node = d_items + q0; sa.rows64 = d_cr; sa.d64 = d_cd; sa.cnt64 = d_cc; sa.stride = ask;
        sa.out_ids = d_fid + q0 * cap; sa.out_d = d_fd + q0 * cap; sa.out_thr = d_thr + q0;
        LY_TRY(launch_lds<k_hnsw_select>(dim3((uint32_t)nqc), dim3(64), sel_lds, st, sa));
        LY_HIP(hipStreamSynchronize(st));
        jb.times3[1] += graph_now_us() - t1;
    }
    double t2 = graph_now_us();
    LY_HIP(hipMemcpy(fid, d_fid, (size_t)nq * cap * 4, hipMemcpyDeviceToHost));
    LY_HIP(hipMemcpy(fd, d_fd, (size_t)nq * cap * 4, hipMemcpyDeviceToHost));
    LY_HIP(hipMemcpy(thr, d_thr, (size_t)nq * 4, hipMemcpyDeviceToHost));
    jb.times3[2] += graph_now_us() - t2;
    return LYNSE_OK;
}

// Rule 4 for the items with dirty[t] != 0 (dirty NULL: every item), from the level's forward lists fid / fd [ns][cap]: U(i) = F(i) and
// the reverse edges, each member once, ordered by (d, node) — as keys, so one integer sort per node.  Fills their lists of `gph`;
// *reselected counts the lists that went through the heuristic again.
static int hnsw_level_adjacency(const HnswLevelJob& jb, HnswGraph& gph, const uint32_t* fid, const float* fd, const uint8_t* dirty, uint64_t* reselected) {
    lynse_hip_flat* h = jb.h;
    const uint32_t ns = jb.ns, cap = jb.cap(), D = h->dim, level = jb.level;
    hipStream_t st = cur(h).stream;
    uint32_t *d_uid = nullptr, *d_oid = nullptr; float *d_ud = nullptr, *d_od = nullptr; uint64_t* d_uoff = nullptr;
    GraphFree fr;
    fr.ps = {(void**)&d_uid, (void**)&d_ud, (void**)&d_uoff, (void**)&d_oid, (void**)&d_od};
    double t2 = graph_now_us();
    auto want = [&](uint32_t t) { return !dirty || dirty[t]; };
    std::vector<uint64_t> off((size_t)ns + 1, 0);
    for (uint32_t t = 0; t < ns; ++t)
        for (uint32_t s = 0; s < cap && fid[(size_t)t * cap + s] != GRAPH_PAD; ++s) {
            if (want(t)) ++off[t + 1];
            const uint32_t jt = jb.item(fid[(size_t)t * cap + s]);
            if (want(jt)) ++off[jt + 1];
        }
    for (uint32_t t = 0; t < ns; ++t) off[t + 1] += off[t];
    std::vector<uint64_t> keys(off[ns]), fill(off.begin(), off.end() - 1);
    for (uint32_t t = 0; t < ns; ++t)
        for (uint32_t s = 0; s < cap && fid[(size_t)t * cap + s] != GRAPH_PAD; ++s) {
            const uint32_t j = fid[(size_t)t * cap + s], jt = jb.item(j);
            const float d = fd[(size_t)t * cap + s];
            if (want(t)) keys[fill[t]++] = make_key(d, j, true);
            if (want(jt)) keys[fill[jt]++] = make_key(d, jb.node(t), true);   // d(j, i) = d(i, j) bit for bit (rule block: symmetric forms)
        }
    std::vector<uint64_t> uoff(1, 0);
    std::vector<uint32_t> over, uid;
    std::vector<float> ud;
    for (uint32_t t = 0; t < ns; ++t) {
        if (!want(t)) continue;
        uint64_t* b = keys.data() + off[t];
        uint64_t* e = keys.data() + off[t + 1];
        std::sort(b, e);
        e = std::unique(b, e);
        const size_t cnt = (size_t)(e - b);
        uint32_t* dst = gph.list(jb.node(t), level);
        if (cnt <= cap) {
            for (size_t s = 0; s < cap; ++s) dst[s] = s < cnt ? key_row(b[s]) : GRAPH_PAD;
        } else {   // more than cap: the heuristic again, over U(i)
            over.push_back(t);
            for (size_t s = 0; s < cnt; ++s) { uid.push_back(key_row(b[s])); ud.push_back(key_score(b[s], true)); }
            uoff.push_back(uid.size());
        }
    }
    jb.times3[2] += graph_now_us() - t2;
    if (!over.empty()) {
        double t3 = graph_now_us();
        const size_t no = over.size();
        LY_HIP(hipMalloc(&d_uid, uid.size() * 4));
        LY_HIP(hipMalloc(&d_ud, ud.size() * 4));
        LY_HIP(hipMalloc(&d_uoff, uoff.size() * 8));
        LY_HIP(hipMalloc(&d_oid, no * cap * 4));
        LY_HIP(hipMalloc(&d_od, no * cap * 4));
        LY_TRY(h2d_done(d_uid, uid.data(), uid.size() * 4));
        LY_TRY(h2d_done(d_ud, ud.data(), ud.size() * 4));
        LY_TRY(h2d_done(d_uoff, uoff.data(), uoff.size() * 8));
        HnswSelectArgs sa{};
        sa.V = h->rows; sa.ld = h->ld; sa.D = D; sa.metric = jb.metric; sa.cap = cap;
        sa.ids32 = d_uid; sa.d32 = d_ud; sa.offs = d_uoff; sa.out_ids = d_oid; sa.out_d = d_od;
        LY_TRY(launch_lds<k_hnsw_select>(dim3((uint32_t)no), dim3(64), 512 + (size_t)D * 4, st, sa));
        LY_HIP(hipStreamSynchronize(st));
        std::vector<uint32_t> oid(no * cap);
        LY_HIP(hipMemcpy(oid.data(), d_oid, oid.size() * 4, hipMemcpyDeviceToHost));
        for (size_t o = 0; o < no; ++o) memcpy(gph.list(jb.node(over[o]), level), &oid[o * cap], (size_t)cap * 4);
        jb.times3[1] += graph_now_us() - t3;
        if (reselected) *reselected += no;
    }
    return LYNSE_OK;
}

// the refusals of a graph over the handle's rows as they are now, shared by build and extend
static int hnsw_check_rows(const lynse_hip_flat* h, uint32_t ef_construction) {
    const uint64_t n = h->n;
    if (n == 0) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "need at least one vector");
    if (n >= 0xffffffffull) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "an HNSW index holds fewer than 2^32 - 1 rows");
    if ((size_t)h->dim * 4 + 512 > PoolRerank::LDS_MAX) return set_error(LYNSE_ERR_UNSUPPORTED, "HNSW: the vector does not fit in LDS");
    if (n > h->cap && ef_construction + 1 > h->cap / 4)
        return set_error(LYNSE_ERR_UNSUPPORTED, "HNSW: ef_construction + 1 beyond a quarter of the scan's candidate capacity over a shard larger than it");
    return LYNSE_OK;
}

// every distance of a build or an extend is the single-row form (rule block): the exact searches follow the handle's ip form
struct HnswFormGuard {
    lynse_hip_flat* h; int f;
    explicit HnswFormGuard(lynse_hip_flat* hh) : h(hh), f(hh->ip_form) { h->ip_form = LYNSE_IPFORM_SINGLE; }
    ~HnswFormGuard() { h->ip_form = f; }
};

// The bulk build under the caller's lock, on context 0.  A failure leaves an earlier graph as it was.
static int hnsw_build_locked(lynse_hip_flat* h, int metric, uint32_t m, uint32_t ef_construction, uint32_t ef_search, int32_t max_level, uint64_t seed) {
    LY_TRY(hnsw_check_rows(h, ef_construction));
    const uint64_t n = h->n;
    std::vector<uint32_t> lv(n);
    hnsw_levels(seed, m, max_level, n, lv.data());
    HnswGraph gph;
    gph.shape(m, lv.data(), n);
    HnswFormGuard form_guard(h);
    double times3[3] = {0.0, 0.0, 0.0};
    std::vector<HnswLevelKeep> keep(gph.top_level + 1);
    for (uint32_t level = 0; level <= gph.top_level; ++level) {
        HnswLevelKeep& kp = keep[level];
        if (level > 0)
            for (uint64_t i = 0; i < n; ++i)
                if (lv[i] >= level) kp.items.push_back((uint32_t)i);
        HnswLevelJob jb{h, metric, level, m, ef_construction, n, level > 0 ? kp.items.data() : nullptr, (uint32_t)(level > 0 ? kp.items.size() : n), {}, {}, times3};
        kp.fid.assign((size_t)jb.ns * jb.cap(), GRAPH_PAD);
        kp.fd.assign((size_t)jb.ns * jb.cap(), INFINITY);
        kp.thr.assign(jb.ns, NAN);
        if (jb.ns <= 1) continue;   // a node alone on its level has no candidates
        jb.index_members();
        std::vector<uint32_t> all;
        if (level == 0) { all.resize(n); for (uint64_t i = 0; i < n; ++i) all[i] = (uint32_t)i; }
        LY_TRY(hnsw_level_forward(jb, level > 0 ? kp.items.data() : all.data(), jb.ns, kp.fid.data(), kp.fd.data(), kp.thr.data()));
        LY_TRY(hnsw_level_adjacency(jb, gph, kp.fid.data(), kp.fd.data(), nullptr, nullptr));
    }
    LY_TRY(hnsw_install(h, gph, metric, ef_search, false));
    HnswState& s = *h->hnsw;
    s.keep.swap(keep);
    s.extendable = true; s.ef_construction = ef_construction; s.max_level = max_level; s.seed = seed;
    s.cand_us = times3[0]; s.select_us = times3[1]; s.reverse_us = times3[2];
    return LYNSE_OK;
}

extern "C" int lynse_hip_flat_build_hnsw(lynse_hip_flat* h, int metric, uint32_t m, uint32_t ef_construction, uint32_t ef_search,
                                         int32_t max_level, uint64_t seed) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    LY_TRY(hnsw_check_metric(metric));
    LY_TRY(hnsw_check_params(m, ef_construction, ef_search));
    std::unique_lock<std::shared_mutex> lk;
    LY_TRY(graph_lock(h, lk));
    LY_TRY(use_device(h));
    LY_TRY(graph_check_handle(h));
    return hnsw_build_locked(h, metric, m, ef_construction, ef_search, max_level, seed);
}

// An undo log of an extend: the kept levels are changed in place and put back unless the new graph was installed.
struct HnswExtendUndo {
    HnswState& s;
    size_t n_levels;
    struct Lv { uint32_t level, cap; size_t ns0; std::vector<uint32_t> idx, fid; std::vector<float> fd, thr; };
    std::vector<Lv> lv;
    bool committed = false;
    explicit HnswExtendUndo(HnswState& ss) : s(ss), n_levels(ss.keep.size()) {}
    ~HnswExtendUndo() {
        if (committed) return;
        for (const Lv& u : lv) {
            if (u.level >= n_levels) continue;
            HnswLevelKeep& kp = s.keep[u.level];
            for (size_t x = 0; x < u.idx.size(); ++x) {
                memcpy(&kp.fid[(size_t)u.idx[x] * u.cap], &u.fid[x * u.cap], (size_t)u.cap * 4);
                memcpy(&kp.fd[(size_t)u.idx[x] * u.cap], &u.fd[x * u.cap], (size_t)u.cap * 4);
                kp.thr[u.idx[x]] = u.thr[x];
            }
            if (u.level > 0) kp.items.resize(u.ns0);
            kp.fid.resize(u.ns0 * u.cap); kp.fd.resize(u.ns0 * u.cap); kp.thr.resize(u.ns0);
        }
        s.keep.resize(n_levels);
    }
};

// rule 7 step b: the old members of the level a new row may enter the candidate list of
static int hnsw_reverse_scan(const HnswLevelJob& jb, uint32_t ns0, const float* thr, std::vector<uint8_t>& flags) {
    lynse_hip_flat* h = jb.h;
    const uint32_t D = h->dim, nn = jb.ns - ns0;
    flags.assign(ns0, 0);
    if (ns0 == 0 || nn == 0) return LYNSE_OK;
    hipStream_t st = cur(h).stream;
    uint32_t *d_old = nullptr, *d_new = nullptr; float* d_thr = nullptr; uint8_t* d_flags = nullptr;
    GraphFree fr;
    fr.ps = {(void**)&d_old, (void**)&d_new, (void**)&d_thr, (void**)&d_flags};
    std::vector<uint32_t> new_ids(nn);
    for (uint32_t t = 0; t < nn; ++t) new_ids[t] = jb.node(ns0 + t);
    if (jb.items) {
        LY_HIP(hipMalloc(&d_old, (size_t)ns0 * 4));
        LY_TRY(h2d_done(d_old, jb.items, (size_t)ns0 * 4));
    }
    LY_HIP(hipMalloc(&d_new, (size_t)nn * 4));
    LY_TRY(h2d_done(d_new, new_ids.data(), (size_t)nn * 4));
    LY_HIP(hipMalloc(&d_thr, (size_t)ns0 * 4));
    LY_TRY(h2d_done(d_thr, thr, (size_t)ns0 * 4));
    LY_HIP(hipMalloc(&d_flags, ns0));
    LY_HIP(hipMemsetAsync(d_flags, 0, ns0, st));
    // new rows per tile: what fits the 160 KiB of the graph kernels, never fewer than one (4 D + 512 fits: hnsw_check_rows)
    const uint32_t tile = (uint32_t)std::max<size_t>(1, std::min<size_t>(nn, PoolRerank::LDS_MAX / ((size_t)D * 4)));
    const uint32_t per_block = HNSW_REVERSE_THREADS / 64 * 8;
    const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(((uint64_t)ns0 + per_block - 1) / per_block, (uint64_t)h->num_cu * 4));
    for (uint32_t t0 = 0; t0 < nn; t0 += tile) {
        HnswReverseArgs a{};
        a.V = h->rows; a.ld = h->ld; a.D = D; a.metric = jb.metric; a.old_ids = d_old; a.n_old = ns0; a.thr = d_thr;
        a.new_ids = d_new; a.tile0 = t0; a.tn = std::min(tile, nn - t0); a.flags = d_flags;
        LY_TRY(launch_lds<k_hnsw_reverse_scan>(dim3(grid), dim3(HNSW_REVERSE_THREADS), (size_t)a.tn * D * 4, st, a));
    }
    LY_HIP(hipStreamSynchronize(st));
    LY_HIP(hipMemcpy(flags.data(), d_flags, ns0, hipMemcpyDeviceToHost));
    return LYNSE_OK;
}

// Rule 7: the graph over all h->n rows, equal to a build over them.  ext[] is lynse_hip_flat_hnsw_extend_stats.
extern "C" int lynse_hip_flat_hnsw_extend(lynse_hip_flat* h, int mode) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    if (mode != 0 && mode != 1) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "HNSW extend: mode must be 0 (auto) or 1 (incremental)");
    std::unique_lock<std::shared_mutex> lk;
    LY_TRY(graph_lock(h, lk));
    LY_TRY(use_device(h));
    LY_TRY(graph_check_handle(h));
    if (!h->hnsw || !h->hnsw->built()) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "no HNSW index on this handle: build or load one first");
    HnswState& s = *h->hnsw;
    if (!s.extendable) return set_error(LYNSE_ERR_UNSUPPORTED, "HNSW extend: a loaded graph carries no forward lists: build it on this handle first");
    const uint64_t n0 = s.n, n1 = h->n;
    if (n1 < n0) return set_error(LYNSE_ERR_INTERNAL, "HNSW extend: the graph covers more rows than the handle holds");
    const double t_start = graph_now_us();
    double ext[12] = {(double)n0, (double)n1, 2.0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    auto done = [&]() { ext[11] = graph_now_us() - t_start; memcpy(s.ext, ext, sizeof ext); return LYNSE_OK; };
    if (n1 == n0) return done();
    LY_TRY(hnsw_check_rows(h, s.ef_construction));
    const int metric = s.metric;
    const uint32_t m = s.m, efc = s.ef_construction;
    if (mode == 0 && (n1 - n0) * (uint64_t)efc >= n0) {   // most old rows would be searched again: the plain build (DESIGN §19)
        LY_TRY(hnsw_build_locked(h, metric, m, efc, s.ef_search, s.max_level, s.seed));
        HnswState& b = *h->hnsw;
        ext[2] = 1.0; ext[8] = b.cand_us; ext[9] = b.select_us; ext[10] = b.reverse_us;
        ext[11] = graph_now_us() - t_start;
        memcpy(b.ext, ext, sizeof ext);
        return LYNSE_OK;
    }
    ext[2] = 0.0;
    // a. levels: the first n0 draws are the stored ones (one stream), entry and top level by shape's rule
    std::vector<uint32_t> lv(n1);
    hnsw_levels(s.seed, m, s.max_level, n1, lv.data());
    if (memcmp(lv.data(), s.levels.data(), (size_t)n0 * 4) != 0) return set_error(LYNSE_ERR_INTERNAL, "HNSW extend: the level stream lost its prefix");
    HnswGraph gph;
    gph.shape(m, lv.data(), n1);
    // the old lists are a prefix of the new arrays: new rows have the highest row numbers
    LY_HIP(hipMemcpy(gph.adj0.data(), s.d_adj0, (size_t)n0 * 2 * m * 4, hipMemcpyDeviceToHost));
    if (!s.upper_node.empty()) LY_HIP(hipMemcpy(gph.upper_adj.data(), s.d_upper_adj, s.upper_node.size() * (size_t)m * 4, hipMemcpyDeviceToHost));
    HnswFormGuard form_guard(h);
    HnswExtendUndo undo(s);
    double times3[3] = {0.0, 0.0, 0.0};
    uint64_t reselected = 0;
    std::vector<uint32_t> fresh, q_nodes, q_items, qfid;
    std::vector<float> qfd, qthr;
    std::vector<uint8_t> flags, dirty;
    for (uint32_t level = 0; level <= gph.top_level; ++level) {
        fresh.clear();
        for (uint64_t i = n0; i < n1; ++i)
            if (lv[i] >= level) fresh.push_back((uint32_t)i);
        if (fresh.empty()) break;   // S_l shrinks with l: no level above has a new member either
        if (level >= s.keep.size()) s.keep.resize(level + 1);
        HnswLevelKeep& kp = s.keep[level];
        const uint32_t cap = level == 0 ? 2 * m : m;
        const uint32_t ns0 = (uint32_t)(level == 0 ? n0 : kp.items.size()), ns = ns0 + (uint32_t)fresh.size();
        undo.lv.push_back({level, cap, ns0, {}, {}, {}, {}});
        HnswExtendUndo::Lv& u = undo.lv.back();
        if (level > 0) kp.items.insert(kp.items.end(), fresh.begin(), fresh.end());
        kp.fid.resize((size_t)ns * cap, GRAPH_PAD);
        kp.fd.resize((size_t)ns * cap, INFINITY);
        kp.thr.resize(ns, NAN);
        ext[3] += (double)fresh.size();
        if (ns <= 1) continue;
        HnswLevelJob jb{h, metric, level, m, efc, n1, level > 0 ? kp.items.data() : nullptr, ns, {}, {}, times3};
        jb.index_members();
        // b. the affected old members
        const double ts = graph_now_us();
        LY_TRY(hnsw_reverse_scan(jb, ns0, kp.thr.data(), flags));
        ext[7] += graph_now_us() - ts;
        q_nodes.clear(); q_items.clear();
        for (uint32_t t = 0; t < ns0; ++t)
            if (flags[t]) { q_items.push_back(t); q_nodes.push_back(jb.node(t)); }
        ext[4] += (double)q_items.size();
        for (uint32_t t = ns0; t < ns; ++t) { q_items.push_back(t); q_nodes.push_back(jb.node(t)); }
        // c. their candidates and forward lists
        const uint32_t nq = (uint32_t)q_items.size();
        qfid.resize((size_t)nq * cap); qfd.resize((size_t)nq * cap); qthr.resize(nq);
        LY_TRY(hnsw_level_forward(jb, q_nodes.data(), nq, qfid.data(), qfd.data(), qthr.data()));
        // d. the dirty lists: a changed forward list, and the members of F_old(i) xor F_new(i)
        dirty.assign(ns, 0);
        for (uint32_t x = 0; x < nq; ++x) {
            const uint32_t t = q_items[x];
            uint32_t* fo = &kp.fid[(size_t)t * cap];
            const uint32_t* fn = &qfid[(size_t)x * cap];
            if (t < ns0) {
                u.idx.push_back(t);
                u.fid.insert(u.fid.end(), fo, fo + cap);
                u.fd.insert(u.fd.end(), &kp.fd[(size_t)t * cap], &kp.fd[(size_t)t * cap] + cap);
                u.thr.push_back(kp.thr[t]);
            }
            kp.thr[t] = qthr[x];
            if (memcmp(fo, fn, (size_t)cap * 4) == 0) continue;
            dirty[t] = 1;
            for (uint32_t a = 0; a < cap && fo[a] != GRAPH_PAD; ++a)
                if (std::find(fn, fn + cap, fo[a]) == fn + cap) dirty[jb.item(fo[a])] = 1;
            for (uint32_t a = 0; a < cap && fn[a] != GRAPH_PAD; ++a)
                if (std::find(fo, fo + cap, fn[a]) == fo + cap) dirty[jb.item(fn[a])] = 1;
            memcpy(fo, fn, (size_t)cap * 4);
            memcpy(&kp.fd[(size_t)t * cap], &qfd[(size_t)x * cap], (size_t)cap * 4);
        }
        for (uint32_t t = 0; t < ns; ++t) ext[5] += dirty[t] ? 1.0 : 0.0;
        LY_TRY(hnsw_level_adjacency(jb, gph, kp.fid.data(), kp.fd.data(), dirty.data(), &reselected));
    }
    // e. install
    LY_TRY(hnsw_install(h, gph, metric, s.ef_search, true));
    undo.committed = true;
    ext[6] = (double)reselected; ext[8] = times3[0]; ext[9] = times3[1]; ext[10] = times3[2];
    return done();
}

// out12 = {rows_before, rows_after, path (0 incremental, 1 plain build, 2 nothing to do), new_items, researched, dirty_lists,
// reselected, scan_us, cand_us, select_us, reverse_us, total_us} of the last extend; zeros before the first
extern "C" int lynse_hip_flat_hnsw_extend_stats(lynse_hip_flat* h, double* out12) {
    if (!h || !out12) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    std::shared_lock<std::shared_mutex> lk(h->rw);
    for (int i = 0; i < 12; ++i) out12[i] = h->hnsw ? h->hnsw->ext[i] : 0.0;
    return LYNSE_OK;
}

// A graph as hnsw_params exports it.  Lists are brought into the stored form: GRAPH_PAD entries dropped, a neighbour named twice kept
// once (its first place) — neither changes a search: the second visit of a node is skipped at level 0 and moves nothing above.
extern "C" int lynse_hip_flat_load_hnsw(lynse_hip_flat* h, int metric, uint32_t m, uint32_t ef_search, const uint32_t* levels, uint64_t n,
                                        const uint32_t* adj0, uint64_t n_upper, const uint32_t* upper_node, const uint32_t* upper_level,
                                        const uint32_t* upper_adj, uint32_t entry) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    LY_TRY(hnsw_check_metric(metric));
    LY_TRY(hnsw_check_params(m, 1, ef_search));
    std::unique_lock<std::shared_mutex> lk;
    LY_TRY(graph_lock(h, lk));
    LY_TRY(use_device(h));
    LY_TRY(graph_check_handle(h));
    if (n == 0) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "need at least one vector");
    if (n >= 0xffffffffull) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "an HNSW index holds fewer than 2^32 - 1 rows");
    if (n > h->n) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "the HNSW index covers more rows than the handle holds");
    if (!levels || !adj0 || (n_upper && (!upper_node || !upper_level || !upper_adj))) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    if ((size_t)h->dim * 4 + 512 > PoolRerank::LDS_MAX) return set_error(LYNSE_ERR_UNSUPPORTED, "HNSW: the vector does not fit in LDS");
    uint64_t nu = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if (levels[i] > HNSW_LEVEL_MAX) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "HNSW: a level beyond 52");
        nu += levels[i];
    }
    if (nu != n_upper) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "HNSW: the upper lists do not match the levels");
    HnswGraph gph;
    gph.shape(m, levels, n);
    for (uint64_t u = 0; u < n_upper; ++u)
        if (upper_node[u] != gph.upper_node[u] || upper_level[u] != gph.upper_level[u])
            return set_error(LYNSE_ERR_INVALID_ARGUMENT, "HNSW: the upper lists are not in ascending (node, level) order of the levels");
    if (entry >= n || levels[entry] != gph.top_level) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "HNSW: the entry point is not a row of the top level");
    gph.entry = entry;
    auto take = [&](const uint32_t* src, uint32_t cap, uint32_t level, uint32_t* dst) -> int {
        return graph_take_list(src, cap, n, "HNSW: a neighbour beyond the rows of the graph", dst, [&](uint32_t v) {
            return levels[v] < level ? set_error(LYNSE_ERR_INVALID_ARGUMENT, "HNSW: a neighbour below the level of its list") : LYNSE_OK;
        });
    };
    for (uint64_t i = 0; i < n; ++i) LY_TRY(take(adj0 + i * 2 * m, 2 * m, 0, gph.list((uint32_t)i, 0)));
    for (uint64_t u = 0; u < n_upper; ++u) LY_TRY(take(upper_adj + u * m, m, upper_level[u], &gph.upper_adj[u * m]));
    return hnsw_install(h, gph, metric, ef_search, false);
}

// info = {metric, m, ef_search, entry, top_level, n_upper}, all 0 (and n_hnsw 0) without an index
extern "C" int lynse_hip_flat_hnsw_params(lynse_hip_flat* h, uint32_t* info, uint64_t* n_hnsw, uint32_t* levels, uint32_t* adj0,
                                          uint32_t* upper_node, uint32_t* upper_level, uint32_t* upper_adj) {
    if (!h || !info || !n_hnsw) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    std::shared_lock<std::shared_mutex> lk(h->rw);
    if (!h->hnsw || !h->hnsw->built()) {
        for (int i = 0; i < 6; ++i) info[i] = 0;
        *n_hnsw = 0;
        return LYNSE_OK;
    }
    const HnswState& s = *h->hnsw;
    const size_t nu = s.upper_node.size();
    info[0] = (uint32_t)s.metric; info[1] = s.m; info[2] = s.ef_search; info[3] = s.entry; info[4] = s.top_level; info[5] = (uint32_t)nu;
    *n_hnsw = s.n;
    LY_TRY(use_device(h));
    if (levels) memcpy(levels, s.levels.data(), s.levels.size() * 4);
    if (upper_node && nu) memcpy(upper_node, s.upper_node.data(), nu * 4);
    if (upper_level && nu) memcpy(upper_level, s.upper_level.data(), nu * 4);
    if (adj0) LY_HIP(hipMemcpy(adj0, s.d_adj0, (size_t)s.n * 2 * s.m * 4, hipMemcpyDeviceToHost));
    if (upper_adj && nu) LY_HIP(hipMemcpy(upper_adj, s.d_upper_adj, nu * s.m * 4, hipMemcpyDeviceToHost));
    return LYNSE_OK;
}

extern "C" int lynse_hip_flat_drop_hnsw(lynse_hip_flat* h) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    LY_WRITER(h, lk);
    LY_TRY(use_device(h));
    if (h->hnsw) h->hnsw->free_index();
    return LYNSE_OK;
}

// out6 = {candidate lists, selection, reverse edges} of the last build (microseconds of host time around synchronised stages), then
// with profiling on: searches timed, their kernel microseconds (HIP events) and the distances they scored
extern "C" int lynse_hip_flat_hnsw_stage_times(lynse_hip_flat* h, double* out6, int reset) {
    if (!h || !out6) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    LY_WRITER(h, lk);
    if (!h->hnsw) { for (int i = 0; i < 6; ++i) out6[i] = 0.0; return LYNSE_OK; }
    HnswState& s = *h->hnsw;
    out6[0] = s.cand_us; out6[1] = s.select_us; out6[2] = s.reverse_us; out6[3] = s.search.searches; out6[4] = s.search.search_us; out6[5] = s.search.scored;
    if (reset) s.search.searches = s.search.search_us = s.search.scored = 0.0;
    return LYNSE_OK;
}

// rule 5; graph_search (graph_host.inc) runs the queries in chunks
extern "C" int lynse_hip_flat_search_hnsw_f32(lynse_hip_flat* h, const float* queries, uint64_t nq, uint32_t k, int metric, uint32_t ef_query,
                                              uint64_t* out_rows, float* out_dists, uint32_t* out_counts) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    LY_TRY(hnsw_check_metric(metric));
    if (nq == 0) return LYNSE_OK;
    if (!queries || !out_counts || (k && (!out_rows || !out_dists))) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    std::unique_lock<std::shared_mutex> lk;
    LY_TRY(graph_lock(h, lk));
    LY_TRY(use_device(h));
    LY_TRY(graph_check_handle(h));
    if (!h->hnsw || !h->hnsw->built()) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "no HNSW index on this handle: build or load one first");
    HnswState& s = *h->hnsw;
    if (metric != s.metric) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "the HNSW index was built for another metric");
    if (ef_query > HNSW_EF_MAX) return set_error(LYNSE_ERR_UNSUPPORTED, "HNSW: ef must be between 1 and 4096");
    if (k == 0) { memset(out_counts, 0, nq * 4); return LYNSE_OK; }
    // ef = max(ef, k); beyond the rows of the graph R never fills, so min(ef, n) answers the same
    const uint32_t ef = (uint32_t)std::min<uint64_t>(std::max<uint32_t>(ef_query ? ef_query : s.ef_search, k), s.n);
    const size_t lds = GraphSearchLds::bytes(ef, hnsw_c_cap(ef), h->dim);
    if (lds > PoolRerank::LDS_MAX) return set_error(LYNSE_ERR_UNSUPPORTED, "HNSW: the beam (24 bytes per ef, ef >= k) and the query do not fit in LDS");
    return graph_search(h, s.search, s.n, lds, "HNSW: the candidate set outgrew its 2 ef slots", queries, nq, k, out_rows, out_dists, out_counts,
                        [&](const GraphSearchChunk& c) {
        HnswSearchArgs a{};
        a.V = h->rows; a.ld = h->ld; a.D = h->dim; a.metric = metric; a.Q = c.Q; a.k = k; a.ef = ef; a.m = s.m;
        a.entry = s.entry; a.top_level = s.top_level; a.adj0 = s.d_adj0; a.upper_off = s.d_upper_off; a.upper_adj = s.d_upper_adj;
        a.vis = c.vis; a.vis_words = c.vis_words; a.out_rows = c.out_rows; a.out_dists = c.out_dists; a.out_counts = c.out_counts;
        a.out_scored = c.out_scored; a.status = c.status;
        return launch_lds<k_hnsw_search>(dim3(c.nqc), dim3(64), c.lds, c.st, a);
    });
}
