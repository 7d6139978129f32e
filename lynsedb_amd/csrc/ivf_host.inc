// ivf_host.inc — IVF-Flat entry points.  Included at the end of lynse_hip.hip.
//
// Replaces IVFIndex (src/index/ivf.rs:19-35, build :132-179, search :181-348) and IvfFlatMmap
// (src/storage/ivf_flat_mmap.rs:22-39, build :56-159, search :225-304).  HBM layout = the
// IvfFlatMmap one: rows physically reordered into contiguous per-partition slabs
// (ivf_flat_mmap.rs:115-130) + partition offsets + original row ids; centroids in a small matrix.
// Search: k_ivf_route ranks centroids (exact, reference order) -> the host groups the (query, list)
// probes by list -> k_scan_h16 in work-list mode scans each probed slab ONCE per query group
// (a slab shared by several queries of the batch is not re-read per query) in three position
// windows with the same threshold / select / exact-rescore machinery as FLAT -> k_final maps slab
// positions to original rows and orders by (distance, original row).

struct IvfScratch {
    uint64_t* d_route_rows = nullptr; float* d_route_d = nullptr; uint32_t* d_route_c = nullptr; size_t route_cap = 0;   // centroid ranking
    uint32_t* d_probes = nullptr; size_t probes_cap = 0;
    uint32_t* d_pair_q = nullptr; size_t pairs_cap = 0;
    GatherPair* d_pairs = nullptr; size_t gpairs_cap = 0;
    IvfTile* d_tiles = nullptr; size_t tiles_cap = 0;
    IvfGroup* d_groups = nullptr; size_t groups_cap = 0;   // device-side grouping (k_ivf_group)
    uint32_t* d_tbase = nullptr; size_t tbase_cap = 0;      // first tile of every (window, group)
    uint32_t* d_prank = nullptr; size_t prank_cap = 0;      // rank of every pair inside its list
    uint32_t* d_ghdr = nullptr;                             // its header: groups, tiles per window, host-path flag, pairs
    uint32_t* h_ghdr = nullptr;                             // pinned mirror
    _Float16* d_gimg = nullptr; size_t gimg_cap = 0;  // halves
    void release() {
        for (void* p : {(void*)d_route_rows, (void*)d_route_d, (void*)d_route_c, (void*)d_probes, (void*)d_pair_q, (void*)d_pairs, (void*)d_tiles, (void*)d_groups,
                        (void*)d_tbase, (void*)d_prank, (void*)d_ghdr, (void*)d_gimg})
            if (p) (void)hipFree(p);
        if (h_ghdr) (void)hipHostFree(h_ghdr);
        *this = IvfScratch();
    }
};

struct lynse_hip_ivf {
    lynse_hip_flat* store = nullptr;  // slab-ordered rows
    uint32_t dim = 0, nlist = 0;
    int metric = M_IP;
    int search_metric = -1;           // the metric of the call in flight (lynse_hip_ivf_search_metric_f32; set and reset under the store lock)
    int ivfflat_routing = 0;          // IvfFlatMmap semantics: IP 16-dim shortlist heuristic, nprobe clamp
    int no_fallback = 0;              // row shard of a larger index: an empty local part of the probed lists is not 'no candidates'
    std::vector<uint64_t> offsets;    // nlist + 1 (slab positions)
    std::vector<uint32_t> orig;       // slab position -> original row
    std::vector<uint32_t> assignments;
    std::vector<float> centroids;     // nlist x dim
    uint32_t* d_orig = nullptr;
    uint64_t* d_offsets = nullptr;    // nlist + 1 (the fused few-query search walks the probed lists on the device)
    uint64_t max_list_len = 0;
    std::vector<uint64_t> worst_rows;  // worst_rows[p] = rows of the p LARGEST lists: what nprobe = p can touch at most
    float* d_centroids = nullptr;
    uint32_t ldc = 0;
    std::vector<uint32_t> rdims;
    uint32_t* d_rdims = nullptr;
    uint64_t row_stride = 1, row_offset = 0;
    // IVF-*-BINARY (ivf.rs:77-127): rows are BinaryQuantizer codes ({0,1} floats + packed u64 words), routing is L2 on
    // the codes, the list scan is packed popcount
    bool binary = false;
    int already_binary = 0;
    std::vector<float> bq_thr;        // dim per-dimension thresholds (0.5 everywhere for {0,1} corpora)
    float* d_bq_thr = nullptr;
    // IVF-{IP,L2,COS}-SQ8 (ivf.rs:132-337 with QuantizerType::Scalar): `store` holds the DECODED rows (the pool stage is the
    // ordinary IVF scan over them), d_raw the original f32 rows in ORIGINAL row order for the exact rerank
    bool sq8 = false;
    std::vector<float> sq_min, sq_scale;  // fitted ScalarQuantizer: min_val, scale = range / 255
    float* d_sq = nullptr;            // [min | scale] on the device (2 x dim)
    float* d_raw = nullptr;           // n x dim original rows
    struct Sq8Scratch {               // per-search buffers of the SQ8 path (grown on demand; searches hold the guard)
        float* d_q = nullptr; size_t q_cap = 0;
        float* d_pdist = nullptr; size_t pdist_cap = 0;
        PoolRerank rr;                // the pool's rows and counts, the rerank's buffers and timing events
    } sq;
    // profiling (lynse_hip_ivf_sq8_stage_times): searches timed, and the pool stage / the rerank in microseconds (HIP events on the
    // search stream; the host selection of a pool beyond the LDS counts to the rerank)
    uint64_t sq_searches = 0;
    double sq_pool_us = 0.0, sq_rerank_us = 0.0;
    // SPANN-{IP,L2,COS}[-SQ8] (spann_host.inc): a row sits in up to replicas + 1 lists, so the slab store holds POSTINGS (store->n of
    // them, `orig` repeats rows) and n_rows rows; `assignments` is empty (no single list per row)
    bool spann = false;
    uint32_t replicas = 0;
    uint64_t n_rows = 0;
    struct SpannScratch {             // per-search buffers of the SPANN path (grown on demand; searches hold the guard)
        float* d_q = nullptr; size_t q_cap = 0;
        uint64_t* d_rows = nullptr; size_t rows_cap = 0;   // the k' keys of the list scan ...
        float* d_dists = nullptr; size_t dists_cap = 0;
        uint32_t* d_cnt = nullptr; size_t cnt_cap = 0;
        uint64_t* d_orow = nullptr; size_t orow_cap = 0;   // ... and the distinct rows (plain modes)
        float* d_odist = nullptr; size_t odist_cap = 0;
        uint32_t* d_ocnt = nullptr; size_t ocnt_cap = 0;
        uint32_t* d_qmap = nullptr; size_t qmap_cap = 0;   // the queries of a fallback rerun
        void release() {
            for (void* p : {(void*)d_q, (void*)d_rows, (void*)d_dists, (void*)d_cnt, (void*)d_orow, (void*)d_odist, (void*)d_ocnt, (void*)d_qmap})
                if (p) (void)hipFree(p);
            *this = SpannScratch();
        }
    } sp;
    lynse_hip_flat* cstore = nullptr; // the centroid matrix as a FLAT shard: exact routing = its top-nprobe search
    uint32_t* d_smask = nullptr;      // subset filter by slab position
    uint64_t smask_words = 0;
    // per-search device scratch (grown on demand), ONE SET PER SEARCH CONTEXT of the slab store: the blocking searches run on context 0
    // under the store's exclusive lock, searches in flight (lynse_hip_ivf_search_submit_f32_device) on the contexts 1.. they lease
    IvfScratch scr[lynse_hip_flat::MAX_CTX];
    int inflight = 0;                 // tickets outstanding (counted under `guard`): insert / delete are refused meanwhile
    uint64_t tk_async = 0, tk_sync = 0, tk_redo = 0;   // tickets enqueued without a host synchronisation / answered inside submit / re-answered inside wait
    // Index-level guard: insert / delete replace the slab store (and with it the store's own reader / writer lock), so every entry
    // point that touches the store takes this mutex first; it survives the replacement (ivf_reassemble hands it back).
    std::shared_ptr<std::mutex> guard = std::make_shared<std::mutex>();
};

// The guard FIELD is written by ivf_reassemble (std::swap of the whole index, then the guard swapped back): a reader copying the
// shared_ptr at that moment would race on the pointer itself (and could lock the wrong mutex).  Every copy and both swaps go through
// this process-wide mutex (held for a few instructions; ThreadSanitizer run: tests/test_tsan_host.py).
static std::mutex g_ivf_guard_mu;
static std::shared_ptr<std::mutex> ivf_guard_of(const lynse_hip_ivf* h) {
    std::lock_guard<std::mutex> lk(g_ivf_guard_mu);
    return h->guard;
}
#define IVF_GUARD(h) const std::shared_ptr<std::mutex> guard_ = ivf_guard_of(h); std::lock_guard<std::mutex> glk_(*guard_)

static std::vector<uint32_t> ivf_routing_dims(const std::vector<float>& cen, uint32_t dim, uint32_t k);
static inline IvfScratch& iscr(lynse_hip_ivf* h) { return h->scr[tl_ctx_slot]; }   // the scratch of the calling thread's search context

static void ivf_free(lynse_hip_ivf* h) {
    if (!h) return;
    if (h->store) {
        (void)hipSetDevice(h->store->device);
        for (void* p : {(void*)h->d_orig, (void*)h->d_offsets, (void*)h->d_centroids, (void*)h->d_rdims, (void*)h->d_bq_thr, (void*)h->d_smask,
                        (void*)h->d_sq, (void*)h->d_raw, (void*)h->sq.d_q, (void*)h->sq.d_pdist})
            if (p) (void)hipFree(p);
        h->sq.rr.release();
        h->sp.release();
        for (auto& x : h->scr) x.release();
        if (h->cstore) lynse_hip_flat_destroy(h->cstore);
        lynse_hip_flat_destroy(h->store);
    }
    delete h;
}

extern "C" int lynse_hip_ivf_destroy(lynse_hip_ivf* h) {
    ivf_free(h);
    return LYNSE_OK;
}
extern "C" uint64_t lynse_hip_ivf_len(const lynse_hip_ivf* h) {
    if (!h) return 0;
    IVF_GUARD(h);   // (insert / delete replace h->store)
    if (h->spann) return h->n_rows;   // (the store holds postings)
    return h->store ? h->store->n : 0;
}
extern "C" uint32_t lynse_hip_ivf_nlist(const lynse_hip_ivf* h) { return h ? h->nlist : 0; }

extern "C" int lynse_hip_ivf_set_row_map(lynse_hip_ivf* h, uint64_t stride, uint64_t offset) {
    if (!h || stride == 0) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "bad row map");
    IVF_GUARD(h);   // (searches read the row map under the guard)
    if (h->sq8 && (stride != 1 || offset != 0)) return set_error(LYNSE_ERR_UNSUPPORTED, "an IVF-*-SQ8 index is not row-sharded");
    if (h->spann) return set_error(LYNSE_ERR_UNSUPPORTED, "a SPANN index is not row-sharded");
    h->row_stride = stride;
    h->row_offset = offset;
    return LYNSE_OK;
}

extern "C" int lynse_hip_ivf_set_fused_search(lynse_hip_ivf* h, int on) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    IVF_GUARD(h);
    if (!h->store) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    if (h->spann && on) return set_error(LYNSE_ERR_UNSUPPORTED, "a SPANN index searches with the staged pipeline (replicated rows)");
    return lynse_hip_flat_set_fused_search(h->store, on);
}

extern "C" int lynse_hip_ivf_set_routing(lynse_hip_ivf* h, int ivfflat_routing) {
    // 1 = IvfFlatMmap semantics (IP 16-dim shortlist heuristic, no empty-probe fallback); 0 = IVFIndex
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    IVF_GUARD(h);
    if (!h->store) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    (void)hipSetDevice(h->store->device);
    if (h->spann) return set_error(LYNSE_ERR_UNSUPPORTED, "a SPANN index ranks every centroid exactly (IVFIndex routing)");
    h->no_fallback = ivfflat_routing == 2 ? 1 : 0;
    if (ivfflat_routing == 2) return LYNSE_OK;  // routing semantics unchanged, only the fallback is switched off
    h->ivfflat_routing = ivfflat_routing ? 1 : 0;
    h->rdims = ivfflat_routing ? ivf_routing_dims(h->centroids, h->dim, h->nlist) : std::vector<uint32_t>();
    if (!h->rdims.empty()) LY_TRY(h2d_done(h->d_rdims, h->rdims.data(), h->rdims.size() * 4));
    return LYNSE_OK;
}

extern "C" int lynse_hip_ivf_export(const lynse_hip_ivf* h, float* centroids, uint32_t* assignments, uint64_t* offsets,
                                    uint32_t* original_ids) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    IVF_GUARD(h);   // (insert / delete rewrite assignments / offsets / original ids)
    if (h->spann) return set_error(LYNSE_ERR_UNSUPPORTED, "export assumes one list per row: lynse_hip_spann_postings gives a SPANN index's lists");
    if (centroids) memcpy(centroids, h->centroids.data(), h->centroids.size() * 4);
    if (assignments) memcpy(assignments, h->assignments.data(), h->assignments.size() * 4);
    if (offsets) memcpy(offsets, h->offsets.data(), h->offsets.size() * 8);
    if (original_ids) memcpy(original_ids, h->orig.data(), h->orig.size() * 4);
    return LYNSE_OK;
}

// select_routing_dims (ivf_flat_mmap.rs:316-348): the 16 highest-variance centroid dims, ascending.
static std::vector<uint32_t> ivf_routing_dims(const std::vector<float>& cen, uint32_t dim, uint32_t k) {
    std::vector<uint32_t> out;
    if (k == 0 || dim == 0 || !(dim >= 64 && k >= 64)) return out;
    std::vector<float> sums(dim, 0.f), sq(dim, 0.f);
    for (uint32_t c = 0; c < k; ++c)
        for (uint32_t d = 0; d < dim; ++d) {
            const float v = cen[(size_t)c * dim + d];
            sums[d] = sums[d] + v;
            const float p = v * v;
            sq[d] = sq[d] + p;
        }
    const float inv_k = 1.0f / (float)k;
    std::vector<std::pair<float, uint32_t>> dv(dim);
    for (uint32_t d = 0; d < dim; ++d) {
        const float mean = sums[d] * inv_k;
        const float a = sq[d] * inv_k, b = mean * mean;
        dv[d] = {a - b, d};
    }
    std::stable_sort(dv.begin(), dv.end(), [](const auto& x, const auto& y) { return x.first > y.first; });
    const uint32_t keep = std::min<uint32_t>(16, dim);
    for (uint32_t i = 0; i < keep; ++i) out.push_back(dv[i].second);
    std::sort(out.begin(), out.end());
    return out;
}

// Assemble the device structures from (rows, centroids, assignments): slab layout of
// IvfFlatMmap::build steps 3-4 (ivf_flat_mmap.rs:105-130) == kmeans::inverted_lists_from_assignments
// order (ascending rows inside a list, kmeans.rs:317-345).
// Appends the rows src[ids[i]] (src in HBM, `dim` floats per row, contiguous) to a store: the slab reordering of a
// device-resident build happens inside HBM.
// (src_ld: row stride of the source in floats, 0 = dim.  scatter_*: rows that do NOT come from d_src — the new rows of an insert,
// n_scatter rows of `dim` floats in HBM — are written to their positions scatter_pos[i] of the appended block afterwards; their
// d_ids entries may point anywhere valid.)
static int flat_append_gathered_device(lynse_hip_flat* h, const float* d_src, const uint32_t* d_ids, uint64_t n, uint32_t src_ld = 0,
                                       const float* d_scatter = nullptr, const uint32_t* d_scatter_pos = nullptr, uint64_t n_scatter = 0) {
    if (n == 0) return LYNSE_OK;
    std::unique_lock<std::shared_mutex> lk(h->rw);
    LY_TRY(use_device(h));
    LY_TRY(grow_rows(h, h->n + n));
    const uint64_t pieces = n * ((h->ld + 3) / 4);
    hipLaunchKernelGGL(k_gather_rows_f32, dim3((uint32_t)std::min<uint64_t>((pieces + 255) / 256, (uint64_t)h->num_cu * 32)), dim3(256), 0,
                       cur(h).stream, d_src, src_ld ? src_ld : h->dim, d_ids, n, h->rows + (size_t)h->n * h->ld, h->ld, h->dim);
    LY_HIP(hipGetLastError());
    if (n_scatter) {
        const uint64_t sp = n_scatter * ((h->ld + 3) / 4);
        hipLaunchKernelGGL(k_scatter_rows_f32, dim3((uint32_t)std::min<uint64_t>((sp + 255) / 256, (uint64_t)h->num_cu * 32)), dim3(256), 0,
                           cur(h).stream, d_scatter, h->dim, d_scatter_pos, n_scatter, h->rows + (size_t)h->n * h->ld, h->ld, h->dim);
        LY_HIP(hipGetLastError());
    }
    LY_HIP(hipStreamSynchronize(cur(h).stream));
    h->n += n;
    return LYNSE_OK;
}

// Where the rows of a RE-assembly come from (IVFIndex::insert without a host round trip of the indexed rows): new original row r is
// the row at slab position old_pos[r] of the OLD store (d_old_rows, stride old_ld floats), or — old_pos[r] == 0xffffffff — the new row
// r - first_new of new_rows (host, dim floats each).
struct IvfRowSource {
    const float* d_old_rows;
    uint32_t old_ld;
    const uint32_t* old_pos;      // host, one entry per row of the new index
    const float* new_rows;        // host
    uint64_t first_new, n_new;
};

// row_off (SPANN, rows on the device only): row i sits in the lists assignments[row_off[i] .. row_off[i + 1]) — the store holds
// row_off[n] postings, `orig` repeats rows, `assignments` stays empty.
static int ivf_assemble(const float* rows, uint64_t n, uint32_t dim, const float* centroids, uint32_t nlist,
                        const uint32_t* assignments, int metric, int ivfflat_routing, int device, lynse_hip_ivf** out,
                        bool rows_on_device = false, const IvfRowSource* rs = nullptr, const uint64_t* row_off = nullptr) {
    auto* h = new lynse_hip_ivf();
    h->dim = dim; h->nlist = nlist; h->metric = metric; h->ivfflat_routing = ivfflat_routing;
    int rc = lynse_hip_flat_create(dim, device, &h->store);
    if (rc != LYNSE_OK) { delete h; return rc; }
    const uint64_t n_rows = n;
    if (row_off) n = row_off[n_rows];   // (from here on: slab positions)
    h->offsets.assign(nlist + 1, 0);
    for (uint64_t i = 0; i < n; ++i) {
        if (assignments[i] >= nlist) { ivf_free(h); return set_error(LYNSE_ERR_INVALID_ARGUMENT, "assignment out of range"); }
        h->offsets[assignments[i] + 1] += 1;
    }
    for (uint32_t p = 0; p < nlist; ++p) h->offsets[p + 1] += h->offsets[p];
    h->orig.resize(n);
    if (!row_off) h->assignments.assign(assignments, assignments + n);
    {
        std::vector<uint64_t> wp(h->offsets.begin(), h->offsets.end() - 1);
        if (row_off) {
            for (uint64_t r = 0; r < n_rows; ++r)
                for (uint64_t j = row_off[r]; j < row_off[r + 1]; ++j) h->orig[wp[assignments[j]]++] = (uint32_t)r;
        } else {
            for (uint64_t i = 0; i < n; ++i) h->orig[wp[assignments[i]]++] = (uint32_t)i;
        }
    }
    auto fail = [&](const char* what) { ivf_free(h); return set_error(LYNSE_ERR_OUT_OF_MEMORY, what); };
    if (hipMalloc(&h->d_orig, std::max<size_t>((size_t)n * 4, 4)) != hipSuccess) return fail("hipMalloc(orig)");
    if (n) (void)h2d_done(h->d_orig, h->orig.data(), (size_t)n * 4);
    if (hipMalloc(&h->d_offsets, ((size_t)nlist + 1) * 8) != hipSuccess) return fail("hipMalloc(offsets)");
    (void)h2d_done(h->d_offsets, h->offsets.data(), ((size_t)nlist + 1) * 8);
    for (uint32_t p = 0; p < nlist; ++p) h->max_list_len = std::max(h->max_list_len, h->offsets[p + 1] - h->offsets[p]);
    {
        std::vector<uint64_t> lens(nlist);
        for (uint32_t p = 0; p < nlist; ++p) lens[p] = h->offsets[p + 1] - h->offsets[p];
        std::sort(lens.begin(), lens.end(), std::greater<uint64_t>());
        h->worst_rows.assign(nlist + 1, 0);
        for (uint32_t p = 0; p < nlist; ++p) h->worst_rows[p + 1] = h->worst_rows[p] + lens[p];
    }
    rc = lynse_hip_flat_reserve(h->store, std::max<uint64_t>(n, 1));
    if (rs) {
        // re-assembly: the indexed rows are gathered from the OLD slab store inside HBM, only the new rows are uploaded
        uint32_t *d_gid = nullptr, *d_spos = nullptr;
        float* d_new = nullptr;
        struct Free { uint32_t*& a; uint32_t*& b; float*& c; ~Free() { if (a) (void)hipFree(a); if (b) (void)hipFree(b); if (c) (void)hipFree(c); } } fr{d_gid, d_spos, d_new};
        std::vector<uint32_t> gid(n), spos(rs->n_new);
        for (uint64_t p = 0; p < n; ++p) {
            const uint32_t r = h->orig[p], op = rs->old_pos[r];
            gid[p] = op == 0xffffffffu ? 0u : op;
            if (op == 0xffffffffu) spos[r - rs->first_new] = (uint32_t)p;
        }
        if (rc == LYNSE_OK && hipMalloc(&d_gid, std::max<size_t>((size_t)n * 4, 4)) != hipSuccess) rc = set_error(LYNSE_ERR_OUT_OF_MEMORY, "hipMalloc(gather ids)");
        if (rc == LYNSE_OK && n) rc = h2d_done(d_gid, gid.data(), (size_t)n * 4);
        if (rc == LYNSE_OK && rs->n_new) {
            if (hipMalloc(&d_spos, (size_t)rs->n_new * 4) != hipSuccess || hipMalloc(&d_new, (size_t)rs->n_new * dim * 4) != hipSuccess)
                rc = set_error(LYNSE_ERR_OUT_OF_MEMORY, "hipMalloc(new rows)");
            if (rc == LYNSE_OK) rc = h2d_done(d_spos, spos.data(), (size_t)rs->n_new * 4);
            if (rc == LYNSE_OK) rc = h2d_done(d_new, rs->new_rows, (size_t)rs->n_new * dim * 4);
        }
        if (rc == LYNSE_OK) rc = flat_append_gathered_device(h->store, rs->d_old_rows, d_gid, n, rs->old_ld, d_new, d_spos, rs->n_new);
    } else if (rows_on_device) {
        // rows already in HBM: the slab order is a gather by original row id inside HBM
        if (rc == LYNSE_OK) rc = flat_append_gathered_device(h->store, rows, h->d_orig, n);
    } else {
        // upload rows in slab order, chunked through a host staging buffer
        const uint64_t chunk = std::max<uint64_t>(1, (64ull << 20) / ((uint64_t)dim * 4));
        std::vector<float> stage((size_t)std::min<uint64_t>(chunk, std::max<uint64_t>(n, 1)) * dim);
        for (uint64_t r = 0; r < n && rc == LYNSE_OK; r += chunk) {
            const uint64_t nr = std::min<uint64_t>(chunk, n - r);
            for (uint64_t i = 0; i < nr; ++i) memcpy(&stage[(size_t)i * dim], rows + (size_t)h->orig[r + i] * dim, (size_t)dim * 4);
            rc = lynse_hip_flat_append_f32(h->store, stage.data(), nr);
        }
    }
    if (rc == LYNSE_OK) rc = lynse_hip_flat_finalize(h->store);
    if (rc != LYNSE_OK) { ivf_free(h); return rc; }
    h->centroids.assign(centroids, centroids + (size_t)nlist * dim);
    h->ldc = dim;
    if (hipMalloc(&h->d_centroids, std::max<size_t>((size_t)nlist * dim * 4, 4)) != hipSuccess) return fail("hipMalloc(centroids)");
    (void)h2d_done(h->d_centroids, centroids, (size_t)nlist * dim * 4);
    // exact routing (mode 0) is a FLAT top-nprobe search over the centroids with the single-row kernels
    rc = lynse_hip_flat_create(dim, device, &h->cstore);
    if (rc == LYNSE_OK) rc = lynse_hip_flat_append_f32(h->cstore, centroids, nlist);
    if (rc == LYNSE_OK) rc = lynse_hip_flat_set_ip_form(h->cstore, LYNSE_IPFORM_SINGLE);
    if (rc == LYNSE_OK) rc = lynse_hip_flat_finalize(h->cstore);
    if (rc != LYNSE_OK) { ivf_free(h); return rc; }
    if (ivfflat_routing) h->rdims = ivf_routing_dims(h->centroids, dim, nlist);
    if (metric >= M_HAMMING) {  // rebuild_packed_codes (ivf.rs:89-108): pack the {0,1} codes with the 0.5 cut
        h->binary = true;
        { const int prc = ensure_packed_locked(h->store); if (prc != LYNSE_OK) { ivf_free(h); return prc; } }
    }
    if (hipMalloc(&h->d_rdims, 16 * 4) != hipSuccess) return fail("hipMalloc(rdims)");
    if (!h->rdims.empty()) (void)h2d_done(h->d_rdims, h->rdims.data(), h->rdims.size() * 4);
    *out = h;
    return LYNSE_OK;
}

static int ivf_check_args(const float* rows, uint64_t n, uint32_t dim, uint32_t nlist, int metric, lynse_hip_ivf** out) {
    if (!out) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    if (dim == 0) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "IVF dimension must be greater than zero");   // ivf_flat_mmap.rs:64-69
    if (nlist == 0) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "IVF partition count must be greater than zero");  // :76-81
    if (!rows && n) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "rows is NULL");
    if (n > 0xfffffff0ull) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "IVF vector count exceeds the u32 ID capacity");  // :89-94
    if (metric_additive(metric)) return metric_check(metric);
    if (!metric_valid(metric)) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "unknown metric");
    if (nlist > 16384) return set_error(LYNSE_ERR_UNSUPPORTED, "nlist > 16384 is not supported yet");
    return LYNSE_OK;
}

// BinaryQuantizer::fit + encode/decode (quantizer/mod.rs:321-393) on the device: thresholds, and the {0,1} codes of `rows`
// (host copy in *enc when enc != NULL).  `thr_in` != NULL skips the fit (load path).
static int bq_fit_encode(const float* rows, uint64_t n, uint32_t dim, int device, const float* thr_in, std::vector<float>* thr,
                         int* already_binary, std::vector<float>* enc) {
    LY_HIP(hipSetDevice(device));
    thr->assign(dim, 0.5f);
    *already_binary = 0;
    if (n == 0) return LYNSE_OK;
    float *d_v = nullptr, *d_t = nullptr;
    uint32_t* d_nb = nullptr;
    struct G { std::vector<void*> b; ~G() { for (void* p : b) if (p) (void)hipFree(p); } } g;
    LY_HIP(hipMalloc(&d_v, (size_t)n * dim * 4)); g.b.push_back(d_v);
    LY_HIP(hipMalloc(&d_t, (size_t)dim * 4 * 3)); g.b.push_back(d_t);
    LY_HIP(hipMalloc(&d_nb, 4)); g.b.push_back(d_nb);
    LY_TRY(h2d_done(d_v, rows, (size_t)n * dim * 4));
    if (thr_in) {
        thr->assign(thr_in, thr_in + dim);
    } else {
        LY_TRY(memset_done(d_nb, 0, 4));
        hipLaunchKernelGGL(k_bq_colstats, dim3(dim), dim3(256), 0, 0, d_v, dim, dim, n, d_t, d_t + dim, d_nb);
        LY_HIP(hipGetLastError());
        uint32_t nb = 0;
        LY_HIP(hipMemcpy(&nb, d_nb, 4, hipMemcpyDeviceToHost));
        *already_binary = nb ? 0 : 1;
        if (nb) {
            hipLaunchKernelGGL(k_bq_median, dim3(dim), dim3(256), 0, 0, d_v, dim, dim, n, d_t + 2 * (size_t)dim);
            LY_HIP(hipGetLastError());
            std::vector<float> st((size_t)dim * 3);
            LY_HIP(hipMemcpy(st.data(), d_t, (size_t)dim * 12, hipMemcpyDeviceToHost));
            for (uint32_t d = 0; d < dim; ++d) {
                const float mn = st[d], mx = st[dim + d], med = st[2 * (size_t)dim + d];
                const float mid = mn + mx;
                (*thr)[d] = (med <= mn || med >= mx) ? 0.5f * mid : med;
            }
        }
    }
    if (enc) {
        LY_TRY(h2d_done(d_t, thr->data(), (size_t)dim * 4));
        hipLaunchKernelGGL(k_bq_binarize, dim3(1024), dim3(256), 0, 0, d_v, dim, dim, n, d_t, d_v, dim);
        LY_HIP(hipGetLastError());
        enc->resize((size_t)n * dim);
        LY_HIP(hipMemcpy(enc->data(), d_v, (size_t)n * dim * 4, hipMemcpyDeviceToHost));
    }
    return LYNSE_OK;
}

static int ivf_set_thresholds(lynse_hip_ivf* h, const std::vector<float>& thr, int already_binary) {
    h->bq_thr = thr;
    h->already_binary = already_binary;
    LY_HIP(hipMalloc(&h->d_bq_thr, std::max<size_t>(thr.size() * 4, 4)));
    LY_TRY(h2d_done(h->d_bq_thr, thr.data(), thr.size() * 4));
    return LYNSE_OK;
}

extern "C" int lynse_hip_ivf_load(const float* rows, uint64_t n, uint32_t dim, const float* centroids, uint32_t nlist,
                                  const uint32_t* assignments, int metric, int device, lynse_hip_ivf** out) {
    LY_TRY(ivf_check_args(rows, n, dim, nlist, metric, out));
    if (!centroids || (!assignments && n)) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    if (metric >= M_HAMMING) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "binary metrics load through lynse_hip_ivf_load_binary");
    return ivf_assemble(rows, n, dim, centroids, nlist, assignments, metric, 0, device, out);
}

extern "C" int lynse_hip_ivf_load_binary(const float* rows, uint64_t n, uint32_t dim, const float* centroids, uint32_t nlist,
                                         const uint32_t* assignments, int metric, const float* thresholds, int device,
                                         lynse_hip_ivf** out) {
    LY_TRY(ivf_check_args(rows, n, dim, nlist, metric, out));
    if (!centroids || (!assignments && n) || !thresholds) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    if (metric < M_HAMMING) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "lynse_hip_ivf_load_binary needs a binary metric");
    std::vector<float> thr, enc;
    int ab = 0;
    LY_TRY(bq_fit_encode(rows, n, dim, device, thresholds, &thr, &ab, &enc));
    LY_TRY(ivf_assemble(enc.data(), n, dim, centroids, nlist, assignments, metric, 0, device, out));
    const int rc = ivf_set_thresholds(*out, thr, 0);
    if (rc != LYNSE_OK) { ivf_free(*out); *out = nullptr; }
    return rc;
}

extern "C" int lynse_hip_ivf_thresholds(const lynse_hip_ivf* h, float* thresholds, int* already_binary) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "not a binary IVF index");
    IVF_GUARD(h);
    if (!h->binary) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "not a binary IVF index");
    if (thresholds) memcpy(thresholds, h->bq_thr.data(), h->bq_thr.size() * 4);
    if (already_binary) *already_binary = h->already_binary;
    return LYNSE_OK;
}

// ---------------------------------------------------------------------------------- k-means ----
// kmeans::train_for_metric (kmeans.rs:74-139) on the device.
namespace {
struct FastRng {  // kmeans.rs:21-35
    uint64_t s;
    double next() {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (double)(s >> 33) / (double)(1ull << 31);
    }
};
}  // namespace

// Row-sharded training (lynse_hip_ivf_kmeans_sharded): `rows` are THIS rank's rows (global row g = local g / world on rank g % world),
// `reduce` sums a host buffer over all ranks in place (dtype 0 f32, 1 u32, 2 f32 in rank order).  The algorithm is kmeans_train on the
// union — same FastRng sample and farthest-first init (the sample rows are gathered by a sum: exactly one rank owns each), assignment
// of the local rows, GLOBAL counts / empty-cluster rule / stop test — with the centroid sums formed per rank and added IN RANK ORDER,
// ((p0 + p1) + p2) + ...: the specification at every world size (oracle: lo_kmeans_train_sharded).
struct KmShard {
    uint32_t rank = 0, world = 1;
    uint64_t n_global = 0;
    // sums a HOST buffer over the ranks in place: dtype 0 = f32 in any order (the init sample: one owner per row, zeros elsewhere),
    // 1 = u32, 2 = f32 in RANK order, ((p0 + p1) + p2) + ... (the centroid sums: defined bit for bit at every world size)
    std::function<int(void*, uint64_t, int)> reduce;
    // the communicator's form of a Lloyd iteration's reduction, on device buffers (comm_host.inc): d_sums (count floats, written on
    // `st`) all-gathered and added in rank order, the member counts (from d_off) + the rank's "changed" word all-reduced as integers;
    // the reduced sums and the k + 1 words land in h_sums / h_counts.  Unset = the host callback above.
    std::function<int(float* d_sums, uint64_t count, const uint64_t* d_off, uint32_t k, uint32_t changed, hipStream_t st, float* h_sums, uint32_t* h_counts)> reduce_iter;
};

static int ivf_kmeans(const float* rows, uint64_t n, uint32_t dim, uint32_t requested, uint32_t max_iter, int metric,
                      int device, std::vector<float>* centroids_out, std::vector<uint32_t>* assign_out, uint32_t* k_out,
                      bool rows_on_device = false, const KmShard* sh = nullptr) {
    const uint64_t n_all = sh ? sh->n_global : n;   // rows of the whole collection
    const uint32_t k = (uint32_t)std::min<uint64_t>(requested, n_all);
    *k_out = k;
    centroids_out->assign((size_t)k * dim, 0.f);
    assign_out->assign(n, 0u);
    if (n_all == 0 || k == 0) return LYNSE_OK;
    LY_HIP(hipSetDevice(device));
    // ---- the data as a FLAT store (queries for the assignment step come straight from it)
    lynse_hip_flat* data = nullptr;
    LY_TRY(lynse_hip_flat_create(dim, device, &data));
    struct Guard { lynse_hip_flat*& d; std::vector<void*> bufs; lynse_hip_flat* cen = nullptr;
                   ~Guard() { for (void* p : bufs) if (p) (void)hipFree(p); if (cen) lynse_hip_flat_destroy(cen); if (d) lynse_hip_flat_destroy(d); } } guard{data};
    LY_TRY(lynse_hip_flat_reserve(data, std::max<uint64_t>(n, 1)));
    if (n) {
        if (rows_on_device) LY_TRY(lynse_hip_flat_append_f32_device(data, rows, n));
        else LY_TRY(lynse_hip_flat_append_f32(data, rows, n));
    }
    const uint32_t ld = data->ld;
    hipStream_t st = cur(data).stream;

    // ---- init: kmeans_pp_init_metric (kmeans.rs:141-196) — over the rows of the WHOLE collection
    FastRng rng{42};
    uint64_t sample_n = std::min<uint64_t>(n_all, std::min<uint64_t>(std::max<uint64_t>((uint64_t)k * 32, 2048), 10000));
    std::vector<uint64_t> idx(n_all);
    for (uint64_t i = 0; i < n_all; ++i) idx[i] = i;
    if (sample_n < n_all) {
        for (uint64_t i = 0; i < sample_n; ++i) {
            const uint64_t span = n_all - i;
            uint64_t off = (uint64_t)(rng.next() * (double)span);
            if (off > span - 1) off = span - 1;
            std::swap(idx[i], idx[i + off]);
        }
    }
    std::vector<float> sample((size_t)sample_n * dim, 0.0f);
    // the sample rows this rank owns (all of them without sharding): position in the sample, local row
    std::vector<uint64_t> own_pos;
    std::vector<uint32_t> own_row;
    for (uint64_t s = 0; s < sample_n; ++s) {
        if (!sh) { own_pos.push_back(s); own_row.push_back((uint32_t)idx[s]); }
        else if (idx[s] % sh->world == sh->rank) { own_pos.push_back(s); own_row.push_back((uint32_t)(idx[s] / sh->world)); }
    }
    if (rows_on_device && !own_row.empty()) {  // the init sample is gathered inside HBM and read back once
        const uint64_t m = own_row.size();
        std::vector<float> tmp((size_t)m * dim);
        uint32_t* d_ids = nullptr; float* d_tmp = nullptr;
        LY_HIP(hipMalloc(&d_ids, (size_t)m * 4)); guard.bufs.push_back(d_ids);
        LY_HIP(hipMalloc(&d_tmp, (size_t)m * dim * 4)); guard.bufs.push_back(d_tmp);
        LY_HIP(hipMemcpyAsync(d_ids, own_row.data(), (size_t)m * 4, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_gather_rows_f32, dim3((uint32_t)std::min<uint64_t>((m * ((dim + 3) / 4) + 255) / 256, 4096)), dim3(256), 0, st,
                           rows, dim, d_ids, m, d_tmp, dim, dim);
        LY_HIP(hipGetLastError());
        LY_HIP(hipMemcpyAsync(tmp.data(), d_tmp, (size_t)m * dim * 4, hipMemcpyDeviceToHost, st));
        LY_HIP(hipStreamSynchronize(st));
        for (uint64_t j = 0; j < m; ++j) memcpy(&sample[(size_t)own_pos[j] * dim], &tmp[(size_t)j * dim], (size_t)dim * 4);
    } else {
        for (uint64_t j = 0; j < own_row.size(); ++j) memcpy(&sample[(size_t)own_pos[j] * dim], rows + (size_t)own_row[j] * dim, (size_t)dim * 4);
    }
    if (sh) {   // every sample row has exactly one owner; the others contribute zeros: the sum is the row, bit for bit (x + 0 = x; -0 rows become +0: they compare equal)
        if (const int rr = sh->reduce(sample.data(), (uint64_t)sample_n * dim, 0))
            return rr == 2 ? set_error(LYNSE_ERR_TIMEOUT, "the reduction of the k-means sample did not finish within the wait timeout (a rank is gone?)")
                           : set_error(LYNSE_ERR_DEVICE, "the reduction of the k-means sample failed");
    }
    std::vector<float>& cen = *centroids_out;
    const uint64_t first = (uint64_t)(rng.next() * (double)sample_n) % sample_n;
    memcpy(&cen[0], &sample[(size_t)first * dim], (size_t)dim * 4);
    float *d_sample = nullptr, *d_point = nullptr, *d_minrank = nullptr;
    LY_HIP(hipMalloc(&d_sample, (size_t)sample_n * dim * 4)); guard.bufs.push_back(d_sample);
    LY_HIP(hipMalloc(&d_point, (size_t)dim * 4)); guard.bufs.push_back(d_point);
    LY_HIP(hipMalloc(&d_minrank, (size_t)sample_n * 4)); guard.bufs.push_back(d_minrank);
    LY_HIP(hipMemcpyAsync(d_sample, sample.data(), (size_t)sample_n * dim * 4, hipMemcpyHostToDevice, st));
    std::vector<float> minrank((size_t)sample_n, 3.402823466e+38f);
    LY_HIP(hipMemcpyAsync(d_minrank, minrank.data(), (size_t)sample_n * 4, hipMemcpyHostToDevice, st));
    for (uint32_t c = 1; c < k; ++c) {
        LY_HIP(hipMemcpyAsync(d_point, &cen[(size_t)(c - 1) * dim], (size_t)dim * 4, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_kmeans_minrank, dim3((uint32_t)((sample_n * 8 + 255) / 256)), dim3(256), 0, st, d_sample, dim, dim,
                           (uint32_t)sample_n, d_point, metric, d_minrank);
        LY_HIP(hipGetLastError());
        LY_HIP(hipMemcpyAsync(minrank.data(), d_minrank, (size_t)sample_n * 4, hipMemcpyDeviceToHost, st));
        LY_HIP(hipStreamSynchronize(st));
        uint64_t best = 0;  // Iterator::max_by keeps the LAST maximal element (kmeans.rs:185-190)
        for (uint64_t i = 1; i < sample_n; ++i)
            if (!(minrank[i] < minrank[best])) best = i;
        memcpy(&cen[(size_t)c * dim], &sample[(size_t)best * dim], (size_t)dim * 4);
    }

    // ---- Lloyd (kmeans.rs:96-130)
    std::vector<uint32_t> cur(n, 0xffffffffu), nxt(n);
    std::vector<float> sums((size_t)k * dim);
    float* d_sums = nullptr; uint32_t* d_members = nullptr; uint64_t* d_off = nullptr;
    LY_HIP(hipMalloc(&d_sums, (size_t)k * dim * 4)); guard.bufs.push_back(d_sums);
    LY_HIP(hipMalloc(&d_members, (size_t)n * 4)); guard.bufs.push_back(d_members);
    LY_HIP(hipMalloc(&d_off, ((size_t)k + 1) * 8)); guard.bufs.push_back(d_off);
    std::vector<uint64_t> rowsbuf(256);
    std::vector<float> dbuf(256);
    std::vector<uint32_t> cbuf(256);
    float* d_q = nullptr; uint64_t* d_r = nullptr; float* d_d = nullptr; uint32_t* d_c = nullptr;
    constexpr uint64_t AQ = 32768;  // rows assigned per search call (passes of ASSIGN_QCHUNK rows inside)
    constexpr uint32_t ASSIGN_QCHUNK = 8192;
    LY_HIP(hipMalloc(&d_q, AQ * (size_t)dim * 4)); guard.bufs.push_back(d_q);
    LY_HIP(hipMalloc(&d_r, AQ * 8)); guard.bufs.push_back(d_r);
    LY_HIP(hipMalloc(&d_d, AQ * 4)); guard.bufs.push_back(d_d);
    LY_HIP(hipMalloc(&d_c, AQ * 4)); guard.bufs.push_back(d_c);
    std::vector<uint64_t> hrows(AQ);
    float* d_q2 = nullptr;          // the undecided rows of an assignment call, gathered (allocated on first use)

    auto assign = [&](std::vector<uint32_t>& out) -> int {  // assign_metric (kmeans.rs:237-264)
        if (guard.cen) { lynse_hip_flat_destroy(guard.cen); guard.cen = nullptr; }
        LY_TRY(lynse_hip_flat_create(dim, device, &guard.cen));
        LY_TRY(lynse_hip_flat_append_f32(guard.cen, cen.data(), k));
        LY_TRY(lynse_hip_flat_set_ip_form(guard.cen, LYNSE_IPFORM_SINGLE));  // compute_distance_f32 = single-row kernels
        // the assignment is a top-1 search of EVERY row against the centroids: thousands of rows per launch (one k_scan_h16
        // grid row per 256 of them) instead of one 4..16-workgroup launch set per 256 rows; candidate slots = the centroids
        if (k <= 16384) {
            uint32_t cap = 256;
            while (cap < k) cap <<= 1;
            // ONE emit-all stage over all centroids (the widened pass scores several 256-row chunks per launch and has no
            // threshold stages): stage 0 = the whole store — with the default 4096-row first stage more than 4096 centroids
            // made a two-stage plan the widened pass refuses (found by the n = 20,000 / nlist = 5,000 parity test)
            LY_TRY(lynse_hip_flat_set_plan(guard.cen, cap, guard.cen->growth, cap));
            guard.cen->qchunk = ASSIGN_QCHUNK;
        }
        // Round 5 (SURVEY 2a K9): the arg-best epilogue — lane-max scan + k_assign_pick (flat_assign_top1_device); only the rows whose two
        // best coarse centroids lie within the certified margin go through the exact top-1 search.  LYNSE_HIP_ASSIGN_FAST=0: every row
        // through the search (A/B; read per build)
        bool fast = k <= 16384 && env_on("LYNSE_HIP_ASSIGN_FAST", true);
        std::vector<uint32_t> hids(AQ), hredo(AQ);
        uint32_t* d_ids = reinterpret_cast<uint32_t*>(d_r);           // (AQ x 8 bytes: ids in the first half, the redo list in the second)
        uint32_t* d_redo = reinterpret_cast<uint32_t*>(d_r) + AQ;
        for (uint64_t r0 = 0; r0 < n; r0 += AQ) {
            const uint64_t nr = std::min<uint64_t>(AQ, n - r0);
            LY_TRY(lynse_hip_flat_copy_rows_device(data, r0, nr, d_q));
            if (fast) {
                const int frc = flat_assign_top1_device(guard.cen, d_q, nr, metric, d_ids, d_redo, d_c);
                if (frc == LYNSE_ERR_UNSUPPORTED) fast = false;
                else if (frc != LYNSE_OK) return frc;
            }
            if (fast) {
                uint32_t nredo = 0;
                LY_HIP(hipMemcpy(&nredo, d_c, 4, hipMemcpyDeviceToHost));
                LY_HIP(hipMemcpy(hids.data(), d_ids, nr * 4, hipMemcpyDeviceToHost));
                if (nredo) {   // undecided rows: gathered into the front of a second buffer, answered exactly, scattered back
                    if (!d_q2) { LY_HIP(hipMalloc(&d_q2, AQ * (size_t)dim * 4)); guard.bufs.push_back(d_q2); }
                    LY_HIP(hipMemcpy(hredo.data(), d_redo, (size_t)nredo * 4, hipMemcpyDeviceToHost));
                    hipLaunchKernelGGL(k_gather_rows_f32, dim3((uint32_t)std::min<uint64_t>(((uint64_t)nredo * ((dim + 3) / 4) + 255) / 256, 4096)), dim3(256), 0, st,
                                       d_q, dim, d_redo, (uint64_t)nredo, d_q2, dim, dim);
                    LY_HIP(hipGetLastError());
                    LY_HIP(hipStreamSynchronize(st));
                    LY_TRY(lynse_hip_flat_search_f32_device(guard.cen, d_q2, nredo, 1, metric, d_r, d_d, d_c, nullptr));
                    LY_HIP(hipMemcpy(hrows.data(), d_r, (size_t)nredo * 8, hipMemcpyDeviceToHost));
                    for (uint32_t i = 0; i < nredo; ++i) hids[hredo[i]] = (uint32_t)hrows[i];
                }
                for (uint64_t i = 0; i < nr; ++i) out[r0 + i] = hids[i];
                continue;
            }
            LY_TRY(lynse_hip_flat_search_f32_device(guard.cen, d_q, nr, 1, metric, d_r, d_d, d_c, nullptr));
            LY_HIP(hipMemcpy(hrows.data(), d_r, nr * 8, hipMemcpyDeviceToHost));
            for (uint64_t i = 0; i < nr; ++i) out[r0 + i] = (uint32_t)hrows[i];
        }
        return LYNSE_OK;
    };

    for (uint32_t it = 0; it < max_iter; ++it) {
        LY_TRY(assign(nxt));
        bool changed = nxt != cur;
        cur = nxt;
        std::vector<uint64_t> off(k + 1, 0);
        for (uint64_t i = 0; i < n; ++i) off[cur[i] + 1] += 1;
        std::vector<uint32_t> counts(k + 1);   // [k]: "an assignment changed on this rank" — the stop test of the whole collection rides along with the counts
        for (uint32_t c = 0; c < k; ++c) { counts[c] = (uint32_t)off[c + 1]; off[c + 1] += off[c]; }
        counts[k] = changed ? 1u : 0u;
        std::vector<uint32_t> members(n);
        {
            std::vector<uint64_t> wp(off.begin(), off.end() - 1);
            for (uint64_t i = 0; i < n; ++i) members[wp[cur[i]]++] = (uint32_t)i;
        }
        LY_HIP(hipMemcpyAsync(d_members, members.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
        LY_HIP(hipMemcpyAsync(d_off, off.data(), ((size_t)k + 1) * 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_kmeans_sums, dim3(k), dim3(256), 0, st, data->rows, ld, dim, d_members, d_off, d_sums, dim);
        LY_HIP(hipGetLastError());
        // per-rank sums (sequential over the rank's members) added over the ranks IN RANK ORDER; counts + stop test of the whole collection
        int rr = 0;
        if (sh && sh->reduce_iter) {   // the communicator: all-gather + rank-ordered add + integer all-reduce on device buffers, one read-back
            rr = sh->reduce_iter(d_sums, (uint64_t)k * dim, d_off, k, counts[k], st, sums.data(), counts.data());
        } else {
            LY_HIP(hipMemcpyAsync(sums.data(), d_sums, (size_t)k * dim * 4, hipMemcpyDeviceToHost, st));
            LY_HIP(hipStreamSynchronize(st));
            if (sh) {
                rr = sh->reduce(sums.data(), (uint64_t)k * dim, 2);
                if (rr == 0) rr = sh->reduce(counts.data(), (uint64_t)k + 1, 1);
            }
        }
        if (rr) return rr == 2 ? set_error(LYNSE_ERR_TIMEOUT, "the reduction of the centroid sums did not finish within the wait timeout (a rank is gone?)")
                               : set_error(LYNSE_ERR_DEVICE, "the reduction of the centroid sums failed");
        if (sh) changed = counts[k] != 0;
        uint32_t max_c = 0, max_count = 0;  // max_by_key keeps the LAST maximum (kmeans.rs:105-110)
        for (uint32_t c = 0; c < k; ++c)
            if (counts[c] >= max_count) { max_count = counts[c]; max_c = c; }
        for (uint32_t c = 0; c < k; ++c) {  // kmeans.rs:112-125 (in order: an empty cluster may read an already updated source)
            if (counts[c] > 0) {
                const float inv = 1.0f / (float)counts[c];
                for (uint32_t d = 0; d < dim; ++d) cen[(size_t)c * dim + d] = sums[(size_t)c * dim + d] * inv;
            } else if (max_count > 1) {
                for (uint32_t d = 0; d < dim; ++d) {
                    const float f = 1e-4f * (float)d;
                    const float g = 1.0f + f;
                    cen[(size_t)c * dim + d] = cen[(size_t)max_c * dim + d] * g;
                }
            }
        }
        if (!changed) break;
    }
    LY_TRY(assign(*assign_out));  // final re-assign (kmeans.rs:133)
    return LYNSE_OK;
}

extern "C" int lynse_hip_ivf_build(const float* rows, uint64_t n, uint32_t dim, uint32_t nlist, uint32_t max_iter, int metric,
                                   int l2_partitions, int device, lynse_hip_ivf** out) {
    LY_TRY(ivf_check_args(rows, n, dim, nlist, metric, out));
    if (l2_partitions && n < nlist)  // ivf_flat_mmap.rs:83-88
        return set_error(LYNSE_ERR_INVALID_ARGUMENT, "IVF requires at least as many vectors as partitions");
    std::vector<float> cen;
    std::vector<uint32_t> asg;
    uint32_t k = 0;
    if (metric >= M_HAMMING) {  // IVF-*-BINARY (ivf.rs:147-175): fit + encode, k-means with L2 on the codes
        if (l2_partitions) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "IvfFlat partitions are defined for ip / l2 / cosine");
        if (n == 0) return set_error(LYNSE_ERR_INDEX_NOT_BUILT, "no vectors to index");
        std::vector<float> thr, enc;
        int ab = 0;
        LY_TRY(bq_fit_encode(rows, n, dim, device, nullptr, &thr, &ab, &enc));
        LY_TRY(ivf_kmeans(enc.data(), n, dim, nlist, max_iter, M_L2, device, &cen, &asg, &k));
        LY_TRY(ivf_assemble(enc.data(), n, dim, cen.data(), k, asg.data(), metric, 0, device, out));
        const int rc = ivf_set_thresholds(*out, thr, ab);
        if (rc != LYNSE_OK) { ivf_free(*out); *out = nullptr; }
        return rc;
    }
    // IvfFlatMmap trains L2 Voronoi cells (ivf_flat_mmap.rs:98); IVFIndex trains with the routing metric (ivf.rs:163-170)
    LY_TRY(ivf_kmeans(rows, n, dim, nlist, max_iter, l2_partitions ? M_L2 : metric, device, &cen, &asg, &k));
    if (k == 0) return set_error(LYNSE_ERR_INDEX_NOT_BUILT, "no vectors to index");
    return ivf_assemble(rows, n, dim, cen.data(), k, asg.data(), metric, l2_partitions ? 1 : 0, device, out);
}

// Device-resident twins (float metrics): the rows are already in HBM — IvfFlatMmap::build reads them from an mmapped store
// (ivf_flat_mmap.rs:56-159), here from device memory: k-means, slab reordering (a gather inside HBM) and the store never
// touch host RAM with row data (a 6.25M x 768 shard of config 4 is 19 GB); centroids / assignments stay host-side state.
extern "C" int lynse_hip_ivf_build_device(const float* d_rows, uint64_t n, uint32_t dim, uint32_t nlist, uint32_t max_iter, int metric,
                                          int l2_partitions, int device, lynse_hip_ivf** out) {
    LY_TRY(ivf_check_args(d_rows, n, dim, nlist, metric, out));
    if (metric >= M_HAMMING) return set_error(LYNSE_ERR_UNSUPPORTED, "the device-resident IVF build takes ip / l2 / cosine (binary IVF builds from host rows)");
    if (l2_partitions && n < nlist) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "IVF requires at least as many vectors as partitions");
    if (n == 0) return set_error(LYNSE_ERR_INDEX_NOT_BUILT, "no vectors to index");
    std::vector<float> cen;
    std::vector<uint32_t> asg;
    uint32_t k = 0;
    LY_TRY(ivf_kmeans(d_rows, n, dim, nlist, max_iter, l2_partitions ? M_L2 : metric, device, &cen, &asg, &k, true));
    return ivf_assemble(d_rows, n, dim, cen.data(), k, asg.data(), metric, l2_partitions ? 1 : 0, device, out, true);
}

extern "C" int lynse_hip_ivf_load_device(const float* d_rows, uint64_t n, uint32_t dim, const float* centroids, uint32_t nlist,
                                         const uint32_t* assignments, int metric, int device, lynse_hip_ivf** out) {
    LY_TRY(ivf_check_args(d_rows, n, dim, nlist, metric, out));
    if (!centroids || (!assignments && n)) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    if (metric >= M_HAMMING) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "binary metrics load through lynse_hip_ivf_load_binary");
    return ivf_assemble(d_rows, n, dim, centroids, nlist, assignments, metric, 0, device, out, true);
}

// ---------------------------------------------------------------------------- IVF-*-SQ8 ----
// IVFIndex with QuantizerType::Scalar (ivf.rs:132-337, ScalarQuantizer quantizer/mod.rs:110-250): the quantizer is fitted on
// all rows, k-means (train_for_metric, routing metric = index metric) runs on decode(encode(rows)), the slab store holds those
// decoded rows — the pool stage of a search is the ordinary IVF scan over them with k = pool — and the original f32 rows stay
// in HBM (d_raw, original row order) for the exact rerank.  Kernels: k_ivfsq_* (kernels.h).

// ScalarQuantizer::fit over n rows in HBM (n > 0): mins, scales
static int sq_fit_device(const float* d_v, uint64_t n, uint32_t dim, std::vector<float>* mins, std::vector<float>* scales) {
    const uint32_t strips = (uint32_t)std::min<uint64_t>(n, 1024);
    float* d_p = nullptr;
    struct G { float*& p; ~G() { if (p) (void)hipFree(p); } } g{d_p};
    LY_HIP(hipMalloc(&d_p, ((size_t)strips * 2 + 2) * dim * 4));
    float* d_o = d_p + (size_t)strips * 2 * dim;
    hipLaunchKernelGGL(k_ivfsq_minmax, dim3((dim + 255) / 256, strips), dim3(256), 0, 0, d_v, dim, n, d_p, d_p + (size_t)strips * dim);
    hipLaunchKernelGGL(k_ivfsq_fit, dim3((dim + 255) / 256), dim3(256), 0, 0, d_p, d_p + (size_t)strips * dim, dim, strips, d_o, d_o + dim);
    LY_HIP(hipGetLastError());
    std::vector<float> o((size_t)dim * 2);
    LY_HIP(hipMemcpy(o.data(), d_o, (size_t)dim * 8, hipMemcpyDeviceToHost));
    mins->assign(o.begin(), o.begin() + dim);
    scales->assign(o.begin() + dim, o.end());
    return LYNSE_OK;
}

// encode -> decode of n rows (HBM -> HBM, in place allowed) with the quantizer d_sq = [min | scale]
static int sq_codec_device(const float* d_in, uint64_t n, uint32_t dim, const float* d_sq, float* d_out, hipStream_t st) {
    if (n == 0) return LYNSE_OK;
    const uint64_t total = n * dim;
    hipLaunchKernelGGL(k_ivfsq_codec, dim3((uint32_t)std::min<uint64_t>((total + 255) / 256, 8192)), dim3(256), 0, st,
                       d_in, n, dim, d_sq, d_sq + dim, d_out, (uint8_t*)nullptr);
    LY_HIP(hipGetLastError());
    return LYNSE_OK;
}

// decode(encode(rows)) of host rows for an SQ8 index (host copy unless dec is NULL): the routing space of insert / assign
static int sq_decode_host(const lynse_hip_ivf* h, const float* rows, uint64_t n, std::vector<float>* dec, float** d_keep = nullptr) {
    if (dec) dec->resize((size_t)n * h->dim);
    if (n == 0) return LYNSE_OK;
    LY_HIP(hipSetDevice(h->store->device));   // (h->d_sq lives on the index's device, whatever the calling thread's current one is)
    float* d_v = nullptr;
    struct G { float*& p; ~G() { if (p) (void)hipFree(p); } } g{d_v};
    LY_HIP(hipMalloc(&d_v, (size_t)n * h->dim * 8));
    LY_TRY(h2d_done(d_v, rows, (size_t)n * h->dim * 4));
    LY_TRY(sq_codec_device(d_v, n, h->dim, h->d_sq, d_v + (size_t)n * h->dim, 0));
    if (dec) LY_HIP(hipMemcpy(dec->data(), d_v + (size_t)n * h->dim, (size_t)n * h->dim * 4, hipMemcpyDeviceToHost));
    else LY_HIP(hipStreamSynchronize(nullptr));
    if (d_keep) { *d_keep = d_v; d_v = nullptr; }   // (the caller takes the buffer: originals first, decoded rows behind them)
    return LYNSE_OK;
}

// the common part of build_sq8 / load_sq8: original rows uploaded, quantizer on the device, decoded rows beside them
static int sq_prepare(const float* rows, uint64_t n, uint32_t dim, const float* mins_in, const float* scales_in, int device,
                      float** d_raw, float** d_dec, float** d_sq, std::vector<float>* mins, std::vector<float>* scales) {
    LY_HIP(hipSetDevice(device));
    LY_HIP(hipMalloc(d_raw, std::max<size_t>((size_t)n * dim * 4, 4)));
    LY_HIP(hipMalloc(d_dec, std::max<size_t>((size_t)n * dim * 4, 4)));
    LY_HIP(hipMalloc(d_sq, (size_t)dim * 8));
    if (n) LY_TRY(h2d_done(*d_raw, rows, (size_t)n * dim * 4));
    if (mins_in) {
        mins->assign(mins_in, mins_in + dim);
        scales->assign(scales_in, scales_in + dim);
    } else {
        LY_TRY(sq_fit_device(*d_raw, n, dim, mins, scales));
    }
    LY_TRY(h2d_done(*d_sq, mins->data(), (size_t)dim * 4));
    LY_TRY(h2d_done(*d_sq + dim, scales->data(), (size_t)dim * 4));
    LY_TRY(sq_codec_device(*d_raw, n, dim, *d_sq, *d_dec, 0));
    LY_HIP(hipStreamSynchronize(nullptr));
    return LYNSE_OK;
}

static int ivf_sq8_common(const float* rows, uint64_t n, uint32_t dim, const float* centroids, uint32_t nlist, const uint32_t* assignments,
                          const float* mins_in, const float* scales_in, uint32_t max_iter, int metric, int device, lynse_hip_ivf** out) {
    if (metric != M_IP && metric != M_L2 && metric != M_COS)
        return set_error(LYNSE_ERR_INVALID_ARGUMENT, "IVF-*-SQ8 is defined for ip / l2 / cosine");
    if (n == 0) return set_error(LYNSE_ERR_INDEX_NOT_BUILT, "no vectors to index");   // ScalarQuantizer::fit: empty training data
    float *d_raw = nullptr, *d_dec = nullptr, *d_sq = nullptr;
    struct G { float*& a; float*& b; float*& c; ~G() { for (float* p : {a, b, c}) if (p) (void)hipFree(p); } } g{d_raw, d_dec, d_sq};
    std::vector<float> mins, scales, cen;
    std::vector<uint32_t> asg;
    LY_TRY(sq_prepare(rows, n, dim, mins_in, scales_in, device, &d_raw, &d_dec, &d_sq, &mins, &scales));
    if (!centroids) {   // train_for_metric on the decoded rows (ivf.rs:163-170)
        uint32_t k = 0;
        LY_TRY(ivf_kmeans(d_dec, n, dim, nlist, max_iter, metric, device, &cen, &asg, &k, true));
        if (k == 0) return set_error(LYNSE_ERR_INDEX_NOT_BUILT, "no vectors to index");
        nlist = k;
        centroids = cen.data();
        assignments = asg.data();
    }
    LY_TRY(ivf_assemble(d_dec, n, dim, centroids, nlist, assignments, metric, 0, device, out, true));
    lynse_hip_ivf* h = *out;
    h->sq8 = true;
    h->sq_min = std::move(mins);
    h->sq_scale = std::move(scales);
    std::swap(h->d_sq, d_sq);
    std::swap(h->d_raw, d_raw);
    return LYNSE_OK;
}

extern "C" int lynse_hip_ivf_build_sq8(const float* rows, uint64_t n, uint32_t dim, uint32_t nlist, uint32_t max_iter, int metric, int device,
                                       lynse_hip_ivf** out) {
    LY_TRY(ivf_check_args(rows, n, dim, nlist, metric, out));
    return ivf_sq8_common(rows, n, dim, nullptr, nlist, nullptr, nullptr, nullptr, max_iter, metric, device, out);
}

extern "C" int lynse_hip_ivf_load_sq8(const float* rows, uint64_t n, uint32_t dim, const float* centroids, uint32_t nlist,
                                      const uint32_t* assignments, const float* mins, const float* scales, int metric, int device,
                                      lynse_hip_ivf** out) {
    LY_TRY(ivf_check_args(rows, n, dim, nlist, metric, out));
    if (!centroids || (!assignments && n) || !mins || !scales) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    return ivf_sq8_common(rows, n, dim, centroids, nlist, assignments, mins, scales, 0, metric, device, out);
}

extern "C" int lynse_hip_ivf_sq8_params(const lynse_hip_ivf* h, float* mins, float* scales) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "not an IVF-*-SQ8 index");
    IVF_GUARD(h);
    if (!h->sq8) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "not an IVF-*-SQ8 index");
    if (mins) memcpy(mins, h->sq_min.data(), h->sq_min.size() * 4);
    if (scales) memcpy(scales, h->sq_scale.data(), h->sq_scale.size() * 4);
    return LYNSE_OK;
}

extern "C" int lynse_hip_ivf_sq8_stage_times(lynse_hip_ivf* h, double* out3, int reset) {
    if (!h || !out3) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    IVF_GUARD(h);
    if (!h->sq8) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "not an IVF-*-SQ8 index");
    out3[0] = (double)h->sq_searches;
    out3[1] = h->sq_pool_us;
    out3[2] = h->sq_rerank_us;
    if (reset) { h->sq_searches = 0; h->sq_pool_us = 0.0; h->sq_rerank_us = 0.0; }
    return LYNSE_OK;
}

// ------------------------------------------------------------------- incremental insert / delete ----
// IVFIndex::insert (ivf.rs:392-441): new vectors go through the quantizer (binary modes), are assigned to the EXISTING
// centroids with the routing metric — compute_distance_f32 against every centroid in ascending order, strictly-better wins —
// and are appended to their list (new row ids are the largest: lists stay in ascending row order).  IVFIndex::delete
// (ivf.rs:350-390): the remaining vectors keep their order, get consecutive row ids and are ALL reassigned to the existing
// centroids (kmeans::assign_metric).  No retraining in either.
//
// The assignment is the (score, centroid id) top-1 of a FLAT search over the centroid store with the single-row kernels:
// the same arithmetic and the same tie rule as the reference's loop (the first of equally good centroids wins).
static int ivf_assign_rows(lynse_hip_ivf* h, const float* rows /* routing space: codes for a binary index */, uint64_t n, uint32_t* out) {
    if (n == 0) return LYNSE_OK;
    const int route_metric = h->binary ? M_L2 : h->metric;   // routing_metric (ivf.rs:77-87)
    std::vector<uint64_t> best(n);
    std::vector<float> bd(n);
    std::vector<uint32_t> bc(n);
    LY_TRY(lynse_hip_flat_search_f32(h->cstore, rows, n, 1, route_metric, best.data(), bd.data(), bc.data()));
    for (uint64_t i = 0; i < n; ++i) out[i] = bc[i] ? (uint32_t)best[i] : 0u;
    return LYNSE_OK;
}

// quantizer.encode -> decode of a binary index (ivf.rs:398-404): values above the fitted threshold become 1.0, else 0.0
static void ivf_encode_rows(const lynse_hip_ivf* h, const float* rows, uint64_t n, std::vector<float>* enc) {
    enc->resize((size_t)n * h->dim);
    for (uint64_t r = 0; r < n; ++r)
        for (uint32_t d = 0; d < h->dim; ++d) (*enc)[(size_t)r * h->dim + d] = rows[(size_t)r * h->dim + d] > h->bq_thr[d] ? 1.0f : 0.0f;
}

extern "C" int lynse_hip_ivf_assign_f32(lynse_hip_ivf* h, const float* rows, uint64_t n, uint32_t* out_assignments) {
    if (!h) return set_error(LYNSE_ERR_INDEX_NOT_BUILT, "IVF index is not built");
    IVF_GUARD(h);   // (insert / delete replace the centroid store too)
    if (!h->store || !h->cstore) return set_error(LYNSE_ERR_INDEX_NOT_BUILT, "IVF index is not built");
    if (h->spann) return set_error(LYNSE_ERR_UNSUPPORTED, "assign is defined for one list per row, not for a SPANN index");
    if (n && (!rows || !out_assignments)) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!h->binary && !h->sq8) return ivf_assign_rows(h, rows, n, out_assignments);
    std::vector<float> enc;
    if (h->sq8) LY_TRY(sq_decode_host(h, rows, n, &enc));
    else ivf_encode_rows(h, rows, n, &enc);
    return ivf_assign_rows(h, enc.data(), n, out_assignments);
}

// the rows of the store in ORIGINAL row order (host copy; a binary index stores the {0,1} codes)
static int ivf_rows_in_original_order(lynse_hip_ivf* h, std::vector<float>* out) {
    const uint64_t n = h->store->n;
    const uint32_t dim = h->dim;
    out->resize((size_t)n * dim);
    const uint64_t chunk = std::max<uint64_t>(1, (64ull << 20) / ((uint64_t)dim * 4));
    std::vector<float> stage((size_t)std::min<uint64_t>(chunk, std::max<uint64_t>(n, 1)) * dim);
    for (uint64_t p0 = 0; p0 < n; p0 += chunk) {
        const uint64_t np_ = std::min<uint64_t>(chunk, n - p0);
        LY_TRY(lynse_hip_flat_read_rows(h->store, p0, np_, stage.data()));
        for (uint64_t i = 0; i < np_; ++i) memcpy(&(*out)[(size_t)h->orig[p0 + i] * dim], &stage[(size_t)i * dim], (size_t)dim * 4);
    }
    return LYNSE_OK;
}

// replace the device structures of `h` with a fresh assembly over (rows, assignments) under the SAME centroids / settings
// (new_raw: an SQ8 index's original rows for the new assembly, n x dim in original row order; owned by the index on success)
// hand the settings of `h` to a fresh assembly `fresh` under the same centroids, then swap them: `h` owns the new structures, the old
// ones are freed (new_raw as in ivf_reassemble)
static int ivf_adopt(lynse_hip_ivf* h, lynse_hip_ivf* fresh, float* new_raw) {
    fresh->no_fallback = h->no_fallback;
    fresh->row_stride = h->row_stride; fresh->row_offset = h->row_offset;
    fresh->store->no_fused = h->store->no_fused;
    if (h->binary) {
        const int rc = ivf_set_thresholds(fresh, h->bq_thr, h->already_binary);
        if (rc != LYNSE_OK) { ivf_free(fresh); return rc; }
    }
    if (h->sq8) {   // the quantizer moves over unchanged (insert does not refit, ivf.rs:392-441); the new original rows come with the call
        fresh->sq8 = true;
        fresh->sq_min = h->sq_min; fresh->sq_scale = h->sq_scale;
        std::swap(fresh->d_sq, h->d_sq);
        fresh->d_raw = new_raw;
        fresh->sq_searches = h->sq_searches; fresh->sq_pool_us = h->sq_pool_us; fresh->sq_rerank_us = h->sq_rerank_us;
    }
    fresh->spann = h->spann;
    fresh->replicas = h->replicas;   // (n_rows is the caller's to set)
    // (profiling state of the old store carries over: it used to be dropped silently)
    fresh->store->profiling = h->store->profiling.load();
    fresh->store->prof_rate = h->store->prof_rate.load();
    {
        std::lock_guard<std::mutex> p1(h->store->prof_mu);
        fresh->store->prof = h->store->prof;
    }
    {
        std::lock_guard<std::mutex> gfl(g_ivf_guard_mu);   // (nobody copies the guard field while it is swapped away and back)
        std::swap(*h, *fresh);   // the caller's handle now owns the new structures, `fresh` the old ones
        std::swap(h->guard, fresh->guard);   // ... and keeps its own guard (the caller holds it locked)
    }
    ivf_free(fresh);
    return LYNSE_OK;
}

static int ivf_reassemble(lynse_hip_ivf* h, const std::vector<float>& rows, uint64_t n, const std::vector<uint32_t>& asg, const IvfRowSource* rs = nullptr,
                          float* new_raw = nullptr) {
    lynse_hip_ivf* fresh = nullptr;
    const int device = h->store->device;
    LY_TRY(ivf_assemble(rs ? nullptr : rows.data(), n, h->dim, h->centroids.data(), h->nlist, asg.data(), h->metric, h->ivfflat_routing, device, &fresh, false, rs));
    return ivf_adopt(h, fresh, new_raw);
}

static int spann_insert(lynse_hip_ivf* h, const float* rows, uint64_t n);
static int spann_delete(lynse_hip_ivf* h, const uint64_t* row_ids, uint64_t n_ids);

extern "C" int lynse_hip_ivf_insert_f32(lynse_hip_ivf* h, const float* rows, uint64_t n) {
    if (!h) return set_error(LYNSE_ERR_INDEX_NOT_BUILT, "IVF index is not built");
    const std::shared_ptr<std::mutex> guard = ivf_guard_of(h);
    std::lock_guard<std::mutex> glk(*guard);   // (a search on another thread must not see the store being replaced)
    if (!h->store || !h->cstore) return set_error(LYNSE_ERR_INDEX_NOT_BUILT, "IVF index is not built");
    // IvfFlatMmap has no insert (ivf_flat_mmap.rs: build-once slabs); its cells are L2 cells whatever the index metric, so the
    // IVFIndex rule "assign with the index metric" (ivf.rs:350-388) would put rows into the wrong lists
    if (h->ivfflat_routing) return set_error(LYNSE_ERR_UNSUPPORTED, "insert is defined for IVFIndex, not for IvfFlat (L2-partitioned) indexes");
    if (h->inflight != 0) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "searches are in flight on this index: wait for the outstanding tickets first");
    if (n == 0) return LYNSE_OK;
    if (!rows) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "rows is NULL");
    if (h->spann) return spann_insert(h, rows, n);
    const uint64_t old_n = h->store->n;
    if (old_n + n > 0xfffffff0ull) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "IVF vector count exceeds the u32 ID capacity");
    std::vector<float> enc_new;
    const float* routed = rows;
    if (h->binary) { ivf_encode_rows(h, rows, n, &enc_new); routed = enc_new.data(); }
    float* new_raw = nullptr;   // SQ8: the original rows of the grown index (old ones + the new ones, original row order)
    struct FreeRaw { float*& p; ~FreeRaw() { if (p) (void)hipFree(p); } } fraw{new_raw};
    if (h->sq8) {   // encode with the FITTED quantizer (no refit: values outside its range clamp), route the decoded rows
        float* d_new = nullptr;
        struct G { float*& p; ~G() { if (p) (void)hipFree(p); } } g{d_new};
        LY_HIP(hipSetDevice(h->store->device));
        LY_TRY(sq_decode_host(h, rows, n, &enc_new, &d_new));
        routed = enc_new.data();
        LY_HIP(hipMalloc(&new_raw, (size_t)(old_n + n) * h->dim * 4));
        if (old_n) LY_HIP(hipMemcpy(new_raw, h->d_raw, (size_t)old_n * h->dim * 4, hipMemcpyDeviceToDevice));
        LY_HIP(hipMemcpy(new_raw + (size_t)old_n * h->dim, d_new, (size_t)n * h->dim * 4, hipMemcpyDeviceToDevice));
    }
    std::vector<uint32_t> asg(h->assignments);
    asg.resize(old_n + n);
    LY_TRY(ivf_assign_rows(h, routed, n, asg.data() + old_n));
    // the indexed rows never leave HBM: the new slab store gathers them from the old one, only the n new rows are uploaded
    // (the old and the new store exist side by side until the swap, as before)
    std::vector<uint32_t> old_pos(old_n + n, 0xffffffffu);
    for (uint64_t p = 0; p < old_n; ++p) old_pos[h->orig[p]] = (uint32_t)p;
    IvfRowSource rs{h->store->rows, h->store->ld, old_pos.data(), routed, old_n, n};
    static const std::vector<float> none;
    LY_TRY(ivf_reassemble(h, none, old_n + n, asg, &rs, new_raw));
    new_raw = nullptr;   // (owned by the index now)
    return LYNSE_OK;
}

extern "C" int lynse_hip_ivf_delete_rows(lynse_hip_ivf* h, const uint64_t* row_ids, uint64_t n_ids) {
    if (!h) return set_error(LYNSE_ERR_INDEX_NOT_BUILT, "IVF index is not built");
    const std::shared_ptr<std::mutex> guard = ivf_guard_of(h);
    std::lock_guard<std::mutex> glk(*guard);
    if (!h->store || !h->cstore) return set_error(LYNSE_ERR_INDEX_NOT_BUILT, "IVF index is not built");
    if (h->ivfflat_routing) return set_error(LYNSE_ERR_UNSUPPORTED, "delete is defined for IVFIndex, not for IvfFlat (L2-partitioned) indexes");
    if (h->inflight != 0) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "searches are in flight on this index: wait for the outstanding tickets first");
    if (n_ids == 0) return LYNSE_OK;
    if (!row_ids) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "row_ids is NULL");
    if (h->spann) return spann_delete(h, row_ids, n_ids);
    const uint64_t old_n = h->store->n;
    std::vector<bool> gone(old_n, false);
    for (uint64_t i = 0; i < n_ids; ++i)
        if (row_ids[i] < old_n) gone[row_ids[i]] = true;   // unknown ids are ignored (a HashSet lookup that never matches)
    float* new_raw = nullptr;   // SQ8: the original rows that are kept, in order (the decoded ones are reassigned below)
    struct FreeRaw { float*& p; ~FreeRaw() { if (p) (void)hipFree(p); } } fraw{new_raw};
    if (h->sq8) {
        std::vector<uint32_t> keep;
        keep.reserve(old_n);
        for (uint64_t r = 0; r < old_n; ++r)
            if (!gone[r]) keep.push_back((uint32_t)r);
        LY_HIP(hipSetDevice(h->store->device));
        uint32_t* d_keep = nullptr;
        struct G { uint32_t*& p; ~G() { if (p) (void)hipFree(p); } } g{d_keep};
        LY_HIP(hipMalloc(&new_raw, std::max<size_t>(keep.size() * h->dim * 4, 4)));
        if (!keep.empty()) {
            LY_HIP(hipMalloc(&d_keep, keep.size() * 4));
            LY_TRY(h2d_done(d_keep, keep.data(), keep.size() * 4));
            const uint64_t pieces = (uint64_t)keep.size() * ((h->dim + 3) / 4);
            hipLaunchKernelGGL(k_gather_rows_f32, dim3((uint32_t)std::min<uint64_t>((pieces + 255) / 256, 8192)), dim3(256), 0, 0,
                               h->d_raw, h->dim, d_keep, (uint64_t)keep.size(), new_raw, h->dim, h->dim);
            LY_HIP(hipGetLastError());
            LY_HIP(hipStreamSynchronize(nullptr));
        }
    }
    if (h->store->ld == h->dim && old_n) {
        // Rows stay in HBM (as in insert): kmeans::assign_metric over everything that is left = the top-1 of a FLAT search over the
        // centroid store with the slab rows themselves as device queries (every old slab position; the deleted ones are dropped
        // afterwards), then the re-assembled store gathers the kept rows from the old one.
        LY_HIP(hipSetDevice(h->store->device));
        uint64_t* d_r = nullptr; float* d_d = nullptr; uint32_t* d_c = nullptr;
        struct Free { uint64_t*& a; float*& b; uint32_t*& c; ~Free() { if (a) (void)hipFree(a); if (b) (void)hipFree(b); if (c) (void)hipFree(c); } } fr{d_r, d_d, d_c};
        LY_HIP(hipMalloc(&d_r, (size_t)old_n * 8));
        LY_HIP(hipMalloc(&d_d, (size_t)old_n * 4));
        LY_HIP(hipMalloc(&d_c, (size_t)old_n * 4));
        const int route_metric = h->binary ? M_L2 : h->metric;   // routing_metric (ivf.rs:77-87)
        LY_TRY(lynse_hip_flat_search_f32_device(h->cstore, h->store->rows, old_n, 1, route_metric, d_r, d_d, d_c, nullptr));
        std::vector<uint64_t> best(old_n);
        std::vector<uint32_t> cnt(old_n);
        LY_HIP(hipMemcpy(best.data(), d_r, (size_t)old_n * 8, hipMemcpyDeviceToHost));
        LY_HIP(hipMemcpy(cnt.data(), d_c, (size_t)old_n * 4, hipMemcpyDeviceToHost));
        std::vector<uint32_t> pos_of_orig(old_n);
        for (uint64_t p = 0; p < old_n; ++p) pos_of_orig[h->orig[p]] = (uint32_t)p;
        std::vector<uint32_t> asg, old_pos;
        asg.reserve(old_n); old_pos.reserve(old_n);
        for (uint64_t r = 0; r < old_n; ++r)
            if (!gone[r]) {
                const uint32_t p = pos_of_orig[r];
                old_pos.push_back(p);
                asg.push_back(cnt[p] ? (uint32_t)best[p] : 0u);
            }
        IvfRowSource rs{h->store->rows, h->store->ld, old_pos.data(), nullptr, (uint64_t)old_pos.size(), 0};
        static const std::vector<float> none;
        LY_TRY(ivf_reassemble(h, none, old_pos.size(), asg, &rs, new_raw));
        new_raw = nullptr;
        return LYNSE_OK;
    }
    std::vector<float> all;
    LY_TRY(ivf_rows_in_original_order(h, &all));
    std::vector<float> kept;
    kept.reserve(all.size());
    uint64_t m = 0;
    for (uint64_t r = 0; r < old_n; ++r)
        if (!gone[r]) { kept.insert(kept.end(), all.begin() + (size_t)r * h->dim, all.begin() + (size_t)(r + 1) * h->dim); ++m; }
    std::vector<uint32_t> asg(m);
    LY_TRY(ivf_assign_rows(h, kept.data(), m, asg.data()));   // kmeans::assign_metric over everything that is left
    LY_TRY(ivf_reassemble(h, kept, m, asg, nullptr, new_raw));
    new_raw = nullptr;
    return LYNSE_OK;
}

// ------------------------------------------------------------------------------------ search ----
template <typename T>
static int ivf_grow(T** p, size_t* cap, size_t need) {
    if (need <= *cap) return LYNSE_OK;
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    size_t nc = std::max(need, *cap * 2);
    LY_HIP(hipMalloc(p, nc * sizeof(T)));
    *cap = nc;
    return LYNSE_OK;
}

static int launch_scan_tiled(const ScanArgs& a, int metric, uint32_t grid, hipStream_t st) {
    return launch_scan_h16<with(F16_SMALL, &H16Cfg::tiled, true)>(a, metric, grid, st);
}

// The probed lists of nq queries staged in the workspace (w.Qf): probes[q * np_eff + r] = the r-th list of query q.
// Exact ranking of all centroids (ivf.rs:227-249) = the (score, centroid id) top-nprobe of a FLAT search over the centroid
// store; IvfFlatMmap's IP heuristic (ivf_flat_mmap.rs:381-421) is k_ivf_route mode 1; nprobe >= nlist probes everything.
// A search IN FLIGHT (lynse_hip_ivf_search_submit_f32_device): the staged pipeline is only ENQUEUED — no host synchronisation, the
// centroid ranking included — and everything the blocking path would have looked at on the host (candidate overflow of the scan or of
// the centroid ranking, the all-lists-empty flag) is OR-ed into one device status word + left in the pinned headers for wait().
struct IvfAsync {
    uint32_t* status;        // device word the flags are OR-ed into (part of the result block of a sharded ticket), or nullptr
    bool routed_by_chunk;    // out: the centroid ranking ran through run_chunk (its overflow flags are in the centroid store's pinned header)
};

static int ivf_route(lynse_hip_ivf* h, uint32_t nq, uint32_t np_eff, int metric, int route_metric, hipStream_t st, std::vector<uint32_t>* probes_out,
                     const uint64_t** dev64 = nullptr, const uint32_t** dev32 = nullptr, IvfAsync* as = nullptr) {
    // dev64 / dev32 (np_eff < nlist only): leave the probes in device memory — the centroid ranking as u64 row ids of the centroid
    // store, or k_ivf_route's u32 list — and skip the copy to the host (device-side grouping, k_ivf_group)
    lynse_hip_flat* s = h->store;
    Workspace& w = cur(s).ws;
    IvfScratch& scr = iscr(h);
    const uint32_t D = h->dim;
    LY_TRY(ivf_grow(&scr.d_probes, &scr.probes_cap, (size_t)nq * np_eff));
    std::vector<uint32_t>& probes = *probes_out;
    probes.assign((size_t)nq * np_eff, 0u);
    const bool heuristic = h->ivfflat_routing && metric == M_IP && D >= 64 && h->nlist >= 64 && !h->rdims.empty() && np_eff < h->nlist;
    if (np_eff >= h->nlist) {
        for (uint32_t q = 0; q < nq; ++q)
            for (uint32_t c = 0; c < h->nlist; ++c) probes[(size_t)q * np_eff + c] = c;  // ivf_flat_mmap.rs:390-392
    } else if (!heuristic) {
        // ---- exact ranking of all centroids (ivf.rs:227-249) = the (score, centroid id) top-nprobe of a FLAT search
        // over the centroid matrix: MFMA coarse pass + exact rescoring instead of nlist sequential scores per query
        if ((size_t)nq * np_eff > scr.route_cap) {
            for (void* p : {(void*)scr.d_route_rows, (void*)scr.d_route_d, (void*)scr.d_route_c})
                if (p) (void)hipFree(p);
            scr.d_route_rows = nullptr; scr.d_route_d = nullptr; scr.d_route_c = nullptr; scr.route_cap = 0;
            const size_t cap = std::max<size_t>((size_t)nq * np_eff, (size_t)QCHUNK * np_eff);
            LY_HIP(hipMalloc(&scr.d_route_rows, cap * 8));
            LY_HIP(hipMalloc(&scr.d_route_d, cap * 4));
            LY_HIP(hipMalloc(&scr.d_route_c, (size_t)QCHUNK * 4));
            scr.route_cap = cap;
        }
        if (as) {
            // in flight: ONE plan level of the centroid store's own pipeline (or its fused few-query kernel) on the ticket's stream, with
            // the workspace of the centroid store's context of the same slot; an overflow of it is part of the ticket's status
            lynse_hip_flat* cs = h->cstore;
            Workspace& cw = cur(cs).ws;
            if (small_path_ok(cs, nq, np_eff, route_metric, false)) {
                LY_TRY(run_small(cs, nq, np_eff, np_eff, route_metric, st, nullptr, scr.d_route_rows, scr.d_route_d, scr.d_route_c, cw.h_hdr + cw.qcap, w.Qf));
                as->routed_by_chunk = false;
            } else {
                ScanProf sprof;
                ChunkReq rq;
                rq.nq = nq; rq.k = rq.out_k = np_eff; rq.metric = route_metric; rq.qsrc = w.Qf; rq.allow_sts = false;
                rq.out.rows = scr.d_route_rows; rq.out.dists = scr.d_route_d; rq.out.counts2 = scr.d_route_c; rq.out.any_ovf = as->status; rq.out.hdr_direct = true;
                LY_TRY(run_chunk(cs, rq, st, &sprof));
                as->routed_by_chunk = true;
            }
            *dev64 = scr.d_route_rows;
            return LYNSE_OK;
        }
        LY_TRY(search_impl(h->cstore, w.Qf, false, nq, np_eff, route_metric, scr.d_route_rows, scr.d_route_d, scr.d_route_c, true, st));
        if (dev64) { *dev64 = scr.d_route_rows; return LYNSE_OK; }
        std::vector<uint64_t> rr((size_t)nq * np_eff);
        LY_HIP(hipMemcpyAsync(rr.data(), scr.d_route_rows, rr.size() * 8, hipMemcpyDeviceToHost, st));
        LY_HIP(hipStreamSynchronize(st));
        for (size_t i = 0; i < rr.size(); ++i) probes[i] = (uint32_t)rr[i];
    } else {
        RouteArgs ra{};
        ra.Qf = w.Qf; ra.D = D; ra.C = h->d_centroids; ra.ldc = h->ldc; ra.nlist = h->nlist; ra.metric = route_metric;
        ra.nprobe = np_eff; ra.mode = heuristic ? 1 : 0; ra.rdims = h->d_rdims; ra.nrd = (uint32_t)h->rdims.size();
        ra.shortlist = std::min<uint32_t>(std::max<uint32_t>(np_eff * 3, 24), 96);  // ivf_flat_mmap.rs:395
        LY_TRY(ensure_lds<k_ivf_route<256>>(16384 * 8));
        uint32_t np2 = 2;
        while (np2 < h->nlist) np2 <<= 1;
        ra.probes = scr.d_probes;
        hipLaunchKernelGGL(k_ivf_route<256>, dim3(nq), dim3(256), (size_t)np2 * 8, st, ra);
        LY_HIP(hipGetLastError());
        if (dev32) { *dev32 = scr.d_probes; return LYNSE_OK; }
        LY_HIP(hipMemcpyAsync(probes.data(), scr.d_probes, probes.size() * 4, hipMemcpyDeviceToHost, st));
        LY_HIP(hipStreamSynchronize(st));
    }

    return LYNSE_OK;
}

// LYNSE_HIP_IVF_DEVICE_GROUPING=0: the probed lists are grouped on the host (A/B; read per call: tests flip it)
static int ivf_device_grouping() { return env_int("LYNSE_HIP_IVF_DEVICE_GROUPING", 1); }

static int ivf_search_chunk_staged(lynse_hip_ivf* h, const float* q_host, uint32_t nq, uint32_t k, uint32_t out_k, uint32_t nprobe,
                                   uint64_t* out_rows, float* out_dists, uint32_t* out_counts, bool safe, bool* overflowed,
                                   const uint32_t* smask, const std::vector<uint64_t>* list_matches, bool on_device, bool i8c, bool force_host = false,
                                   IvfAsync* as = nullptr);

// The certified int8 coarse pass for the staged IVF path: the FLAT rules (i8c_eligible, lynse_hip.hip: f32 slab of >= 64K rows,
// 33..256 queries, IP from any dimension / L2 and cosine from 256 dimensions on, not struck out, LYNSE_HIP_COARSE=i8 / f16
// forces / disables) + whole 128-column slabs (the tiled kernel is compiled without the ragged last slab; the augmented L2
// codes always are).
static bool ivf_i8c_eligible(const lynse_hip_ivf* h, int metric, uint32_t nq, bool safe, bool filtered) {
    const lynse_hip_flat* s = h->store;
    return !h->binary && !safe && !filtered && i8c_eligible(s, metric, false, nq, false, false, true) && (metric == M_L2 ? s->dim >= 256 : s->ld8 % 128 == 0);   // (L2: the augmented codes — the plain-code form of l2_plain is a FLAT tiling)
}

static int ivf_search_chunk(lynse_hip_ivf* h, const float* q_host, uint32_t nq, uint32_t k, uint32_t out_k, uint32_t nprobe,
                            uint64_t* out_rows, float* out_dists, uint32_t* out_counts, bool safe, bool* overflowed,
                            const uint32_t* smask = nullptr, const std::vector<uint64_t>* list_matches = nullptr, bool on_device = false) {
    // on_device: queries and outputs are device pointers (lynse_hip_ivf_search_f32_device)
    // smask / list_matches: SearchParams.subset (ivf.rs:251-265) as a slab-position mask + matches per list
    lynse_hip_flat* s = h->store;
    Workspace& w = cur(s).ws;
    hipStream_t st = cur(s).stream;
    const int metric = h->search_metric >= 0 ? h->search_metric : h->metric;  // IvfFlatMmap::search takes the metric per call
    IvfScratch& scr = iscr(h);
    const bool binary = h->binary;
    const int route_metric = binary ? M_L2 : metric;  // routing_metric (ivf.rs:77-87)
    const uint32_t D = h->dim;

    // ---- a few queries (single-query latency is the reference's usual IVF call): TWO launches, no host round trip —
    // the fused exact search (k_small_search) ranks the centroids, then scans the probed lists straight from the ranking
    // it left in device memory, every row scored exactly from the f32 slab in (distance, original row) order; results
    // land in the caller's device buffers or in pinned memory.  Same results as the staged path below (both are the exact
    // top-k of the probed rows); the all-lists-empty fallback of IVFIndex is flagged and rerun through the staged path.
    {
        const uint32_t np_f = std::min<uint32_t>(nprobe, h->nlist);
        const bool heuristic_f = h->ivfflat_routing && metric == M_IP && D >= 64 && h->nlist >= 64 && !h->rdims.empty();
        if (fused_env() && !s->no_fused && !binary && !smask && !safe && nq <= (uint32_t)SMALL_MAX_Q && k <= (uint32_t)SMALL_MAX_K &&
            np_f < h->nlist && np_f <= (uint32_t)SMALL_MAX_K && !heuristic_f && s->dtype == LYNSE_DTYPE_F32 &&
            // (the probed lists are scored exactly from the f32 slab: at most the np_f largest lists — 1 GB is ~0.3 ms of this kernel;
            // the bound used to be max_list_len x nprobe <= 256 MB, which uneven k-means lists exceed long before the rows do)
            (uint64_t)h->nlist * h->cstore->ld * 4 * nq <= (64ull << 20) && h->worst_rows[np_f] * s->ld * 4 * nq <= (1024ull << 20) &&
            (size_t)((D + 3) / 4 * 4) * 4 + (size_t)128 * 1024 + 64 <= 150u * 1024u) {
            const float* d_q = on_device ? q_host : w.Qf;
            if (!on_device) LY_HIP(hipMemcpyAsync(w.Qf, q_host, (size_t)nq * D * 4, hipMemcpyHostToDevice, st));
            if ((size_t)nq * np_f > scr.route_cap || !scr.d_route_rows) {
                for (void* p : {(void*)scr.d_route_rows, (void*)scr.d_route_d, (void*)scr.d_route_c})
                    if (p) (void)hipFree(p);
                scr.d_route_rows = nullptr; scr.d_route_d = nullptr; scr.d_route_c = nullptr; scr.route_cap = 0;
                const size_t cap = std::max<size_t>((size_t)nq * np_f, (size_t)QCHUNK * np_f);
                LY_HIP(hipMalloc(&scr.d_route_rows, cap * 8));
                LY_HIP(hipMalloc(&scr.d_route_d, cap * 4));
                LY_HIP(hipMalloc(&scr.d_route_c, (size_t)QCHUNK * 4));
                scr.route_cap = cap;
            }
            // (1) centroid ranking: the top-nprobe (score, centroid id) of the centroid matrix, single-row kernels
            SmallRows cr{h->cstore->rows, h->cstore->ld, h->nlist, LYNSE_IPFORM_SINGLE, 1, 0};
            // (2) the probed lists
            const size_t rows_b = (size_t)nq * out_k * 8, dists_b = (size_t)nq * out_k * 4;
            uint64_t* r_dst = on_device ? out_rows : reinterpret_cast<uint64_t*>(w.h_out);
            float* d_dst = on_device ? out_dists : reinterpret_cast<float*>(w.h_out + rows_b);
            uint32_t* c_dst = on_device ? out_counts : w.h_hdr;
            SmallRows sr{s->rows, s->ld, (uint64_t)std::min<uint64_t>(h->worst_rows[np_f], s->n), LYNSE_IPFORM_SINGLE, h->row_stride, h->row_offset};
            SmallIvf si{scr.d_route_rows, np_f, h->nlist, h->d_offsets, h->d_orig, (!h->ivfflat_routing && !h->no_fallback) ? 1 : 0};
            // lynse_hip_ivf_profile_get (round 6: the single-query shape reported no scan at all): HIP events around the list-scan launch, and the
            // rows it really scores — the lengths of the lists the ranking picked, read back behind the search.
            // (round 6, measured and removed: both launches as ONE kernel with a grid-wide hand-over of the probe list — 73.5 against 70.5 us;
            // kernels.h, above FinalArgs)
            hipEvent_t pe0 = nullptr, pe1 = nullptr;
            const bool timed_small = s->profiling.load();
            if (timed_small) { LY_TRY(get_event(s, 0, &pe0)); LY_TRY(get_event(s, 1, &pe1)); }
            LY_TRY(run_small(s, nq, np_f, np_f, route_metric, st, nullptr, scr.d_route_rows, scr.d_route_d, scr.d_route_c, w.overflow, d_q, &cr, nullptr));
            if (timed_small) LY_HIP(hipEventRecord(pe0, st));
            LY_TRY(run_small(s, nq, k, out_k, metric, st, nullptr, r_dst, d_dst, c_dst, w.h_hdr + QCHUNK, d_q, &sr, &si));
            if (timed_small) LY_HIP(hipEventRecord(pe1, st));
            LY_HIP(hipStreamSynchronize(st));
            if (timed_small) {
                std::vector<uint64_t> probes((size_t)nq * np_f);
                LY_HIP(hipMemcpy(probes.data(), scr.d_route_rows, probes.size() * 8, hipMemcpyDeviceToHost));
                uint64_t rows_scored = 0;
                for (uint64_t c : probes)
                    if (c < h->nlist) rows_scored += h->offsets[c + 1] - h->offsets[c];
                float ms = 0.f;
                LY_HIP(hipEventElapsedTime(&ms, pe0, pe1));
                std::lock_guard<std::mutex> plk(s->prof_mu);
                s->prof.scan_us += (double)ms * 1000.0;
                s->prof.scan_launches += 1;
                s->prof.scan_rows += rows_scored;
                s->prof.scan_bytes += rows_scored * (uint64_t)D * 4;
                s->prof.searches += 1;
                s->prof.last_plan = 32u | (2u << 8);   // bit 5: the fused few-query search (two launches: centroid ranking, probed lists; f32 rows)
            }
            bool empty_fallback = false;
            for (uint32_t i = 0; i < nq; ++i) empty_fallback |= w.h_hdr[QCHUNK + i] != 0;
            if (!empty_fallback) {
                if (!on_device) {
                    memcpy(out_rows, w.h_out, rows_b);
                    memcpy(out_dists, w.h_out + rows_b, dists_b);
                    memcpy(out_counts, w.h_hdr, nq * 4);
                }
                *overflowed = false;
                return LYNSE_OK;
            }
        }
    }
    // batches of more than 32 IP queries over a large f32 slab of whole 128-column slabs run the coarse pass on the SQ8 codes
    // (half the bytes of the f16 shadow); the exhaustive retry (safe) and subset-filtered searches stay on the f16 shadow
    const bool i8c = ivf_i8c_eligible(h, metric, nq, safe, smask != nullptr);
    if (i8c) {
        LY_TRY(ensure_i8c_codes_locked(s, metric));
        if (!i8c_codes_finite(s, metric)) i8c_strike_counter(s, metric).store(-1);
    }
    const bool i8c_on = i8c && i8c_codes_finite(s, metric);
    LY_TRY(ivf_search_chunk_staged(h, q_host, nq, k, out_k, nprobe, out_rows, out_dists, out_counts, safe, overflowed, smask, list_matches, on_device, i8c_on));
    bool retried = false;
    if (i8c_on && *overflowed) {   // margins too wide for this data: the same plan on the f16 shadow; three such strikes switch the int8 pass off
        i8c_add_strike(s, metric);
        retried = true;
        LY_TRY(ivf_search_chunk_staged(h, q_host, nq, k, out_k, nprobe, out_rows, out_dists, out_counts, safe, overflowed, smask, list_matches, on_device, false));
    }
    if (s->profiling) {   // lynse_hip_ivf_profile_get: bit 2 = the chunk was answered by the int8 pass, bit 6 = it started on it
        std::lock_guard<std::mutex> plk(s->prof_mu);
        if (safe) s->prof.last_plan &= 64u;   // (the exhaustive rerun of a chunk that overflowed: "started on int8" stays on record)
        else s->prof.last_plan = (i8c_on && !retried ? 4u : 0u) | (i8c_on ? 64u : 0u);
    }
    return LYNSE_OK;
}

static int ivf_search_chunk_staged(lynse_hip_ivf* h, const float* q_host, uint32_t nq, uint32_t k, uint32_t out_k, uint32_t nprobe,
                                   uint64_t* out_rows, float* out_dists, uint32_t* out_counts, bool safe, bool* overflowed,
                                   const uint32_t* smask, const std::vector<uint64_t>* list_matches, bool on_device, bool i8c, bool force_host,
                                   IvfAsync* as) {
    lynse_hip_flat* s = h->store;
    Workspace& w = cur(s).ws;
    hipStream_t st = cur(s).stream;
    const int metric = h->search_metric >= 0 ? h->search_metric : h->metric;
    const bool binary = h->binary;
    const int route_metric = binary ? M_L2 : metric;
    IvfScratch& scr = iscr(h);
    const uint32_t SK = i8c ? 128u : (uint32_t)HK;  // K elements per slab of the scan kernel in use
    // squared L2 / cosine on the int8 pass: inner products of augmented resp. unit vectors in the NEGATED score space
    // (I8cPrepArgs::aug / ::cosine, kernels.h) — scan and select run as IP, the exact rescoring negates, k_final negates back
    const I8cForm form = i8c_form(s, metric, 0, false);   // (nqc = 0: never the plain-code L2 form, a FLAT tiling)
    const I8cOperand opd = i8c ? i8c_operand(s, form, false) : I8cOperand{};
    const bool aug = i8c && form == I8C_L2_AUG, cosq = i8c && form == I8C_COS;
    const int key_metric = (aug || cosq) ? (int)M_IP : metric;
    const uint32_t D = h->dim, nslab = ((i8c ? opd.cols : D) + SK - 1) / SK;
    const uint32_t qpad = SCAN_BQ_LARGE;
    LY_HIP(hipMemcpyAsync(w.Qf, q_host, (size_t)nq * D * 4, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    if (binary) {
        // ---- queries: quantizer encode->decode (ivf.rs:211-222) in place, pack, +inf thresholds
        hipLaunchKernelGGL(k_bq_binarize, dim3(std::min<uint32_t>((uint32_t)(((uint64_t)nq * D + 255) / 256), 1024)), dim3(256), 0, st,
                           w.Qf, D, D, (uint64_t)nq, h->d_bq_thr, w.Qf, D);
        LY_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_pack_bits<float>, dim3((nq + 3) / 4), dim3(256), 0, st, w.Qf, D, D, nq, w.QW, s->words);
        LY_HIP(hipGetLastError());
        std::vector<float> thr0(nq, INFINITY);
        LY_HIP(hipMemcpyAsync(w.thr, thr0.data(), nq * 4, hipMemcpyHostToDevice, st));
        LY_HIP(hipMemsetAsync(w.count, 0, nq * 4, st));
        LY_HIP(hipMemsetAsync(w.overflow, 0, nq * 4, st));
        LY_HIP(hipStreamSynchronize(st));
    } else if (i8c) {
        // ---- certified int8 coarse pass (DESIGN.md §3b) over the probed lists: the SQ8 codes of the slab, the symmetric int8
        // query image, coarse score B_q + s_q * dot within E of the exact score; survivors are rescored exactly as always
        if (nq != qpad || opd.cols % 128 != 0) LY_HIP(hipMemsetAsync(w.Q16, 0, (size_t)nslab * qpad * 128, st));
        I8cPrepArgs p{};
        p.Q = w.Qf; p.D = D; p.qpad = qpad; p.nslab = nslab; p.vmax = s->vmax;
        fill_i8c_prep(p, opd, form);
        p.img = reinterpret_cast<int8_t*>(w.Q16); p.sq = w.qinv; p.bq = w.qn2; p.marg2 = w.marg2; p.thr = w.thr; p.count = w.count; p.overflow = w.overflow;
        p.gsync = w.gsync;
        hipLaunchKernelGGL(k_i8c_prep_queries, dim3(nq), dim3(256), 0, st, p);
        LY_HIP(hipGetLastError());
    } else {
        // ---- queries: device copy + prep (image layout 1, thresholds, margins)
        LY_HIP(hipMemsetAsync(w.Q16, 0, (size_t)nslab * qpad * SK * sizeof(_Float16), st));
        PrepArgs p{};
        p.Q = w.Qf; p.D = D; p.nq = nq; p.qpad = qpad; p.nslab = nslab; p.metric = metric; p.layout = 2;
        p.sv = s->sv; p.vmax = s->vmax; p.vmin = s->vmin; p.cos_degenerate = s->cos_degenerate;
        p.Q16 = w.Q16; p.qinv = w.qinv; p.qn2 = w.qn2; p.qrinv = w.qrinv; p.marg2 = w.marg2; p.thr = w.thr;
        p.count = w.count; p.overflow = w.overflow;
        hipLaunchKernelGGL(k_prep_queries, dim3(nq), dim3(256), 0, st, p);
        LY_HIP(hipGetLastError());
    }

    // ---- routing
    const uint32_t np_eff = std::min<uint32_t>(nprobe, h->nlist);
    const uint32_t tile_rows = binary ? 2048u : (uint32_t)SCAN_BR;
    // Device-side grouping (k_ivf_group): the probes stay in device memory, pairs / groups / tile lists are built by one
    // workgroup, the scan launches read their tile counts from device memory — no copy of the probes to the host, no host
    // loop, no uploads.  Float searches of one pass whose pairs fit one workgroup's LDS; the all-lists-empty fallback of
    // IVFIndex is flagged by the kernel and redone on the host path.  (LYNSE_HIP_IVF_DEVICE_GROUPING=0: host path, A/B.)
    const int dg_env = ivf_device_grouping();
    const uint32_t pass_lists = std::max<uint32_t>(1, w.cap / 16);
    const uint64_t win_bound = (uint64_t)nq * (h->worst_rows[std::min<uint32_t>(np_eff, h->nlist)] / tile_rows + 2ull * np_eff) + 16;
    const bool dev_group = dg_env && !force_host && !binary && !smask && !list_matches && !safe && np_eff < h->nlist && np_eff <= pass_lists &&
                           (uint64_t)nq * np_eff <= IVF_GROUP_MAX_PAIRS && h->nlist <= IVF_GROUP_MAX_LISTS && win_bound * 3 * sizeof(IvfTile) <= (512ull << 20);
    if (as && !dev_group) return set_error(LYNSE_ERR_INTERNAL, "a search in flight needs the device-side grouping");   // (ivf_async_shape_ok said yes)
    std::vector<uint32_t> probes;
    if (!dev_group) LY_TRY(ivf_route(h, nq, np_eff, metric, route_metric, st, &probes));

    // ---- group (query, list) pairs by list; IVFIndex falls back to ALL rows when every probed list
    // is empty (ivf.rs:258-265) — IvfFlatMmap returns nothing (ivf_flat_mmap.rs:278-280)
    // (list, query) pairs, grouped by list with a counting sort (queries stay in ascending order inside a list)
    // A query's lists are scanned in PASSES of at most cap / 16 lists: the first position window of a pass emits every
    // row it covers while the threshold is still open (pass 0) — a0 >= 8 rows per list must fit cap / 2 keys.  Later
    // passes start from the threshold the earlier ones left behind.  (nprobe <= 1024 with the default cap: one pass.)
    std::vector<uint32_t> all_list, all_q, all_pass;  // pairs in query order
    all_list.reserve((size_t)nq * np_eff);
    all_q.reserve((size_t)nq * np_eff);
    all_pass.reserve((size_t)nq * np_eff);
    uint32_t n_pass = 1;
    uint32_t lists_per_pass = std::min<uint32_t>(np_eff, pass_lists);   // most lists one query scans in one pass (the all-lists fallback of IVFIndex: up to nlist)
    for (uint32_t q = 0; q < (dev_group ? 0u : nq); ++q) {
        uint64_t total = 0;
        for (uint32_t r = 0; r < np_eff; ++r) {
            const uint32_t c = probes[(size_t)q * np_eff + r];
            if (c < h->nlist) total += list_matches ? (*list_matches)[c] : h->offsets[c + 1] - h->offsets[c];
        }
        uint32_t rank = 0;
        auto add = [&](uint32_t c) {
            all_list.push_back(c); all_q.push_back(q); all_pass.push_back(rank / pass_lists);
            n_pass = std::max(n_pass, rank / pass_lists + 1);
            ++rank;
        };
        if (total == 0 && !h->ivfflat_routing && !h->no_fallback) {
            for (uint32_t c = 0; c < h->nlist; ++c) add(c);
            lists_per_pass = std::max(lists_per_pass, std::min<uint32_t>(h->nlist, pass_lists));
        } else {
            for (uint32_t r = 0; r < np_eff; ++r) {
                const uint32_t c = probes[(size_t)q * np_eff + r];
                if (c < h->nlist && h->offsets[c + 1] > h->offsets[c]) add(c);
            }
        }
    }
    FinalArgs fa{};
    fa.cand = w.cand; fa.count = w.count; fa.k = k; fa.out_k = out_k; fa.cap = w.cap; fa.metric = key_metric;
    fa.neg_metric1 = (aug || cosq) ? metric + 1 : 0;
    fa.ip_form = LYNSE_IPFORM_SINGLE;  // IVF scores with compute_distance_f32 (ivf.rs:294-298): single-row kernels
    fa.exact = binary ? 1 : 0; fa.Qf = w.Qf; fa.V = s->rows; fa.ld = s->ld; fa.D = D;
    fa.row_stride = h->row_stride; fa.row_offset = h->row_offset;
    fa.orig_ids = binary ? nullptr : h->d_orig;  // the packed scan already emits original rows
    fa.out_rows = w.out_rows; fa.out_dists = w.out_dists; fa.out_counts = w.out_counts; fa.pool_total = nullptr;
    LY_TRY(ensure_lds<k_select<SEL_NT>>(SEL_LDS_MAX));
    LY_TRY(ensure_lds<k_final<SEL_NT>>(SEL_LDS_MAX));
    // one position window: the tiled scan of its tile list (count on the host, or in device memory: ntiles_dev) + the select
    // lynse_hip_ivf_profile_get: HIP events around the tiled scan launches of the blocking searches (scan_us / scan_launches), the
    // rows their tiles cover (scan_rows: a list probed by several 32-query groups is streamed once per group)
    const bool timed = s->profiling && !as;
    std::vector<size_t> scan_ev;
    uint64_t host_tile_rows = 0;
    size_t ev_next = 0;
    auto run_window = [&](const IvfTile* d_win_tiles, uint32_t ntiles_host, const uint32_t* ntiles_dev) -> int {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (timed) {
            LY_TRY(get_event(s, ev_next, &e0)); LY_TRY(get_event(s, ev_next + 1, &e1));
            scan_ev.push_back(ev_next);
            ev_next += 2;
            LY_HIP(hipEventRecord(e0, st));
        }
        if (binary) {
            BinTileArgs b{};
            b.P = s->packed; b.W = s->words; b.QW = w.QW; b.tiles = d_win_tiles; b.ntiles = ntiles_host;
            b.pair_q = scr.d_pair_q; b.orig = h->d_orig; b.mask = smask; b.thr = w.thr; b.cand = w.cand; b.count = w.count; b.cap = w.cap;
            const uint32_t grid = std::min<uint32_t>(b.ntiles, (uint32_t)s->num_cu * 8);
            const size_t lds = (size_t)32 * s->words * 8 + 256;
            switch (metric) {
            case M_HAMMING: hipLaunchKernelGGL(k_scan_binary_tiled<0>, dim3(grid), dim3(256), lds, st, b); break;
            case M_DICE: hipLaunchKernelGGL(k_scan_binary_tiled<2>, dim3(grid), dim3(256), lds, st, b); break;
            default: hipLaunchKernelGGL(k_scan_binary_tiled<1>, dim3(grid), dim3(256), lds, st, b); break;
            }
            LY_HIP(hipGetLastError());
        } else {
        ScanArgs a{};
        a.V = s->rows; a.ld = s->ld; a.V16 = s->rows16; a.ld16 = s->ld16; a.D = D; a.row0 = 0; a.row1 = (uint32_t)s->n; a.Q16 = scr.d_gimg; a.qpad = 32;
        a.nq = nq; a.nslab = nslab; a.ntiles = ntiles_host; a.qinv = w.qinv; a.qn2 = w.qn2; a.qrinv = w.qrinv;
        a.thr = w.thr; a.vn2 = s->vn2; a.vrinv = s->vrinv; a.sv = s->sv; a.vmax2 = s->vmax * s->vmax; a.cand = w.cand; a.count = w.count; a.cap = w.cap;
        a.emit_all = 0; a.debug_flags = 0; a.tiles = d_win_tiles; a.ntiles_dev = ntiles_dev; a.pair_q = scr.d_pair_q; a.mask = smask;
        const uint32_t grid = ntiles_dev ? (uint32_t)s->num_cu * 2 : std::min<uint32_t>(a.ntiles, (uint32_t)s->num_cu * 2);
        if (i8c) {
            a.V16 = reinterpret_cast<const _Float16*>(opd.codes); a.ld16 = opd.ld;
            LY_TRY((launch_h16<with(I8C_SMALL, &H16Cfg::tiled, true)>(grid, st, a)));
        } else
        LY_TRY(launch_scan_tiled(a, metric, grid, st));
        }
        if (timed) LY_HIP(hipEventRecord(e1, st));
        SelectArgs sa{};
        sa.cand = w.cand; sa.count = w.count; sa.overflow = w.overflow; sa.thr = w.thr; sa.marg2 = w.marg2;
        sa.k = k; sa.cap = w.cap; sa.keep_max = w.cap / 2; sa.metric = key_metric; sa.ip_form = LYNSE_IPFORM_SINGLE;
        sa.neg_metric1 = (aug || cosq) ? metric + 1 : 0;
        sa.exact = binary ? 1 : 0; sa.tighten = binary ? 0 : 1; sa.emit_all_n = -1; sa.keep_ties = 1; sa.Qf = w.Qf; sa.V = s->rows; sa.ld = s->ld; sa.D = D;
        sa.lds_bytes = sel_lds_bytes(w.cap, nq);
        hipLaunchKernelGGL(k_select<SEL_NT>, dim3(nq), dim3(SEL_NT), sa.lds_bytes, st, sa);
        LY_HIP(hipGetLastError());
        return LYNSE_OK;
    };
    const uint32_t gimg_halves = nslab * 32 * 64;  // one group image: 32 lines of 128 B per slab (64 halves / 128 int8 codes)
    // ---- position windows inside every probed list: [0,a0) [a0,16*a0) [16*a0, end)
    // (the first window of a pass emits every row it covers: a0 rows of EVERY list a query scans in that pass must fit cap / 2 keys — a
    // query on the all-lists fallback scans up to cap / 16 lists per pass, not nprobe: 64 x 302 lists overflowed every plan)
    const uint32_t a0 = std::max<uint32_t>(8, std::min<uint32_t>(64, w.cap / 2 / std::max<uint32_t>(lists_per_pass, 1)));
    if (dev_group) {
        const uint64_t* p64 = nullptr;
        const uint32_t* p32 = nullptr;
        LY_TRY(ivf_route(h, nq, np_eff, metric, route_metric, st, &probes, &p64, &p32, as));
        const size_t P = (size_t)nq * np_eff;
        const size_t gmax = std::min<size_t>(P, (size_t)h->nlist + P / 32 + 1);
        if ((uint64_t)gmax * gimg_halves > 0xffffffffull) return set_error(LYNSE_ERR_UNSUPPORTED, "too many (list, query-group) pairs in one batch");
        LY_TRY(ivf_grow(&scr.d_pair_q, &scr.pairs_cap, P));
        LY_TRY(ivf_grow(&scr.d_groups, &scr.groups_cap, gmax));
        LY_TRY(ivf_grow(&scr.d_tbase, &scr.tbase_cap, gmax * 3));
        LY_TRY(ivf_grow(&scr.d_prank, &scr.prank_cap, P));
        LY_TRY(ivf_grow(&scr.d_gimg, &scr.gimg_cap, gmax * (size_t)gimg_halves));
        LY_TRY(ivf_grow(&scr.d_tiles, &scr.tiles_cap, (size_t)win_bound * 3));
        if (!scr.d_ghdr) {
            LY_HIP(hipMalloc(&scr.d_ghdr, 8 * 4));
            LY_HIP(hipHostMalloc(&scr.h_ghdr, 8 * 4, hipHostMallocDefault));
        }
        IvfGroupArgs ga{};
        ga.probes64 = p64; ga.probes32 = p32; ga.nq = nq; ga.np = np_eff; ga.nlist = h->nlist; ga.offsets = h->d_offsets; ga.gimg_halves = gimg_halves;
        ga.a0 = a0; ga.tile_rows = tile_rows; ga.win_cap = (uint32_t)win_bound; ga.flag_empty = (!h->ivfflat_routing && !h->no_fallback) ? 1u : 0u;
        ga.pair_q = scr.d_pair_q; ga.groups = scr.d_groups; ga.tiles = scr.d_tiles; ga.hdr = scr.d_ghdr; ga.tbase = scr.d_tbase; ga.gmax = (uint32_t)gmax; ga.prank = scr.d_prank;
        const size_t glds = ((size_t)h->nlist * 2 + std::max<size_t>(h->nlist, P) + 16 + 256) * 4;
        LY_TRY(ensure_lds<k_ivf_group<1024>>(((size_t)IVF_GROUP_MAX_LISTS * 2 + IVF_GROUP_MAX_PAIRS + 16 + 256) * 4 + 64));
        hipLaunchKernelGGL(k_ivf_group<1024>, dim3(1), dim3(1024), glds, st, ga);
        hipLaunchKernelGGL(k_ivf_emit_tiles, dim3(64), dim3(256), 0, st, ga);
        hipLaunchKernelGGL(k_ivf_gather_groups, dim3((uint32_t)s->num_cu * 8), dim3(256), 0, st, w.Q16, qpad, scr.d_gimg, scr.d_groups, scr.d_pair_q,
                           scr.d_ghdr, nslab);
        LY_HIP(hipGetLastError());
        LY_HIP(hipMemcpyAsync(scr.h_ghdr, scr.d_ghdr, 8 * 4, hipMemcpyDeviceToHost, st));   // (read behind the final synchronise)
        const uint64_t longest = h->worst_rows[1];   // the longest list of the index
        for (int wi = 0; wi < 3; ++wi) {
            if (wi == 1 && longest <= a0) break;
            if (wi == 2 && longest <= (uint64_t)a0 * 16) break;
            LY_TRY(run_window(scr.d_tiles + (size_t)wi * win_bound, (uint32_t)win_bound, scr.d_ghdr + 1 + wi));
        }
    }
    // (host path) the pair / tile lists are the SOURCE of asynchronous copies: they live until the final synchronise of the call
    // (a large pageable source is pinned and copied by DMA — freeing it at the end of the pass would race with that copy)
    std::vector<uint32_t> pair_q;
    std::vector<GatherPair> gpairs;
    std::vector<IvfTile> all_tiles;
    for (uint32_t pass = 0; pass < (dev_group ? 0u : n_pass); ++pass) {
    std::vector<uint32_t> pl_list, pl_q;  // the pairs of this pass, in query order
    if (n_pass == 1) { pl_list.swap(all_list); pl_q.swap(all_q); }
    else {
        for (size_t i = 0; i < all_list.size(); ++i)
            if (all_pass[i] == pass) { pl_list.push_back(all_list[i]); pl_q.push_back(all_q[i]); }
    }
    std::vector<uint32_t> lstart(h->nlist + 1, 0);
    for (uint32_t c : pl_list) lstart[c + 1] += 1;
    for (uint32_t c = 0; c < h->nlist; ++c) lstart[c + 1] += lstart[c];
    std::vector<uint32_t> sorted_q(pl_q.size());
    {
        std::vector<uint32_t> wp(lstart.begin(), lstart.end() - 1);
        for (size_t i = 0; i < pl_q.size(); ++i) sorted_q[wp[pl_list[i]]++] = pl_q[i];
    }
    struct Group { uint32_t list, pair0, nq, qimg_off; };
    std::vector<Group> groups;
    pair_q.clear();
    gpairs.clear();
    pair_q.reserve(sorted_q.size());
    gpairs.reserve(sorted_q.size());
    uint64_t max_len = 0;
    for (uint32_t c = 0; c < h->nlist; ++c) {
        const uint32_t q0 = lstart[c], q1 = lstart[c + 1];
        for (uint32_t b = q0; b < q1; b += 32) {
            const uint32_t m = std::min<uint32_t>(32, q1 - b);
            Group g{c, (uint32_t)pair_q.size(), m, (uint32_t)(groups.size() * (size_t)gimg_halves)};
            for (uint32_t i = 0; i < m; ++i) {
                pair_q.push_back(sorted_q[b + i]);
                gpairs.push_back({sorted_q[b + i], g.qimg_off, i});
            }
            groups.push_back(g);
            max_len = std::max<uint64_t>(max_len, h->offsets[c + 1] - h->offsets[c]);
        }
    }
    if (!groups.empty()) {
        if ((uint64_t)groups.size() * gimg_halves > 0xffffffffull)
            return set_error(LYNSE_ERR_UNSUPPORTED, "too many (list, query-group) pairs in one batch");
        LY_TRY(ivf_grow(&scr.d_pair_q, &scr.pairs_cap, pair_q.size()));
        LY_HIP(hipMemcpyAsync(scr.d_pair_q, pair_q.data(), pair_q.size() * 4, hipMemcpyHostToDevice, st));
        if (!binary) {
            LY_TRY(ivf_grow(&scr.d_pairs, &scr.gpairs_cap, gpairs.size()));
            LY_TRY(ivf_grow(&scr.d_gimg, &scr.gimg_cap, groups.size() * (size_t)gimg_halves));
            LY_HIP(hipMemcpyAsync(scr.d_pairs, gpairs.data(), gpairs.size() * sizeof(GatherPair), hipMemcpyHostToDevice, st));
            LY_HIP(hipMemsetAsync(scr.d_gimg, 0, groups.size() * (size_t)gimg_halves * 2, st));
            const uint32_t slots = i8c ? 8u : SK / 8;   // 16-B slots per line
            const uint64_t gt = (uint64_t)gpairs.size() * nslab * slots;
            hipLaunchKernelGGL(k_ivf_gather_q, dim3((uint32_t)std::min<uint64_t>((gt + 255) / 256, 65535)), dim3(256), 0, st, w.Q16,
                               qpad, scr.d_gimg, scr.d_pairs, (uint32_t)gpairs.size(), nslab, slots);
            LY_HIP(hipGetLastError());
        }

        std::vector<std::pair<uint64_t, uint64_t>> windows;
        if (safe) {
            for (uint64_t b = 0; b < max_len; b += a0) windows.push_back({b, b + a0});
        } else {
            windows.push_back({0, a0});
            if (max_len > a0) windows.push_back({a0, (uint64_t)a0 * 16});
            if (max_len > (uint64_t)a0 * 16) windows.push_back({(uint64_t)a0 * 16, max_len});
        }
        // the tile lists of ALL windows go up in one copy (no host round trip between the windows)
        all_tiles.clear();
        std::vector<std::pair<size_t, size_t>> win_range;  // [first, count) in all_tiles
        for (auto& win : windows) {
            const size_t first = all_tiles.size();
            for (auto& g : groups) {
                const uint64_t b = h->offsets[g.list], len = h->offsets[g.list + 1] - b;
                const uint64_t lo = std::min(win.first, len), hi = std::min(win.second, len);
                for (uint64_t r = lo; r < hi; r += tile_rows)
                    all_tiles.push_back({(uint32_t)(b + r), (uint32_t)std::min<uint64_t>(tile_rows, hi - r), g.qimg_off, g.pair0, g.nq});
            }
            win_range.push_back({first, all_tiles.size() - first});
        }
        if (timed) for (auto& tl : all_tiles) host_tile_rows += tl.nrows;
        if (!all_tiles.empty()) {
            LY_TRY(ivf_grow(&scr.d_tiles, &scr.tiles_cap, all_tiles.size()));
            LY_HIP(hipMemcpyAsync(scr.d_tiles, all_tiles.data(), all_tiles.size() * sizeof(IvfTile), hipMemcpyHostToDevice, st));
        }
        for (auto& wr : win_range) {
            if (wr.second == 0) continue;
            const IvfTile* d_win_tiles = scr.d_tiles + wr.first;
            struct { size_t n; size_t size() const { return n; } } tiles{wr.second};
            LY_TRY(run_window(d_win_tiles, (uint32_t)tiles.size(), nullptr));
        }
    }
    if (n_pass > 1) LY_HIP(hipStreamSynchronize(st));  // the pass's host-side tile / pair lists are about to be rebuilt
    }  // passes
    if (!fa.exact) {  // spread the exact rescoring over the chip (pools are large on clustered data), then only sort
        hipLaunchKernelGGL(k_rescore_pool<256>, dim3(nq, nq >= 64 ? 4 : 32), dim3(256), 0, st, fa);
        LY_HIP(hipGetLastError());
        fa.exact = 1;
    }
    if (as && as->status) fa.any_overflow = as->status;
    // k_final writes the results where they belong — the caller's device arrays, or the pinned (device-visible) staging buffer of small
    // host-API results — and counts + overflow flags straight into the pinned header of the context: no copy kernels behind the search
    // (they were four 5-us launches of a 1 ms C4 batch); only large host results go through the workspace and two device-to-host copies
    const size_t rows_b = (size_t)nq * out_k * 8, dists_b = (size_t)nq * out_k * 4;
    const bool staged = !on_device && rows_b + dists_b <= H_OUT_BYTES;
    if (on_device) { fa.out_rows = out_rows; fa.out_dists = out_dists; fa.out_counts = out_counts; }
    else if (staged) { fa.out_rows = reinterpret_cast<uint64_t*>(w.h_out); fa.out_dists = reinterpret_cast<float*>(w.h_out + rows_b); }
    fa.overflow = w.overflow; fa.h_hdr = w.h_hdr; fa.hdr_q = QCHUNK;
    fa.lds_bytes = sel_lds_bytes(w.cap, nq);
    hipLaunchKernelGGL(k_final<SEL_NT>, dim3(nq), dim3(SEL_NT), fa.lds_bytes, st, fa);
    LY_HIP(hipGetLastError());
    if (!on_device && !staged) {
        LY_HIP(hipMemcpyAsync(out_rows, w.out_rows, rows_b, hipMemcpyDeviceToHost, st));
        LY_HIP(hipMemcpyAsync(out_dists, w.out_dists, dists_b, hipMemcpyDeviceToHost, st));
    }
    if (as) {   // in flight: wait() reads the pinned headers (w.h_hdr, scr.h_ghdr, the centroid store's) behind the ticket's event
        if (as->status) {
            hipLaunchKernelGGL(k_or_word, dim3(1), dim3(1), 0, st, as->status, (const uint32_t*)(scr.d_ghdr + 4));
            LY_HIP(hipGetLastError());
        }
        return LYNSE_OK;
    }
    LY_HIP(hipStreamSynchronize(st));
    if (timed) {
        std::lock_guard<std::mutex> plk(s->prof_mu);
        for (size_t e : scan_ev) {
            float ms = 0.f;
            LY_HIP(hipEventElapsedTime(&ms, cur(s).ev_pool[e], cur(s).ev_pool[e + 1]));
            s->prof.scan_us += (double)ms * 1000.0;
            s->prof.scan_launches += 1;
        }
        const uint64_t rows_scanned = dev_group ? (uint64_t)scr.h_ghdr[6] : host_tile_rows;
        s->prof.scan_rows += rows_scanned;
        s->prof.scan_bytes += rows_scanned * (uint64_t)D * 4;
        s->prof.searches += 1;
    }
    if (dev_group && scr.h_ghdr[4] != 0)   // a query whose probed lists are all empty (IVFIndex scans every list then): the host path
        return ivf_search_chunk_staged(h, q_host, nq, k, out_k, nprobe, out_rows, out_dists, out_counts, safe, overflowed, smask, list_matches, on_device, i8c, true);
    if (staged) { memcpy(out_rows, w.h_out, rows_b); memcpy(out_dists, w.h_out + rows_b, dists_b); }
    if (!on_device) memcpy(out_counts, w.h_hdr, nq * 4);
    *overflowed = false;
    for (uint32_t i = 0; i < nq; ++i) *overflowed |= w.h_hdr[QCHUNK + i] != 0;
    return LYNSE_OK;
}

// IVF search with k > cap / 4 (IVFIndex::search, ivf.rs:181-348, takes any k): per query the probed lists' rows — or ALL rows
// when every probed list is empty and the index is an IVFIndex (:258-265) — are scored exactly on the device
// (k_ivf_score_positions) and the host keeps the k best (score, original row) keys: the canonical order.  One query at a
// time: a rare shape, not a tuned one.  Called with the store's lock held, statistics final, a workspace present.
static int ivf_search_large_k(lynse_hip_ivf* h, const float* queries, uint64_t nq, uint32_t k, uint32_t kk, uint32_t nprobe,
                              uint64_t* out_rows, float* out_dists, uint32_t* out_counts, bool on_device, const std::vector<bool>* allowed = nullptr) {
    lynse_hip_flat* s = h->store;
    Workspace& w = cur(s).ws;
    hipStream_t st = cur(s).stream;
    const int metric = h->search_metric >= 0 ? h->search_metric : h->metric;
    const bool asc = metric_ascending(metric);
    const uint32_t D = h->dim, np_eff = std::min<uint32_t>(nprobe, h->nlist);
    uint32_t* d_pos = nullptr;
    uint64_t* d_keys = nullptr;
    size_t cap_pos = 0;
    struct G { uint32_t** a; uint64_t** b; ~G() { if (*a) (void)hipFree(*a); if (*b) (void)hipFree(*b); } } guard{&d_pos, &d_keys};
    std::vector<uint64_t> o_rows(on_device ? (size_t)nq * k : 0);
    std::vector<float> o_dists(on_device ? (size_t)nq * k : 0);
    std::vector<uint32_t> o_counts(on_device ? nq : 0);
    uint64_t* res_rows = on_device ? o_rows.data() : out_rows;
    float* res_dists = on_device ? o_dists.data() : out_dists;
    uint32_t* res_counts = on_device ? o_counts.data() : out_counts;
    std::vector<uint32_t> pos, probes;
    std::vector<uint64_t> keys;
    const bool binary = h->binary;
    if (binary) LY_TRY(ensure_packed_locked(s));
    for (uint64_t q = 0; q < nq; ++q) {
        LY_HIP(hipMemcpyAsync(w.Qf, queries + q * D, (size_t)D * 4, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
        if (binary) {  // the query goes through the quantizer (ivf.rs:211-222), then routing is L2 on the codes
            hipLaunchKernelGGL(k_bq_binarize, dim3(std::min<uint32_t>((D + 255) / 256, 1024u)), dim3(256), 0, st, w.Qf, D, D, (uint64_t)1, h->d_bq_thr, w.Qf, D);
            hipLaunchKernelGGL(k_pack_bits<float>, dim3(1), dim3(256), 0, st, w.Qf, D, D, 1u, w.QW, s->words);
            LY_HIP(hipGetLastError());
        }
        LY_TRY(ivf_route(h, 1, np_eff, metric, binary ? (int)M_L2 : metric, st, &probes));
        pos.clear();
        for (uint32_t r = 0; r < np_eff; ++r) {
            const uint32_t c = probes[r];
            if (c >= h->nlist) continue;
            for (uint64_t p = h->offsets[c]; p < h->offsets[c + 1]; ++p)
                if (!allowed || (*allowed)[h->orig[p]]) pos.push_back((uint32_t)p);
        }
        if (pos.empty() && !h->ivfflat_routing && !h->no_fallback) {   // ivf.rs:258-265: nothing in the probed lists -> every (subset) row
            for (uint64_t p = 0; p < s->n; ++p)
                if (!allowed || (*allowed)[h->orig[p]]) pos.push_back((uint32_t)p);
        }
        const uint32_t P = (uint32_t)pos.size();
        if (P) {
            if (P > cap_pos) {
                if (d_pos) (void)hipFree(d_pos);
                if (d_keys) (void)hipFree(d_keys);
                d_pos = nullptr; d_keys = nullptr;
                cap_pos = std::max<size_t>(P, cap_pos * 2);
                LY_HIP(hipMalloc(&d_pos, cap_pos * 4));
                LY_HIP(hipMalloc(&d_keys, cap_pos * 8));
            }
            LY_HIP(hipMemcpyAsync(d_pos, pos.data(), (size_t)P * 4, hipMemcpyHostToDevice, st));
            if (binary) {
                IvfScorePackedArgs a{s->packed, s->words, w.QW, d_pos, h->d_orig, P, metric == M_HAMMING ? 0 : (metric == M_DICE ? 2 : 1), d_keys};
                hipLaunchKernelGGL(k_ivf_score_positions_packed, dim3(std::min<uint32_t>((P + 31) / 32, (uint32_t)s->num_cu * 8)), dim3(256), 0, st, a);
            } else {
                IvfScoreArgs a{s->rows, s->ld, D, w.Qf, d_pos, h->d_orig, P, metric, d_keys};
                hipLaunchKernelGGL(k_ivf_score_positions, dim3(std::min<uint32_t>((P + 31) / 32, (uint32_t)s->num_cu * 8)), dim3(256), 0, st, a);
            }
            LY_HIP(hipGetLastError());
            keys.resize(P);
            LY_HIP(hipMemcpyAsync(keys.data(), d_keys, (size_t)P * 8, hipMemcpyDeviceToHost, st));
            LY_HIP(hipStreamSynchronize(st));
        }
        res_counts[q] = select_pool_keys(keys.data(), P, kk, k, asc, res_rows + q * k, res_dists + q * k, h->row_stride, h->row_offset);
    }
    if (on_device) {
        LY_TRY(h2d_done(out_rows, o_rows.data(), o_rows.size() * 8));
        LY_TRY(h2d_done(out_dists, o_dists.data(), o_dists.size() * 4));
        LY_TRY(h2d_done(out_counts, o_counts.data(), o_counts.size() * 4));
    }
    return LYNSE_OK;
}

static int ivf_search_locked(lynse_hip_ivf* h, const float* queries, uint64_t nq, uint32_t k, uint32_t nprobe,
                             uint64_t* out_rows, float* out_dists, uint32_t* out_counts, bool filtered,
                             const uint64_t* subset, uint64_t n_subset, int metric_override, bool on_device);
static int ivf_search_sq8(lynse_hip_ivf* h, const float* queries, uint64_t nq, uint32_t k, uint32_t nprobe,
                          uint64_t* out_rows, float* out_dists, uint32_t* out_counts, bool filtered,
                          const uint64_t* subset, uint64_t n_subset, bool on_device);
static int spann_search(lynse_hip_ivf* h, const float* queries, uint64_t nq, uint32_t k, uint32_t nprobe,
                        uint64_t* out_rows, float* out_dists, uint32_t* out_counts, bool filtered, const uint64_t* subset, uint64_t n_subset);

static int ivf_search_impl(lynse_hip_ivf* h, const float* queries, uint64_t nq, uint32_t k, uint32_t nprobe,
                           uint64_t* out_rows, float* out_dists, uint32_t* out_counts, bool filtered,
                           const uint64_t* subset, uint64_t n_subset, int metric_override = -1, bool on_device = false) {
    if (!h) return set_error(LYNSE_ERR_INDEX_NOT_BUILT, "IVF index is not built");  // ivf.rs:187-189
    if (nq == 0) return LYNSE_OK;
    if (!queries || !out_counts || (k && (!out_rows || !out_dists))) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    if (filtered && n_subset && !subset) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "subset is NULL");
    const std::shared_ptr<std::mutex> guard = ivf_guard_of(h);
    std::lock_guard<std::mutex> glk(*guard);   // (insert / delete replace h->store: read it under the index guard)
    if (!h->store) return set_error(LYNSE_ERR_INDEX_NOT_BUILT, "IVF index is not built");
    if (h->spann) {
        if (metric_override >= 0) return set_error(LYNSE_ERR_UNSUPPORTED, "a SPANN index searches with the metric it was built for");
        if (on_device) return set_error(LYNSE_ERR_UNSUPPORTED, "device-resident search is not defined for a SPANN index");
        return spann_search(h, queries, nq, k, nprobe, out_rows, out_dists, out_counts, filtered, subset, n_subset);
    }
    if (h->sq8) {
        if (metric_override >= 0) return set_error(LYNSE_ERR_UNSUPPORTED, "an IVF-*-SQ8 index searches with the metric it was built for");
        return ivf_search_sq8(h, queries, nq, k, nprobe, out_rows, out_dists, out_counts, filtered, subset, n_subset, on_device);
    }
    return ivf_search_locked(h, queries, nq, k, nprobe, out_rows, out_dists, out_counts, filtered, subset, n_subset, metric_override, on_device);
}

// the search itself, the index guard held
static int ivf_search_locked(lynse_hip_ivf* h, const float* queries, uint64_t nq, uint32_t k, uint32_t nprobe,
                             uint64_t* out_rows, float* out_dists, uint32_t* out_counts, bool filtered,
                             const uint64_t* subset, uint64_t n_subset, int metric_override, bool on_device) {
    lynse_hip_flat* s = h->store;
    std::unique_lock<std::shared_mutex> lk(s->rw);
    struct MetricScope {  // the metric of THIS call (lynse_hip_ivf_search_metric_f32), visible to ivf_search_chunk under the lock
        lynse_hip_ivf* h;
        MetricScope(lynse_hip_ivf* hh, int m) : h(hh) { h->search_metric = m; }
        ~MetricScope() { h->search_metric = -1; }
    } metric_scope(h, metric_override);
    LY_TRY(use_device(s));
    if (s->n == 0 || k == 0) {
        if (on_device) LY_TRY(memset_done(out_counts, 0, nq * 4));
        else memset(out_counts, 0, nq * 4);
        return LYNSE_OK;
    }
    if (nprobe == 0) nprobe = 1;  // ivf.rs:192-196 / ivf_flat_mmap.rs:236
    const uint32_t kk = (uint32_t)std::min<uint64_t>(k, s->n);
    if (kk > s->cap / 4 || (h->binary && s->words > 16u * BIN_MAX_CHUNKS)) {
        // k beyond the candidate capacity of the staged pipeline — or packed rows wider than the 4096 bits the tiled popcount
        // kernel keeps in registers: every row of the probed lists scored exactly, host top-k
        std::vector<bool> allowed;   // SearchParams.subset by original row (ivf.rs:251-256)
        if (filtered) {
            allowed.assign(s->n, false);
            uint64_t valid = 0;
            for (uint64_t i = 0; i < n_subset; ++i)
                if (subset[i] < s->n && !allowed[subset[i]]) { allowed[subset[i]] = true; ++valid; }
            if (valid == 0) { memset(out_counts, 0, nq * 4); return LYNSE_OK; }  // ivf.rs:267-269
        }
        LY_TRY(finalize_locked(s)); LY_TRY(ensure_shadow_locked(s));   // (the slab scans read the f16 shadow unless a batch takes the int8 pass; built once)
        LY_TRY(ensure_workspace(s, 1));
        return ivf_search_large_k(h, queries, nq, k, kk, nprobe, out_rows, out_dists, out_counts, on_device, filtered ? &allowed : nullptr);
    }
    LY_TRY(finalize_locked(s)); LY_TRY(ensure_shadow_locked(s));   // (the slab scans read the f16 shadow unless a batch takes the int8 pass; built once)
    LY_TRY(ensure_workspace(s, k));
    const uint32_t* smask = nullptr;
    std::vector<uint64_t> list_matches;
    if (filtered) {  // subset (original row ids) -> matches per list (host) + slab-position bitmask (device)
        list_matches.assign(h->nlist, 0);
        const uint64_t n_rows = h->spann ? h->n_rows : s->n;
        std::vector<bool> seen(n_rows, false);
        uint64_t valid = 0;
        for (uint64_t i = 0; i < n_subset; ++i) {
            const uint64_t r = subset[i];
            if (r < n_rows && !seen[r]) { seen[r] = true; if (!h->spann) list_matches[h->assignments[r]] += 1; ++valid; }
        }
        if (valid == 0) { memset(out_counts, 0, nq * 4); return LYNSE_OK; }  // ivf.rs:267-269
        if (h->spann)   // (a row counts in every list it sits in)
            for (uint32_t c = 0; c < h->nlist; ++c)
                for (uint64_t p = h->offsets[c]; p < h->offsets[c + 1]; ++p) list_matches[c] += seen[h->orig[p]] ? 1 : 0;
        const uint64_t words = (s->n + 31) / 32 + 8;
        auto& fc = cur(s);   // (the slab store's context 0: IVF searches hold its exclusive lock)
        if (words > fc.mask_words) {
            if (fc.d_mask) (void)hipFree(fc.d_mask);
            fc.d_mask = nullptr;
            LY_HIP(hipMalloc(&fc.d_mask, words * 4));
            fc.mask_words = words;
        }
        if (words > h->smask_words) {
            if (h->d_smask) (void)hipFree(h->d_smask);
            h->d_smask = nullptr;
            LY_HIP(hipMalloc(&h->d_smask, words * 4));
            h->smask_words = words;
        }
        if (n_subset > fc.subset_cap) {
            if (fc.d_subset) (void)hipFree(fc.d_subset);
            fc.d_subset = nullptr;
            LY_HIP(hipMalloc(&fc.d_subset, n_subset * 8));
            fc.subset_cap = n_subset;
        }
        hipStream_t st = cur(s).stream;
        LY_HIP(hipMemsetAsync(fc.d_mask, 0, words * 4, st));
        LY_HIP(hipMemsetAsync(h->d_smask, 0, words * 4, st));
        LY_HIP(hipMemcpyAsync(fc.d_subset, subset, n_subset * 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_mask_build, dim3((uint32_t)std::min<uint64_t>((n_subset + 255) / 256, (uint64_t)s->num_cu * 8)), dim3(256), 0, st,
                           fc.d_subset, n_subset, s->n, fc.d_mask);
        hipLaunchKernelGGL(k_mask_permute, dim3((uint32_t)std::min<uint64_t>((s->n + 255) / 256, (uint64_t)s->num_cu * 8)), dim3(256), 0, st,
                           fc.d_mask, h->d_orig, s->n, h->d_smask);
        LY_HIP(hipGetLastError());
        LY_HIP(hipStreamSynchronize(st));
        smask = h->d_smask;
    }
    for (uint64_t q0 = 0; q0 < nq; q0 += QCHUNK) {
        const uint32_t nqc = (uint32_t)std::min<uint64_t>(QCHUNK, nq - q0);
        bool ovf = false;
        LY_TRY(ivf_search_chunk(h, queries + q0 * h->dim, nqc, kk, k, nprobe, out_rows + q0 * k, out_dists + q0 * k,
                                out_counts + q0, false, &ovf, smask, filtered ? &list_matches : nullptr, on_device));
        if (ovf) {
            LY_TRY(ivf_search_chunk(h, queries + q0 * h->dim, nqc, kk, k, nprobe, out_rows + q0 * k, out_dists + q0 * k,
                                    out_counts + q0, true, &ovf, smask, filtered ? &list_matches : nullptr, on_device));
            if (ovf) return set_error(LYNSE_ERR_INTERNAL, "candidate overflow on the exhaustive IVF plan");
        }
    }
    return LYNSE_OK;
}

// IVFIndex::search of an SQ8 index (ivf.rs:181-337), the index guard held.  The query is encoded and decoded; the POOL STAGE is
// the ordinary IVF search of the decoded query over the decoded slab store with k = pool = min(max(10 k, k), n) — the same centroid
// ranking, probe rule, all-lists-empty fallback, subset, kernels and plans (certified int8 pass, large-k path) — so each query's
// pool is the best min(pool, |candidates|) candidates by (decoded distance, original row), left in device memory.  The RERANK
// (PoolRerank, rerank_host.inc) scores them exactly against the original query and rows and keeps the best min(k, pool) by
// (exact distance, original row); a pool above what one workgroup's LDS sorts (16,384 keys) is selected on the host.
// The rerank adds its pool entries to the search context's rescored-candidate counter (lynse_hip_ivf_profile_get: pool_entries =
// the pool stage's exact rescoring + the rerank).
static int ivf_search_sq8(lynse_hip_ivf* h, const float* queries, uint64_t nq, uint32_t k, uint32_t nprobe,
                          uint64_t* out_rows, float* out_dists, uint32_t* out_counts, bool filtered,
                          const uint64_t* subset, uint64_t n_subset, bool on_device) {
    lynse_hip_flat* s = h->store;
    const uint64_t n = s->n;
    const uint32_t D = h->dim;
    auto zero_counts = [&]() -> int {
        if (on_device) return memset_done(out_counts, 0, nq * 4);
        memset(out_counts, 0, nq * 4);
        return LYNSE_OK;
    };
    if (n == 0 || k == 0) return zero_counts();
    if (filtered) {   // no subset row in the index: nothing to answer from (ivf.rs:267-269)
        bool any = false;
        for (uint64_t i = 0; i < n_subset && !any; ++i) any = subset[i] < n;
        if (!any) return zero_counts();
    }
    const uint32_t pool = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(10ull * k, k), n);
    const uint64_t qc = std::max<uint64_t>(1, std::min<uint64_t>(QCHUNK, (256ull << 20) / ((uint64_t)pool * 16)));
    auto& sc = h->sq;
    LY_HIP(hipSetDevice(s->device));
    PoolRerank::Search rr(sc.rr);
    LY_TRY(rr.begin(h->d_raw, n, D, D, h->metric, pool, k, k, qc, on_device, s->profiling.load(), "IVF-*-SQ8 rerank"));
    LY_TRY(ivf_grow(&sc.d_q, &sc.q_cap, (size_t)qc * D * 2));
    LY_TRY(ivf_grow(&sc.d_pdist, &sc.pdist_cap, (size_t)qc * pool));
    float* d_qo = sc.d_q;                       // original queries
    float* d_qd = sc.d_q + (size_t)qc * D;      // decoded queries
    for (uint64_t q0 = 0; q0 < nq; q0 += qc) {
        const uint32_t nqc = (uint32_t)std::min<uint64_t>(qc, nq - q0);
        {
            std::unique_lock<std::shared_mutex> lk(s->rw);
            LY_TRY(use_device(s));
            hipStream_t st = cur(s).stream;
            LY_HIP(hipMemcpyAsync(d_qo, queries + q0 * D, (size_t)nqc * D * 4, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
            LY_TRY(sq_codec_device(d_qo, nqc, D, h->d_sq, d_qd, st));
            LY_TRY(rr.pool_start(st));
            LY_HIP(hipStreamSynchronize(st));
        }
        // pool stage: the decoded queries over the decoded rows, k = pool, results left in device memory
        LY_TRY(ivf_search_locked(h, d_qd, nqc, pool, nprobe, sc.rr.d_prow, sc.d_pdist, sc.rr.d_pcnt, filtered, subset, n_subset, -1, true));
        std::unique_lock<std::shared_mutex> lk(s->rw);
        LY_TRY(use_device(s));
        LY_TRY(rr.run(d_qo, nqc, out_rows + q0 * k, out_dists + q0 * k, out_counts + q0, s->profiling.load() ? cur(s).ws.pool_total : nullptr,
                      cur(s).stream));
    }
    if (rr.timed) { h->sq_searches += 1; h->sq_pool_us += rr.pool_us; h->sq_rerank_us += rr.rerank_us; }
    return LYNSE_OK;
}

extern "C" int lynse_hip_ivf_search_f32(lynse_hip_ivf* h, const float* queries, uint64_t nq, uint32_t k, uint32_t nprobe,
                                        uint64_t* out_rows, float* out_dists, uint32_t* out_counts) {
    return ivf_search_impl(h, queries, nq, k, nprobe, out_rows, out_dists, out_counts, false, nullptr, 0);
}

// IvfFlatMmap::search(query, k, nprobe, metric) (ivf_flat_mmap.rs:225-305, PyIvfFlatIndex.search src/python/mod.rs:2130-2155):
// the partitions are metric-agnostic L2 cells, centroid routing, scoring and the sort direction follow the metric of the
// CALL.  Float indexes only (a binary index is tied to its quantizer and metric).
extern "C" int lynse_hip_ivf_search_metric_f32(lynse_hip_ivf* h, const float* queries, uint64_t nq, uint32_t k, uint32_t nprobe,
                                               int metric, uint64_t* out_rows, float* out_dists, uint32_t* out_counts) {
    if (!h) return set_error(LYNSE_ERR_INDEX_NOT_BUILT, "IVF index is not built");
    LY_TRY(metric_check(metric));
    bool is_binary, is_sq8;
    int index_metric;
    {   // (insert / delete swap the whole index structure under the guard: even its constant fields are read under it)
        IVF_GUARD(h);
        if (!h->store) return set_error(LYNSE_ERR_INDEX_NOT_BUILT, "IVF index is not built");
        is_binary = h->binary != 0;
        is_sq8 = h->sq8;
        index_metric = h->metric;
        if (h->spann) return set_error(LYNSE_ERR_UNSUPPORTED, "IvfFlatMmap::search(metric) is not defined for a SPANN index");
    }
    if (is_sq8) return set_error(LYNSE_ERR_UNSUPPORTED, "IvfFlatMmap::search(metric) is not defined for an IVF-*-SQ8 index (IVFIndex searches with its build metric)");
    if (is_binary || metric >= M_HAMMING) {
        if (metric == index_metric || (is_binary && metric >= M_HAMMING && (metric == M_TANIMOTO ? M_JACCARD : metric) == (index_metric == M_TANIMOTO ? M_JACCARD : index_metric)))
            return ivf_search_impl(h, queries, nq, k, nprobe, out_rows, out_dists, out_counts, false, nullptr, 0);
        return set_error(LYNSE_ERR_INVALID_ARGUMENT, "a binary IVF index searches with the metric it was built for, a float index with ip / l2 / cosine");
    }
    return ivf_search_impl(h, queries, nq, k, nprobe, out_rows, out_dists, out_counts, false, nullptr, 0, metric);
}

// lynse_hip_ivf_search_f32 with queries and outputs in device memory (a row-sharded IVF hands its per-rank candidates to the
// RCCL exchange without a host round trip).
extern "C" int lynse_hip_ivf_search_f32_device(lynse_hip_ivf* h, const float* d_queries, uint64_t nq, uint32_t k, uint32_t nprobe,
                                               uint64_t* d_out_rows, float* d_out_dists, uint32_t* d_out_counts) {
    return ivf_search_impl(h, d_queries, nq, k, nprobe, d_out_rows, d_out_dists, d_out_counts, false, nullptr, 0, -1, true);
}

extern "C" int lynse_hip_ivf_search_filtered_f32(lynse_hip_ivf* h, const float* queries, uint64_t nq, uint32_t k, uint32_t nprobe,
                                                 const uint64_t* subset_rows, uint64_t n_subset, uint64_t* out_rows,
                                                 float* out_dists, uint32_t* out_counts) {
    if (n_subset == 0) {  // an empty subset matches nothing
        if (!out_counts) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
        memset(out_counts, 0, nq * 4);
        return LYNSE_OK;
    }
    return ivf_search_impl(h, queries, nq, k, nprobe, out_rows, out_dists, out_counts, true, subset_rows, n_subset);
}

extern "C" int lynse_hip_ivf_profile_enable(lynse_hip_ivf* h, int on) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    IVF_GUARD(h);
    if (!h->store) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    return lynse_hip_flat_profile_enable(h->store, on);
}
extern "C" int lynse_hip_ivf_profile_get(lynse_hip_ivf* h, lynse_hip_profile* out, int reset) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    IVF_GUARD(h);
    if (!h->store) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    return lynse_hip_flat_profile_get(h->store, out, reset);
}
