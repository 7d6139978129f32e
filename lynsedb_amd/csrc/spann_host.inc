// spann_host.inc — SPANN-{IP,L2,COS}[-SQ8] entry points (SPANNIndex, src/index/spann.rs).  Included after ivf_host.inc.
//
// A SPANN index is an IVF handle (lynse_hip_ivf) with `spann` set: the centroids are k-means (train_for_metric, as IVFIndex),
// a row sits in up to replicas + 1 posting lists (k_spann_postings / k_spann_slow, spann.h), and the slab store holds one copy
// of the row per list it sits in, lists in ascending row order.  Search is the IVF list scan with k' = k (replicas + 1), cut
// to the first k distinct rows by k_spann_unique; a query with fewer than k distinct candidates is answered again over every
// list (spann.rs:376-379: fewer than k distinct candidates -> all rows).  SQ8 keeps the IVF-*-SQ8 layout: decoded rows in
// the slab store, the original rows in d_raw, the pool of min(max(10 k, k), candidates) distinct rows reranked by PoolRerank.

// The lists of n rows in HBM (`dim` floats each) under the centroids of `cs` (the centroid store, single-row kernels) /
// `centroids` (host copy): row i sits in lists[row_off[i] .. row_off[i + 1]), the first one its primary.
static int spann_postings(lynse_hip_flat* cs, const float* d_rows, uint64_t n, uint32_t dim, const float* centroids, uint32_t nlist,
                          int metric, uint32_t R, std::vector<uint64_t>* row_off, std::vector<uint32_t>* lists) {
    row_off->assign(n + 1, 0);
    lists->clear();
    if (n == 0) return LYNSE_OK;
    const uint32_t keep = std::min<uint32_t>(R + 1, nlist);
    float cmax = 0.0f;
    int cbad = 0;
    for (size_t i = 0; i < (size_t)nlist * dim; ++i) {
        if (!std::isfinite(centroids[i])) cbad = 1;
        else cmax = std::max(cmax, std::fabs(centroids[i]));
    }
    constexpr uint64_t B = 65536;   // rows per FLAT search of the top-keep
    const uint64_t nb = std::min<uint64_t>(B, n);
    uint8_t* d_flag = nullptr;
    uint32_t *d_lists = nullptr, *d_cnt = nullptr, *d_slow = nullptr, *d_nslow = nullptr, *d_tc = nullptr;
    uint64_t* d_tr = nullptr;
    float* d_td = nullptr;
    struct G { std::vector<void*> b; ~G() { for (void* p : b) if (p) (void)hipFree(p); } } g;
    auto alloc = [&](auto** p, size_t bytes) -> int {
        LY_HIP(hipMalloc(p, std::max<size_t>(bytes, 4)));
        g.b.push_back((void*)*p);
        return LYNSE_OK;
    };
    LY_TRY(alloc(&d_flag, n));
    LY_TRY(alloc(&d_lists, (size_t)n * keep * 4));
    LY_TRY(alloc(&d_cnt, (size_t)n * 4));
    LY_TRY(alloc(&d_slow, (size_t)n * 4));
    LY_TRY(alloc(&d_nslow, 4));
    LY_TRY(alloc(&d_tr, (size_t)nb * keep * 8));
    LY_TRY(alloc(&d_td, (size_t)nb * keep * 4));
    LY_TRY(alloc(&d_tc, (size_t)nb * 4));
    LY_TRY(memset_done(d_nslow, 0, 4));
    hipLaunchKernelGGL(k_spann_flag, dim3((uint32_t)std::min<uint64_t>((n + 3) / 4, 8192)), dim3(256), 0, 0, d_rows, dim, dim, n, cmax, metric,
                       cbad, d_flag);
    LY_HIP(hipGetLastError());
    LY_HIP(hipStreamSynchronize(nullptr));
    for (uint64_t r0 = 0; r0 < n; r0 += B) {
        const uint64_t nr = std::min<uint64_t>(B, n - r0);
        // the canonical (rank, centroid) top-keep: the exact FLAT search of the rows against the centroid store
        LY_TRY(lynse_hip_flat_search_f32_device(cs, d_rows + (size_t)r0 * dim, nr, keep, metric, d_tr, d_td, d_tc, nullptr));
        SpannPostArgs a{d_tr, d_td, d_tc, d_flag, nr, r0, keep, R, metric, d_lists, d_cnt, d_slow, d_nslow};
        hipLaunchKernelGGL(k_spann_postings, dim3((uint32_t)((nr + 255) / 256)), dim3(256), 0, 0, a);
        LY_HIP(hipGetLastError());
        LY_HIP(hipStreamSynchronize(nullptr));
    }
    uint32_t n_slow = 0;
    LY_HIP(hipMemcpy(&n_slow, d_nslow, 4, hipMemcpyDeviceToHost));
    if (n_slow) {   // rows that can meet a NaN / infinite rank: the sequential rule over every centroid
        const size_t lds = (size_t)nlist * 4 + (size_t)keep * 8;
        LY_TRY(ensure_lds<k_spann_slow>(16384 * 4 + SPANN_MAX_KEEP * 8));
        hipLaunchKernelGGL(k_spann_slow, dim3(n_slow), dim3(256), lds, 0, d_rows, dim, cs->rows, cs->ld, dim, nlist, keep, R, metric, d_slow,
                           d_lists, d_cnt);
        LY_HIP(hipGetLastError());
        LY_HIP(hipStreamSynchronize(nullptr));
    }
    std::vector<uint32_t> cnt(n), all((size_t)n * keep);
    LY_HIP(hipMemcpy(cnt.data(), d_cnt, (size_t)n * 4, hipMemcpyDeviceToHost));
    LY_HIP(hipMemcpy(all.data(), d_lists, (size_t)n * keep * 4, hipMemcpyDeviceToHost));
    for (uint64_t r = 0; r < n; ++r) {
        if (cnt[r] == 0 || cnt[r] > keep) return set_error(LYNSE_ERR_INTERNAL, "SPANN posting count out of range");
        (*row_off)[r + 1] = (*row_off)[r] + cnt[r];
    }
    lists->resize((*row_off)[n]);
    for (uint64_t r = 0; r < n; ++r)
        for (uint32_t j = 0; j < cnt[r]; ++j) {
            const uint32_t c = all[(size_t)r * keep + j];
            if (c >= nlist) return set_error(LYNSE_ERR_INTERNAL, "SPANN posting list out of range");
            (*lists)[(*row_off)[r] + j] = c;
        }
    return LYNSE_OK;
}

// the centroid matrix as a FLAT shard with the single-row kernels (as ivf_assemble builds it)
static int spann_centroid_store(const float* centroids, uint32_t nlist, uint32_t dim, int device, lynse_hip_flat** out) {
    LY_TRY(lynse_hip_flat_create(dim, device, out));
    int rc = lynse_hip_flat_append_f32(*out, centroids, nlist);
    if (rc == LYNSE_OK) rc = lynse_hip_flat_set_ip_form(*out, LYNSE_IPFORM_SINGLE);
    if (rc == LYNSE_OK) rc = lynse_hip_flat_finalize(*out);
    if (rc != LYNSE_OK) { lynse_hip_flat_destroy(*out); *out = nullptr; }
    return rc;
}

static int spann_check(uint64_t n, uint32_t dim, int metric, uint32_t R) {
    if (metric != M_IP && metric != M_L2 && metric != M_COS) return set_error(LYNSE_ERR_UNSUPPORTED, "SPANN is defined for ip / l2 / cosine");
    if (R + 1 > SPANN_MAX_KEEP) return set_error(LYNSE_ERR_UNSUPPORTED, "replica_count > 63 is not supported");
    if (n == 0) return set_error(LYNSE_ERR_INDEX_NOT_BUILT, "no vectors to index");
    if ((uint64_t)n * (R + 1) > 0xfffffff0ull) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "SPANN posting count exceeds the u32 position capacity");
    (void)dim;
    return LYNSE_OK;
}

// the common part of build and load: rows (host) -> d_rows (decoded under SQ8) [+ d_raw, d_sq]; centroids == NULL trains them;
// list_off / list_rows == NULL derives the lists with the posting rule
static int spann_common(const float* rows, uint64_t n, uint32_t dim, uint32_t nlist, uint32_t max_iter, int metric, uint32_t R,
                        int sq8, const float* mins_in, const float* scales_in, const float* centroids, const uint64_t* list_off,
                        const uint32_t* list_rows, int device, lynse_hip_ivf** out) {
    LY_TRY(spann_check(n, dim, metric, R));
    float *d_raw = nullptr, *d_dec = nullptr, *d_sq = nullptr;
    struct G { float*& a; float*& b; float*& c; ~G() { for (float* p : {a, b, c}) if (p) (void)hipFree(p); } } g{d_raw, d_dec, d_sq};
    std::vector<float> mins, scales, cen;
    std::vector<uint32_t> asg;
    if (sq8) {
        LY_TRY(sq_prepare(rows, n, dim, mins_in, scales_in, device, &d_raw, &d_dec, &d_sq, &mins, &scales));
    } else {
        LY_HIP(hipSetDevice(device));
        LY_HIP(hipMalloc(&d_dec, (size_t)n * dim * 4));
        LY_TRY(h2d_done(d_dec, rows, (size_t)n * dim * 4));
    }
    std::vector<uint64_t> row_off;
    std::vector<uint32_t> lists;
    if (!centroids) {   // train_for_metric(decoded, n, dim, n_clusters, 20, metric) (spann.rs:291-298)
        uint32_t k = 0;
        LY_TRY(ivf_kmeans(d_dec, n, dim, nlist, max_iter, metric, device, &cen, &asg, &k, true));
        if (k == 0) return set_error(LYNSE_ERR_INDEX_NOT_BUILT, "no vectors to index");
        nlist = k;
        centroids = cen.data();
    } else {
        cen.assign(centroids, centroids + (size_t)nlist * dim);
    }
    if (list_off) {   // load: the lists as given (list-major CSR) -> row-major
        if (list_off[0] != 0) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "list offsets must start at 0");
        std::vector<uint64_t> per(n + 1, 0);
        for (uint32_t c = 0; c < nlist; ++c) {
            if (list_off[c + 1] < list_off[c]) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "list offsets must not decrease");
            for (uint64_t p = list_off[c]; p < list_off[c + 1]; ++p) {
                if (list_rows[p] >= n) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "list row out of range");
                per[list_rows[p] + 1] += 1;
            }
        }
        // every row in 1 .. R + 1 distinct lists: the search relies on it (k (R + 1) keys hold k distinct rows), insert / delete
        // gather every row from one of its positions
        for (uint64_t r = 0; r < n; ++r)
            if (per[r + 1] == 0 || per[r + 1] > (uint64_t)R + 1)
                return set_error(LYNSE_ERR_INVALID_ARGUMENT, "every row must sit in 1 .. replica_count + 1 lists");
        for (uint64_t r = 0; r < n; ++r) per[r + 1] += per[r];
        row_off = per;
        lists.resize(per[n]);
        std::vector<uint64_t> wp(per.begin(), per.end() - 1);
        for (uint32_t c = 0; c < nlist; ++c)
            for (uint64_t p = list_off[c]; p < list_off[c + 1]; ++p) lists[wp[list_rows[p]]++] = c;
        for (uint64_t r = 0; r < n; ++r)   // (a row's lists come out in ascending order: a repeat is a neighbour)
            for (uint64_t j = per[r] + 1; j < per[r + 1]; ++j)
                if (lists[j] == lists[j - 1]) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "a row sits twice in one list");
    } else if (R == 0) {   // the k-means assignments are the lists (spann.rs:300-303)
        row_off.resize(n + 1);
        for (uint64_t r = 0; r <= n; ++r) row_off[r] = r;
        lists = asg;
    } else {   // the posting rule against the final centroids (spann.rs:304-306)
        lynse_hip_flat* cs = nullptr;
        LY_TRY(spann_centroid_store(centroids, nlist, dim, device, &cs));
        const int rc = spann_postings(cs, d_dec, n, dim, centroids, nlist, metric, R, &row_off, &lists);
        lynse_hip_flat_destroy(cs);
        LY_TRY(rc);
    }
    LY_TRY(ivf_assemble(d_dec, n, dim, centroids, nlist, lists.data(), metric, 0, device, out, true, nullptr, row_off.data()));
    lynse_hip_ivf* h = *out;
    h->spann = true;
    h->replicas = R;
    h->n_rows = n;
    // the fused few-query list scan assumes one slab position per row: its selection loses the second copy of a (distance, row)
    // key, so a SPANN store always takes the staged pipeline (the setting moves over with insert / delete, ivf_adopt)
    h->store->no_fused = 1;
    if (sq8) {
        h->sq8 = true;
        h->sq_min = std::move(mins);
        h->sq_scale = std::move(scales);
        std::swap(h->d_sq, d_sq);
        std::swap(h->d_raw, d_raw);
    }
    return LYNSE_OK;
}

extern "C" int lynse_hip_spann_build(const float* rows, uint64_t n, uint32_t dim, uint32_t nlist, uint32_t max_iter, int metric,
                                     uint32_t replica_count, int sq8, int device, lynse_hip_ivf** out) {
    LY_TRY(ivf_check_args(rows, n, dim, nlist, metric, out));
    return spann_common(rows, n, dim, nlist, max_iter, metric, replica_count, sq8, nullptr, nullptr, nullptr, nullptr, nullptr, device, out);
}

extern "C" int lynse_hip_spann_load(const float* rows, uint64_t n, uint32_t dim, const float* centroids, uint32_t nlist,
                                    const uint64_t* list_offsets, const uint32_t* list_rows, uint32_t replica_count, int metric,
                                    const float* mins, const float* scales, int device, lynse_hip_ivf** out) {
    LY_TRY(ivf_check_args(rows, n, dim, nlist, metric, out));
    if (!centroids || !list_offsets || (!list_rows && list_offsets[nlist])) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!mins != !scales) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "mins and scales go together");
    return spann_common(rows, n, dim, nlist, 0, metric, replica_count, mins ? 1 : 0, mins, scales, centroids, list_offsets, list_rows, device, out);
}

extern "C" int lynse_hip_spann_postings(const lynse_hip_ivf* h, uint64_t* offsets, uint32_t* rows, uint64_t* n_postings) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "not a SPANN index");
    IVF_GUARD(h);
    if (!h->spann) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "not a SPANN index");
    if (n_postings) *n_postings = h->orig.size();
    if (offsets) memcpy(offsets, h->offsets.data(), h->offsets.size() * 8);
    if (rows) memcpy(rows, h->orig.data(), h->orig.size() * 4);
    return LYNSE_OK;
}

extern "C" int lynse_hip_spann_replica_count(const lynse_hip_ivf* h, uint32_t* replica_count) {
    if (!h || !replica_count) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    IVF_GUARD(h);
    if (!h->spann) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "not a SPANN index");
    *replica_count = h->replicas;
    return LYNSE_OK;
}

// ------------------------------------------------------------------------------- insert / delete ----
// The rows of the index in original row order, in HBM (decoded rows under SQ8): row r is gathered from its first slab position.
static int spann_rows_in_order(lynse_hip_ivf* h, const std::vector<uint32_t>& rows, float* d_out) {
    if (rows.empty()) return LYNSE_OK;
    std::vector<uint32_t> first(h->n_rows, 0xffffffffu);
    for (uint64_t p = h->orig.size(); p-- > 0;) first[h->orig[p]] = (uint32_t)p;
    std::vector<uint32_t> pos(rows.size());
    for (size_t i = 0; i < rows.size(); ++i) {
        pos[i] = first[rows[i]];
        if (pos[i] == 0xffffffffu) return set_error(LYNSE_ERR_INTERNAL, "a SPANN row sits in no list");
    }
    uint32_t* d_pos = nullptr;
    struct G { uint32_t*& p; ~G() { if (p) (void)hipFree(p); } } g{d_pos};
    LY_HIP(hipMalloc(&d_pos, pos.size() * 4));
    LY_TRY(h2d_done(d_pos, pos.data(), pos.size() * 4));
    const uint64_t pieces = (uint64_t)pos.size() * ((h->dim + 3) / 4);
    hipLaunchKernelGGL(k_gather_rows_f32, dim3((uint32_t)std::min<uint64_t>((pieces + 255) / 256, 8192)), dim3(256), 0, 0,
                       h->store->rows, h->store->ld, d_pos, (uint64_t)pos.size(), d_out, h->dim, h->dim);
    LY_HIP(hipGetLastError());
    LY_HIP(hipStreamSynchronize(nullptr));
    return LYNSE_OK;
}

// re-assemble over n rows in HBM (original row order) with their lists, and hand the index over (new_raw: ivf_adopt)
static int spann_reassemble(lynse_hip_ivf* h, const float* d_rows, uint64_t n, const std::vector<uint64_t>& row_off,
                            const std::vector<uint32_t>& lists, float* new_raw) {
    lynse_hip_ivf* fresh = nullptr;
    LY_TRY(ivf_assemble(d_rows, n, h->dim, h->centroids.data(), h->nlist, lists.data(), h->metric, 0, h->store->device, &fresh, true, nullptr,
                        row_off.data()));
    fresh->n_rows = n;
    return ivf_adopt(h, fresh, new_raw);
}

// SPANNIndex::insert (spann.rs:459-509): the new rows are encoded with the fitted quantizer (no refit), placed by the posting rule
// against the unchanged centroids and appended to the end of each of their lists.
static int spann_insert(lynse_hip_ivf* h, const float* rows, uint64_t n) {
    const uint64_t old_n = h->n_rows, total = old_n + n;
    const uint32_t D = h->dim;
    if (total * (h->replicas + 1) > 0xfffffff0ull) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "SPANN posting count exceeds the u32 position capacity");
    LY_HIP(hipSetDevice(h->store->device));
    float *d_all = nullptr, *d_new = nullptr, *new_raw = nullptr;
    struct G { float*& a; float*& b; float*& c; ~G() { for (float* p : {a, b, c}) if (p) (void)hipFree(p); } } g{d_all, d_new, new_raw};
    LY_HIP(hipMalloc(&d_all, (size_t)total * D * 4));
    const float* d_routed = nullptr;   // the new rows as the index sees them (decoded under SQ8)
    if (h->sq8) {
        LY_TRY(sq_decode_host(h, rows, n, nullptr, &d_new));   // (d_new: originals, then the decoded rows; no host copy)
        d_routed = d_new + (size_t)n * D;
        LY_HIP(hipMalloc(&new_raw, (size_t)total * D * 4));
        if (old_n) LY_HIP(hipMemcpy(new_raw, h->d_raw, (size_t)old_n * D * 4, hipMemcpyDeviceToDevice));
        LY_HIP(hipMemcpy(new_raw + (size_t)old_n * D, d_new, (size_t)n * D * 4, hipMemcpyDeviceToDevice));
    } else {
        LY_HIP(hipMalloc(&d_new, (size_t)n * D * 4));
        LY_TRY(h2d_done(d_new, rows, (size_t)n * D * 4));
        d_routed = d_new;
    }
    std::vector<uint64_t> new_off;
    std::vector<uint32_t> new_lists;
    LY_TRY(spann_postings(h->cstore, d_routed, n, D, h->centroids.data(), h->nlist, h->metric, h->replicas, &new_off, &new_lists));
    // the old rows' lists (from the slab layout), then the new ones
    std::vector<uint64_t> row_off(total + 1, 0);
    for (uint64_t p = 0; p < h->orig.size(); ++p) row_off[h->orig[p] + 1] += 1;
    for (uint64_t r = 0; r < old_n; ++r) row_off[r + 1] += row_off[r];
    std::vector<uint32_t> lists(row_off[old_n] + new_lists.size());
    {
        std::vector<uint64_t> wp(row_off.begin(), row_off.begin() + old_n);
        for (uint32_t c = 0; c < h->nlist; ++c)
            for (uint64_t p = h->offsets[c]; p < h->offsets[c + 1]; ++p) lists[wp[h->orig[p]]++] = c;
    }
    for (uint64_t r = 0; r < n; ++r) row_off[old_n + r + 1] = row_off[old_n] + new_off[r + 1];
    std::copy(new_lists.begin(), new_lists.end(), lists.begin() + row_off[old_n]);
    std::vector<uint32_t> old_rows(old_n);
    for (uint64_t r = 0; r < old_n; ++r) old_rows[r] = (uint32_t)r;
    LY_TRY(spann_rows_in_order(h, old_rows, d_all));
    LY_HIP(hipMemcpy(d_all + (size_t)old_n * D, d_routed, (size_t)n * D * 4, hipMemcpyDeviceToDevice));
    LY_TRY(spann_reassemble(h, d_all, total, row_off, lists, new_raw));
    new_raw = nullptr;   // (owned by the index now)
    return LYNSE_OK;
}

// SPANNIndex::delete (spann.rs:435-457): the rows go, the rest keep their order under consecutive row ids, and ALL lists are
// rebuilt with the posting rule (replicas = 0 included: the lists then follow the final centroids, not the k-means assignments).
static int spann_delete(lynse_hip_ivf* h, const uint64_t* row_ids, uint64_t n_ids) {
    const uint64_t old_n = h->n_rows;
    const uint32_t D = h->dim;
    std::vector<bool> gone(old_n, false);
    for (uint64_t i = 0; i < n_ids; ++i)
        if (row_ids[i] < old_n) gone[row_ids[i]] = true;   // unknown ids are ignored
    std::vector<uint32_t> keep;
    keep.reserve(old_n);
    for (uint64_t r = 0; r < old_n; ++r)
        if (!gone[r]) keep.push_back((uint32_t)r);
    const uint64_t m = keep.size();
    LY_HIP(hipSetDevice(h->store->device));
    float *d_all = nullptr, *new_raw = nullptr;
    uint32_t* d_keep = nullptr;
    struct G { float*& a; float*& b; uint32_t*& c; ~G() { if (a) (void)hipFree(a); if (b) (void)hipFree(b); if (c) (void)hipFree(c); } } g{d_all, new_raw, d_keep};
    LY_HIP(hipMalloc(&d_all, std::max<size_t>((size_t)m * D * 4, 4)));
    LY_TRY(spann_rows_in_order(h, keep, d_all));
    if (h->sq8) {   // the original rows that are kept, in order
        LY_HIP(hipMalloc(&new_raw, std::max<size_t>((size_t)m * D * 4, 4)));
        if (m) {
            LY_HIP(hipMalloc(&d_keep, (size_t)m * 4));
            LY_TRY(h2d_done(d_keep, keep.data(), (size_t)m * 4));
            const uint64_t pieces = m * ((D + 3) / 4);
            hipLaunchKernelGGL(k_gather_rows_f32, dim3((uint32_t)std::min<uint64_t>((pieces + 255) / 256, 8192)), dim3(256), 0, 0,
                               h->d_raw, D, d_keep, m, new_raw, D, D);
            LY_HIP(hipGetLastError());
            LY_HIP(hipStreamSynchronize(nullptr));
        }
    }
    std::vector<uint64_t> row_off;
    std::vector<uint32_t> lists;
    LY_TRY(spann_postings(h->cstore, d_all, m, D, h->centroids.data(), h->nlist, h->metric, h->replicas, &row_off, &lists));
    LY_TRY(spann_reassemble(h, d_all, m, row_off, lists, new_raw));
    new_raw = nullptr;
    return LYNSE_OK;
}

// ------------------------------------------------------------------------------------------ search ----
// The k_spann_unique launch on the slab store's stream, the store lock held: `nq` queries of `in_k` keys in sp.d_rows / d_dists / d_cnt
// -> the first k_sel distinct rows of output query qmap[q] at stride out_k.
static int spann_unique(lynse_hip_ivf* h, uint32_t nq, uint32_t in_k, uint32_t k_sel, const uint32_t* d_qmap, uint64_t* d_orow, float* d_odist,
                        uint32_t* d_ocnt, uint32_t out_k) {
    lynse_hip_flat* s = h->store;
    std::unique_lock<std::shared_mutex> lk(s->rw);
    LY_TRY(use_device(s));
    hipStream_t st = cur(s).stream;
    hipLaunchKernelGGL(k_spann_unique, dim3(nq), dim3(64), 0, st, h->sp.d_rows, d_odist ? h->sp.d_dists : nullptr, h->sp.d_cnt, in_k, nq, k_sel,
                       d_qmap, d_orow, d_odist, d_ocnt, out_k, metric_ascending(h->metric) ? 1 : 0);
    LY_HIP(hipGetLastError());
    LY_HIP(hipStreamSynchronize(st));
    return LYNSE_OK;
}

// One chunk of device queries d_q (nqc of them): the list scan with k' = k_sel (replicas + 1) keys, cut to the first k_sel distinct rows
// (d_orow / d_odist at stride out_k, counts d_ocnt); the queries with fewer than k_min distinct candidates run again over every list.
static int spann_chunk(lynse_hip_ivf* h, const float* d_q, uint32_t nqc, uint32_t k_sel, uint32_t k_min, uint32_t nprobe, bool filtered,
                       const uint64_t* subset, uint64_t n_subset, uint64_t* d_orow, float* d_odist, uint32_t* d_ocnt, uint32_t out_k) {
    auto& sp = h->sp;
    const uint64_t kp = (uint64_t)k_sel * (h->replicas + 1);
    const uint32_t D = h->dim;
    LY_TRY(ivf_search_locked(h, d_q, nqc, (uint32_t)kp, nprobe, sp.d_rows, sp.d_dists, sp.d_cnt, filtered, subset, n_subset, -1, true));
    LY_TRY(spann_unique(h, nqc, (uint32_t)kp, k_sel, nullptr, d_orow, d_odist, d_ocnt, out_k));
    const uint32_t np_eff = std::min<uint32_t>(std::max<uint32_t>(nprobe, 1), h->nlist);
    if (np_eff >= h->nlist) return LYNSE_OK;   // (every list probed already: nothing more to find)
    std::vector<uint32_t> cnt(nqc), redo;
    LY_HIP(hipMemcpy(cnt.data(), d_ocnt, (size_t)nqc * 4, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < nqc; ++i)
        if (cnt[i] < k_min) redo.push_back(i);
    if (redo.empty()) return LYNSE_OK;
    // fewer than k distinct candidates (spann.rs:376-379): the candidates become all (subset) rows = every list probed
    float* d_rq = sp.d_q + (size_t)nqc * D;   // (the second half of the query buffer)
    LY_HIP(hipMemcpy(sp.d_qmap, redo.data(), redo.size() * 4, hipMemcpyHostToDevice));
    const uint64_t pieces = (uint64_t)redo.size() * ((D + 3) / 4);
    hipLaunchKernelGGL(k_gather_rows_f32, dim3((uint32_t)std::min<uint64_t>((pieces + 255) / 256, 8192)), dim3(256), 0, 0, d_q, D, sp.d_qmap,
                       (uint64_t)redo.size(), d_rq, D, D);
    LY_HIP(hipGetLastError());
    LY_HIP(hipStreamSynchronize(nullptr));
    LY_TRY(ivf_search_locked(h, d_rq, (uint32_t)redo.size(), (uint32_t)kp, h->nlist, sp.d_rows, sp.d_dists, sp.d_cnt, filtered, subset, n_subset, -1, true));
    return spann_unique(h, (uint32_t)redo.size(), (uint32_t)kp, k_sel, sp.d_qmap, d_orow, d_odist, d_ocnt, out_k);
}

// SPANNIndex::search (spann.rs:326-433), the index guard held.  Plain modes: the top k distinct rows by (distance, row).  SQ8: the
// query is encoded and decoded, the pool = min(max(10 k, k), |candidates|) distinct rows by decoded distance is reranked exactly
// against the original query and rows (PoolRerank), the best min(k, pool) kept.
static int spann_search(lynse_hip_ivf* h, const float* queries, uint64_t nq, uint32_t k, uint32_t nprobe,
                        uint64_t* out_rows, float* out_dists, uint32_t* out_counts, bool filtered, const uint64_t* subset, uint64_t n_subset) {
    lynse_hip_flat* s = h->store;
    const uint64_t n = h->n_rows;
    const uint32_t D = h->dim;
    if (n == 0) return set_error(LYNSE_ERR_INDEX_NOT_BUILT, "SPANN index is not built");   // spann.rs:332-334
    if (k == 0) { memset(out_counts, 0, nq * 4); return LYNSE_OK; }
    if (filtered) {   // no subset row in the index: no candidates, not even after the fallback — every slot padded
        bool any = false;
        for (uint64_t i = 0; i < n_subset && !any; ++i) any = subset[i] < n;
        if (!any) {
            const float worst = metric_ascending(h->metric) ? INFINITY : -INFINITY;
            for (uint64_t i = 0; i < nq * k; ++i) { out_rows[i] = ~0ull; out_dists[i] = worst; }
            memset(out_counts, 0, nq * 4);
            return LYNSE_OK;
        }
    }
    const uint32_t k_sel = h->sq8 ? (uint32_t)std::min<uint64_t>(std::max<uint64_t>(10ull * k, k), n) : (uint32_t)std::min<uint64_t>(k, n);
    const uint64_t kp = (uint64_t)k_sel * (h->replicas + 1);
    if (kp > 0xffffffffull) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "k x (replica_count + 1) exceeds the u32 range");
    const uint64_t qc = std::max<uint64_t>(1, std::min<uint64_t>(QCHUNK, (256ull << 20) / (kp * 16)));
    auto& sp = h->sp;
    LY_HIP(hipSetDevice(s->device));
    LY_TRY(ivf_grow(&sp.d_q, &sp.q_cap, (size_t)qc * D * 2));
    LY_TRY(ivf_grow(&sp.d_rows, &sp.rows_cap, (size_t)qc * kp));
    LY_TRY(ivf_grow(&sp.d_dists, &sp.dists_cap, (size_t)qc * kp));
    LY_TRY(ivf_grow(&sp.d_cnt, &sp.cnt_cap, (size_t)qc));
    LY_TRY(ivf_grow(&sp.d_qmap, &sp.qmap_cap, (size_t)qc));
    if (!h->sq8) {
        LY_TRY(ivf_grow(&sp.d_orow, &sp.orow_cap, (size_t)qc * k));
        LY_TRY(ivf_grow(&sp.d_odist, &sp.odist_cap, (size_t)qc * k));
        LY_TRY(ivf_grow(&sp.d_ocnt, &sp.ocnt_cap, (size_t)qc));
        for (uint64_t q0 = 0; q0 < nq; q0 += qc) {
            const uint32_t nqc = (uint32_t)std::min<uint64_t>(qc, nq - q0);
            LY_TRY(h2d_done(sp.d_q, queries + q0 * D, (size_t)nqc * D * 4));
            LY_TRY(spann_chunk(h, sp.d_q, nqc, k_sel, k_sel, nprobe, filtered, subset, n_subset, sp.d_orow, sp.d_odist, sp.d_ocnt, k));
            LY_HIP(hipMemcpy(out_rows + q0 * k, sp.d_orow, (size_t)nqc * k * 8, hipMemcpyDeviceToHost));
            LY_HIP(hipMemcpy(out_dists + q0 * k, sp.d_odist, (size_t)nqc * k * 4, hipMemcpyDeviceToHost));
            LY_HIP(hipMemcpy(out_counts + q0, sp.d_ocnt, (size_t)nqc * 4, hipMemcpyDeviceToHost));
        }
        return LYNSE_OK;
    }
    // SQ8: the pool stage leaves the distinct pool rows in PoolRerank's d_prow / d_pcnt
    auto& sc = h->sq;
    PoolRerank::Search rr(sc.rr);
    LY_TRY(rr.begin(h->d_raw, n, D, D, h->metric, k_sel, k, k, qc, false, s->profiling.load(), "SPANN-*-SQ8 rerank"));
    LY_TRY(ivf_grow(&sc.d_q, &sc.q_cap, (size_t)qc * D));
    const uint32_t k_min = (uint32_t)std::min<uint64_t>(k, n);
    for (uint64_t q0 = 0; q0 < nq; q0 += qc) {
        const uint32_t nqc = (uint32_t)std::min<uint64_t>(qc, nq - q0);
        {
            std::unique_lock<std::shared_mutex> lk(s->rw);
            LY_TRY(use_device(s));
            hipStream_t st = cur(s).stream;
            LY_HIP(hipMemcpyAsync(sc.d_q, queries + q0 * D, (size_t)nqc * D * 4, hipMemcpyHostToDevice, st));
            LY_TRY(sq_codec_device(sc.d_q, nqc, D, h->d_sq, sp.d_q, st));
            LY_TRY(rr.pool_start(st));
            LY_HIP(hipStreamSynchronize(st));
        }
        // (the pool keeps no distances: k_spann_unique writes rows and counts only)
        LY_TRY(spann_chunk(h, sp.d_q, nqc, k_sel, k_min, nprobe, filtered, subset, n_subset, sc.rr.d_prow, nullptr, sc.rr.d_pcnt, k_sel));
        std::unique_lock<std::shared_mutex> lk(s->rw);
        LY_TRY(use_device(s));
        LY_TRY(rr.run(sc.d_q, nqc, out_rows + q0 * k, out_dists + q0 * k, out_counts + q0, s->profiling.load() ? cur(s).ws.pool_total : nullptr,
                      cur(s).stream));
    }
    if (rr.timed) { h->sq_searches += 1; h->sq_pool_us += rr.pool_us; h->sq_rerank_us += rr.rerank_us; }
    return LYNSE_OK;
}
