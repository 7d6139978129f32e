// fields_host.inc — field filters (FieldStore::query_from_index, src/storage/field_store.rs:1527-1590): a handle of its own that holds
// typed field columns in HBM and evaluates a compiled predicate over them into BitSet words on the device.  Included at the end of
// lynse_hip.hip after text_host.inc; the kernel is in fields.h.  include/lynse_hip.h FIELD FILTERS, DESIGN.md §25.

constexpr uint32_t FIELD_MAX_COLUMNS = 4096;

struct FieldColumn {
    uint64_t n = 0, n_arrays = 0, n_elems = 0;
    uint8_t* d_tags = nullptr;
    uint64_t* d_payloads = nullptr;
    uint64_t* d_arr_ptr = nullptr;
    uint8_t* d_etags = nullptr;
    uint64_t* d_epayloads = nullptr;
    void release() {
        for (void* p : {(void*)d_tags, (void*)d_payloads, (void*)d_arr_ptr, (void*)d_etags, (void*)d_epayloads})
            if (p) (void)hipFree(p);
        *this = FieldColumn{};
    }
    uint64_t bytes() const { return n * 9 + (n_arrays ? (n_arrays + 1) * 8 : 0) + n_elems * 9; }
};

struct lynse_hip_fields {
    std::mutex mu;   // every call is a writer: the words and the program buffers are per handle
    int device = 0;
    uint32_t num_cu = 256;
    hipStream_t stream = nullptr;
    std::vector<FieldColumn> cols;
    // the result of the last filter and the scratch of a filter
    uint64_t* d_words = nullptr;
    size_t words_cap = 0;
    uint64_t n_words = 0;
    unsigned long long* d_count = nullptr;
    FieldLeafDev* d_leaves = nullptr;
    uint64_t* d_aux = nullptr;
    size_t aux_cap = 0;
    hipEvent_t ev[2] = {nullptr, nullptr};
};

extern "C" int lynse_hip_fields_create(int device, lynse_hip_fields** out) {
    if (!out) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    int ndev = 0;
    LY_TRY(lynse_hip_device_count(&ndev));
    if (ndev <= 0) return set_error(LYNSE_ERR_DEVICE, "no HIP device available (this library has no CPU fallback)");
    if (device < 0 || device >= ndev) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "device ordinal out of range");
    LY_HIP(hipSetDevice(device));
    auto* h = new lynse_hip_fields();
    h->device = device;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) h->num_cu = prop.multiProcessorCount;
    hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc(&h->d_count, 8);
    if (e == hipSuccess) e = hipMalloc(&h->d_leaves, sizeof(FieldLeafDev) * FIELD_MAX_LEAVES);
    if (e != hipSuccess) {
        lynse_hip_fields_destroy(h);
        return set_error(LYNSE_ERR_DEVICE, std::string("lynse_hip_fields_create: ") + hipGetErrorString(e));
    }
    *out = h;
    return LYNSE_OK;
}

extern "C" int lynse_hip_fields_destroy(lynse_hip_fields* h) {
    if (!h) return LYNSE_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (FieldColumn& c : h->cols) c.release();
    for (void* p : {(void*)h->d_words, (void*)h->d_count, (void*)h->d_leaves, (void*)h->d_aux})
        if (p) (void)hipFree(p);
    for (hipEvent_t e : h->ev)
        if (e) (void)hipEventDestroy(e);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return LYNSE_OK;
}

// Replaces the whole column.  Everything is checked before any device work; a failed upload leaves the column dropped, not torn.
extern "C" int lynse_hip_fields_set_column(lynse_hip_fields* h, uint32_t column, const uint8_t* tags, const uint64_t* payloads, uint64_t n,
                                           const uint64_t* arr_ptr, uint64_t n_arrays, const uint8_t* elem_tags, const uint64_t* elem_payloads) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    if (column >= FIELD_MAX_COLUMNS) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "field column id must be below 4096");
    if (n && (!tags || !payloads)) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_arrays && !arr_ptr) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    uint64_t n_elems = 0;
    if (n_arrays) {
        if (arr_ptr[0] != 0) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "field column: arr_ptr must start at 0");
        for (uint64_t a = 0; a < n_arrays; ++a)
            if (arr_ptr[a + 1] < arr_ptr[a]) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "field column: arr_ptr must not decrease");
        n_elems = arr_ptr[n_arrays];
        if (n_elems && (!elem_tags || !elem_payloads)) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
        for (uint64_t e = 0; e < n_elems; ++e)
            if (elem_tags[e] < FTAG_NULL || elem_tags[e] > FTAG_STR)
                return set_error(LYNSE_ERR_INVALID_ARGUMENT, "field column: an array element is null, a bool, a number or a string");
    }
    for (uint64_t r = 0; r < n; ++r) {
        if (tags[r] >= FTAG_COUNT) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "field column: unknown tag");
        if (tags[r] == FTAG_ARRAY && payloads[r] >= n_arrays)
            return set_error(LYNSE_ERR_INVALID_ARGUMENT, "field column: an array row's payload must index arr_ptr");
    }
    std::lock_guard<std::mutex> lk(h->mu);
    LY_HIP(hipSetDevice(h->device));
    if (column < h->cols.size()) h->cols[column].release();
    if (n == 0) return LYNSE_OK;
    if (column >= h->cols.size()) h->cols.resize((size_t)column + 1);
    FieldColumn c;
    auto fail = [&](int rc) {
        c.release();
        return rc;
    };
    auto up = [&](auto** dst, const void* src, size_t bytes) -> int {
        LY_HIP(hipMalloc(dst, bytes));
        return h2d_done(*dst, src, bytes);
    };
    int rc = up(&c.d_tags, tags, (size_t)n);
    if (rc == LYNSE_OK) rc = up(&c.d_payloads, payloads, (size_t)n * 8);
    if (rc == LYNSE_OK && n_arrays) rc = up(&c.d_arr_ptr, arr_ptr, ((size_t)n_arrays + 1) * 8);
    if (rc == LYNSE_OK && n_elems) rc = up(&c.d_etags, elem_tags, (size_t)n_elems);
    if (rc == LYNSE_OK && n_elems) rc = up(&c.d_epayloads, elem_payloads, (size_t)n_elems * 8);
    if (rc != LYNSE_OK) return fail(rc);
    c.n = n;
    c.n_arrays = n_arrays;
    c.n_elems = n_elems;
    h->cols[column] = c;
    return LYNSE_OK;
}

extern "C" int lynse_hip_fields_drop_column(lynse_hip_fields* h, uint32_t column) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    std::lock_guard<std::mutex> lk(h->mu);
    LY_HIP(hipSetDevice(h->device));
    if (column < h->cols.size()) h->cols[column].release();
    return LYNSE_OK;
}

extern "C" int lynse_hip_fields_column_rows(lynse_hip_fields* h, uint32_t column, uint64_t* out_rows) {
    if (!h || !out_rows) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    *out_rows = column < h->cols.size() ? h->cols[column].n : 0;
    return LYNSE_OK;
}

extern "C" uint64_t lynse_hip_fields_hbm_bytes(lynse_hip_fields* h) {
    if (!h) return 0;
    std::lock_guard<std::mutex> lk(h->mu);
    uint64_t b = (uint64_t)h->words_cap * 8 + (uint64_t)h->aux_cap * 8;
    for (const FieldColumn& c : h->cols) b += c.bytes();
    return b;
}

extern "C" int lynse_hip_fields_filter(lynse_hip_fields* h, uint64_t n, int combine, const lynse_hip_field_leaf* leaves, uint32_t n_leaves,
                                       const uint64_t* aux, uint64_t aux_words, uint64_t* out_count, float* out_kernel_us) {
    if (!h || !out_count) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    *out_count = 0;
    if (out_kernel_us) *out_kernel_us = 0.f;
    if (combine != LYNSE_FIELD_ALL && combine != LYNSE_FIELD_ANY) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "field filter: combine is ALL (0) or ANY (1)");
    if (n_leaves == 0 || n_leaves > FIELD_MAX_LEAVES) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "field filter: 1 to 32 leaves");
    if (!leaves || (aux_words && !aux)) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    LY_HIP(hipSetDevice(h->device));
    // every leaf against its column and the aux block, before anything is queued: the kernel reads what these checks bound
    FieldLeafDev dev[FIELD_MAX_LEAVES];
    for (uint32_t l = 0; l < n_leaves; ++l) {
        const lynse_hip_field_leaf& s = leaves[l];
        FieldLeafDev& d = dev[l];
        d = FieldLeafDev{};
        d.kind = s.kind;
        d.op = s.op;
        d.flags = s.flags;
        d.key_tag = s.key_tag;
        d.key = s.key;
        if (s.kind > FLEAF_CONTAINS) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "field filter: unknown leaf kind");
        if (s.kind == FLEAF_NUM_RANGE && s.op > FOP_GE) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "field filter: unknown range operator");
        if (s.kind == FLEAF_KEYSET) {
            if (s.aux_len > FIELD_MAX_KEYS) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "field filter: at most 65,536 keys per list");
            if (s.aux_off > aux_words || aux_words - s.aux_off < FIELD_KEYSET_HEAD + s.aux_len)
                return set_error(LYNSE_ERR_INVALID_ARGUMENT, "field filter: a key list lies outside aux");
            const uint64_t* st = aux + s.aux_off;
            if (st[0] != 0 || st[FTAG_COUNT] != s.aux_len) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "field filter: key list segment starts must run from 0 to aux_len");
            for (uint32_t t = 0; t < FTAG_COUNT; ++t) {
                if (st[t + 1] < st[t]) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "field filter: key list segment starts must not decrease");
                for (uint64_t i = st[t] + 1; i < st[t + 1]; ++i)
                    if (st[FIELD_KEYSET_HEAD + i - 1] >= st[FIELD_KEYSET_HEAD + i])
                        return set_error(LYNSE_ERR_INVALID_ARGUMENT, "field filter: the keys of a tag must be strictly ascending");
            }
        }
        if (s.kind == FLEAF_STRTABLE && (s.aux_off > aux_words || aux_words - s.aux_off < (s.aux_len + 63) / 64))
            return set_error(LYNSE_ERR_INVALID_ARGUMENT, "field filter: a string table lies outside aux");
        if (s.column == LYNSE_FIELD_NO_COLUMN || s.column >= h->cols.size() || h->cols[s.column].n == 0) continue;   // a field no row carries
        const FieldColumn& c = h->cols[s.column];
        if (c.n != n) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "field filter: a column does not hold n rows");
        d.tags = c.d_tags;
        d.payloads = c.d_payloads;
        d.arr_ptr = c.d_arr_ptr;
        d.etags = c.d_etags;
        d.epayloads = c.d_epayloads;
        d.n_arrays = c.n_arrays;
    }
    const uint64_t nw = (n + 63) / 64;
    h->n_words = 0;
    if (n == 0) return LYNSE_OK;
    LY_TRY(ivf_grow(&h->d_words, &h->words_cap, (size_t)nw));
    LY_TRY(ivf_grow(&h->d_aux, &h->aux_cap, (size_t)std::max<uint64_t>(1, aux_words)));
    for (uint32_t l = 0; l < n_leaves; ++l) {
        const bool has_aux = leaves[l].kind == FLEAF_KEYSET || leaves[l].kind == FLEAF_STRTABLE;
        dev[l].aux = has_aux ? h->d_aux + leaves[l].aux_off : nullptr;
        dev[l].aux_len = has_aux ? leaves[l].aux_len : 0;
    }
    for (hipEvent_t& e : h->ev)
        if (!e) LY_HIP(hipEventCreate(&e));
    hipStream_t st = h->stream;
    auto queued = [&](hipError_t e) -> int {   // (the copies of caller and stack memory must not outlive the call)
        if (e == hipSuccess) return LYNSE_OK;
        (void)hipStreamSynchronize(st);
        return set_error(LYNSE_ERR_DEVICE, std::string("lynse_hip_fields_filter: ") + hipGetErrorString(e));
    };
    if (aux_words) LY_TRY(queued(hipMemcpyAsync(h->d_aux, aux, (size_t)aux_words * 8, hipMemcpyHostToDevice, st)));
    LY_TRY(queued(hipMemcpyAsync(h->d_leaves, dev, sizeof(FieldLeafDev) * n_leaves, hipMemcpyHostToDevice, st)));
    LY_TRY(queued(hipMemsetAsync(h->d_count, 0, 8, st)));
    FieldFilterArgs a{};
    a.leaves = h->d_leaves;
    a.n_leaves = n_leaves;
    a.any = combine == LYNSE_FIELD_ANY ? 1u : 0u;
    a.n = n;
    a.words = h->d_words;
    a.count = h->d_count;
    // (grid-stride: at most 4 workgroups per CU, 262,144 rows a pass on 256 CUs)
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((n + FIELD_NT - 1) / FIELD_NT, (uint64_t)h->num_cu * 4);
    LY_TRY(queued(hipEventRecord(h->ev[0], st)));
    hipLaunchKernelGGL(k_field_filter, dim3(blocks), dim3(FIELD_NT), 0, st, a);
    LY_TRY(queued(hipGetLastError()));
    LY_TRY(queued(hipEventRecord(h->ev[1], st)));
    unsigned long long count = 0;
    LY_TRY(queued(hipMemcpyAsync(&count, h->d_count, 8, hipMemcpyDeviceToHost, st)));
    LY_HIP(hipStreamSynchronize(st));
    if (out_kernel_us) {
        float ms = 0.f;
        LY_HIP(hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
        *out_kernel_us = ms * 1000.0f;
    }
    h->n_words = nw;
    *out_count = (uint64_t)count;
    return LYNSE_OK;
}

extern "C" int lynse_hip_fields_words(lynse_hip_fields* h, uint64_t* out_words, uint64_t n_words) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    std::lock_guard<std::mutex> lk(h->mu);
    if (n_words != h->n_words) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "field filter: n_words is not the word count of the last filter");
    if (n_words == 0) return LYNSE_OK;
    if (!out_words) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    LY_HIP(hipSetDevice(h->device));
    LY_HIP(hipMemcpy(out_words, h->d_words, (size_t)n_words * 8, hipMemcpyDeviceToHost));
    return LYNSE_OK;
}

extern "C" int lynse_hip_fields_words_device(lynse_hip_fields* h, const uint64_t** out_d_words, uint64_t* out_n_words) {
    if (!h || !out_d_words || !out_n_words) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    *out_d_words = h->n_words ? h->d_words : nullptr;
    *out_n_words = h->n_words;
    return LYNSE_OK;
}

extern "C" int lynse_hip_flat_search_filtered_bitset_device_f32(lynse_hip_flat* h, const float* queries, uint64_t nq, uint32_t k, int metric,
                                                                const uint64_t* d_bitset_words, uint64_t n_words, uint64_t count,
                                                                uint64_t* out_rows, float* out_dists, uint32_t* out_counts) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    if (n_words && !d_bitset_words) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "bitset is NULL");
    const uint64_t n = lynse_hip_flat_len(h);
    if (count > n || (n_words < (1ull << 57) && count > n_words * 64)) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "count exceeds the rows the words cover");
    if (metric_additive(metric)) {   // the additive metrics keep their host-side subset plumbing
        std::vector<uint64_t> host(std::max<uint64_t>(1, n_words), 0ull);
        LY_TRY(use_device(h));
        if (n_words) LY_HIP(hipMemcpy(host.data(), d_bitset_words, (size_t)n_words * 8, hipMemcpyDeviceToHost));
        return additive_search(h, queries, nq, k, metric, true, nullptr, 0, host.data(), n_words, out_rows, out_dists, out_counts);
    }
    return search_impl(h, queries, false, nq, k, metric, out_rows, out_dists, out_counts, false, nullptr, nullptr, count, true,
                       d_bitset_words, n_words, false, true);
}

// ---- named vector fields: the device mask remap (include/lynse_hip.h NAMED VECTOR FIELDS, DESIGN.md §26) ----------------------------
// A handle of its own that holds row_of (field row -> collection row) in HBM and rewrites BitSet words over collection rows into
// BitSet words over field rows (k_bitset_remap, fields.h).  The map is uploaded whole; a remap leaves its words in the handle.

struct lynse_hip_rowmap {
    std::mutex mu;   // every call is a writer: the words are per handle
    int device = 0;
    uint32_t num_cu = 256;
    hipStream_t stream = nullptr;
    uint32_t* d_row_of = nullptr;
    size_t row_cap = 0;
    uint64_t n_out = 0;
    uint64_t bound = 0;      // 1 + the largest row_of entry that is not ROWMAP_NONE, 0 without one: what n_src + n_tail must reach
    bool has_map = false;
    uint64_t* d_src = nullptr;   // source words given from host memory
    size_t src_cap = 0;
    uint64_t* d_tail = nullptr;
    size_t tail_cap = 0;
    uint64_t* d_words = nullptr;
    size_t words_cap = 0;
    uint64_t n_words = 0;
    bool has_words = false;
    unsigned long long* d_count = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
};

extern "C" int lynse_hip_rowmap_create(int device, lynse_hip_rowmap** out) {
    if (!out) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    int ndev = 0;
    LY_TRY(lynse_hip_device_count(&ndev));
    if (ndev <= 0) return set_error(LYNSE_ERR_DEVICE, "no HIP device available (this library has no CPU fallback)");
    if (device < 0 || device >= ndev) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "device ordinal out of range");
    LY_HIP(hipSetDevice(device));
    auto* h = new lynse_hip_rowmap();
    h->device = device;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) h->num_cu = prop.multiProcessorCount;
    hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc(&h->d_count, 8);
    if (e != hipSuccess) {
        lynse_hip_rowmap_destroy(h);
        return set_error(LYNSE_ERR_DEVICE, std::string("lynse_hip_rowmap_create: ") + hipGetErrorString(e));
    }
    *out = h;
    return LYNSE_OK;
}

extern "C" int lynse_hip_rowmap_destroy(lynse_hip_rowmap* h) {
    if (!h) return LYNSE_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (void* p : {(void*)h->d_row_of, (void*)h->d_src, (void*)h->d_tail, (void*)h->d_words, (void*)h->d_count})
        if (p) (void)hipFree(p);
    for (hipEvent_t e : h->ev)
        if (e) (void)hipEventDestroy(e);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return LYNSE_OK;
}

// Replaces the whole map.  A failed upload leaves the handle without a map, not with a torn one.
extern "C" int lynse_hip_rowmap_set(lynse_hip_rowmap* h, const uint32_t* row_of, uint64_t n_out) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    if (n_out && !row_of) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_out >= (uint64_t)ROWMAP_NONE) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "row map: at most 2^32 - 2 rows");
    uint64_t bound = 0;
    for (uint64_t r = 0; r < n_out; ++r)
        if (row_of[r] != ROWMAP_NONE) bound = std::max<uint64_t>(bound, (uint64_t)row_of[r] + 1);
    std::lock_guard<std::mutex> lk(h->mu);
    LY_HIP(hipSetDevice(h->device));
    h->has_map = false;
    h->has_words = false;
    h->n_words = 0;
    LY_TRY(ivf_grow(&h->d_row_of, &h->row_cap, (size_t)std::max<uint64_t>(1, n_out)));
    if (n_out) LY_TRY(h2d_done(h->d_row_of, row_of, (size_t)n_out * 4));
    h->n_out = n_out;
    h->bound = bound;
    h->has_map = true;
    return LYNSE_OK;
}

extern "C" int lynse_hip_rowmap_len(lynse_hip_rowmap* h, uint64_t* out_rows, uint64_t* out_bound) {
    if (!h || !out_rows || !out_bound) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    *out_rows = h->has_map ? h->n_out : 0;
    *out_bound = h->has_map ? h->bound : 0;
    return LYNSE_OK;
}

extern "C" uint64_t lynse_hip_rowmap_hbm_bytes(lynse_hip_rowmap* h) {
    if (!h) return 0;
    std::lock_guard<std::mutex> lk(h->mu);
    return (uint64_t)h->row_cap * 4 + ((uint64_t)h->src_cap + h->tail_cap + h->words_cap) * 8;
}

extern "C" int lynse_hip_rowmap_remap(lynse_hip_rowmap* h, const uint64_t* src_words, uint64_t n_src_words, uint64_t n_src, int src_on_device,
                                      const uint64_t* tail_words, uint64_t n_tail_words, uint64_t n_tail, uint64_t* out_count,
                                      float* out_kernel_us) {
    if (!h || !out_count) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    *out_count = 0;
    if (out_kernel_us) *out_kernel_us = 0.f;
    // everything the kernel indexes with, before anything is queued
    if (n_src_words != (n_src + 63) / 64) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "row map: n_src_words is not the word count of n_src bits");
    if (n_tail_words != (n_tail + 63) / 64) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "row map: n_tail_words is not the word count of n_tail bits");
    if ((n_src_words && !src_words) || (n_tail_words && !tail_words)) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_src > (uint64_t)ROWMAP_NONE || n_tail > (uint64_t)ROWMAP_NONE || n_src + n_tail > (uint64_t)ROWMAP_NONE)
        return set_error(LYNSE_ERR_INVALID_ARGUMENT, "row map: the source rows must be numbered below 2^32 - 1");
    std::lock_guard<std::mutex> lk(h->mu);
    if (!h->has_map) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "row map: remap before set");
    if (h->bound > n_src + n_tail) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "row map: a row_of entry lies at or beyond n_src + n_tail");
    LY_HIP(hipSetDevice(h->device));
    const uint64_t n_out = h->n_out, nw = (n_out + 63) / 64;
    h->has_words = false;
    h->n_words = 0;
    if (n_out == 0) {
        h->has_words = true;
        return LYNSE_OK;
    }
    LY_TRY(ivf_grow(&h->d_words, &h->words_cap, (size_t)nw));
    if (n_tail_words) LY_TRY(ivf_grow(&h->d_tail, &h->tail_cap, (size_t)n_tail_words));
    if (!src_on_device && n_src_words) LY_TRY(ivf_grow(&h->d_src, &h->src_cap, (size_t)n_src_words));
    for (hipEvent_t& e : h->ev)
        if (!e) LY_HIP(hipEventCreate(&e));
    hipStream_t st = h->stream;
    auto queued = [&](hipError_t e) -> int {   // (the copies of caller memory must not outlive the call)
        if (e == hipSuccess) return LYNSE_OK;
        (void)hipStreamSynchronize(st);
        return set_error(LYNSE_ERR_DEVICE, std::string("lynse_hip_rowmap_remap: ") + hipGetErrorString(e));
    };
    if (!src_on_device && n_src_words) LY_TRY(queued(hipMemcpyAsync(h->d_src, src_words, (size_t)n_src_words * 8, hipMemcpyHostToDevice, st)));
    if (n_tail_words) LY_TRY(queued(hipMemcpyAsync(h->d_tail, tail_words, (size_t)n_tail_words * 8, hipMemcpyHostToDevice, st)));
    LY_TRY(queued(hipMemsetAsync(h->d_count, 0, 8, st)));
    BitsetRemapArgs a{};
    a.row_of = h->d_row_of;
    a.n_out = n_out;
    a.src = src_on_device ? src_words : h->d_src;
    a.n_src = n_src;
    a.tail = n_tail_words ? h->d_tail : nullptr;
    a.n_tail = n_tail;
    a.words = h->d_words;
    a.count = h->d_count;
    // (grid-stride as k_field_filter: at most 4 workgroups per CU, 262,144 rows a pass on 256 CUs)
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((n_out + FIELD_NT - 1) / FIELD_NT, (uint64_t)h->num_cu * 4);
    LY_TRY(queued(hipEventRecord(h->ev[0], st)));
    hipLaunchKernelGGL(k_bitset_remap, dim3(blocks), dim3(FIELD_NT), 0, st, a);
    LY_TRY(queued(hipGetLastError()));
    LY_TRY(queued(hipEventRecord(h->ev[1], st)));
    unsigned long long count = 0;
    LY_TRY(queued(hipMemcpyAsync(&count, h->d_count, 8, hipMemcpyDeviceToHost, st)));
    LY_HIP(hipStreamSynchronize(st));
    if (out_kernel_us) {
        float ms = 0.f;
        LY_HIP(hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
        *out_kernel_us = ms * 1000.0f;
    }
    h->n_words = nw;
    h->has_words = true;
    *out_count = (uint64_t)count;
    return LYNSE_OK;
}

extern "C" int lynse_hip_rowmap_words(lynse_hip_rowmap* h, uint64_t* out_words, uint64_t n_words) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    std::lock_guard<std::mutex> lk(h->mu);
    if (!h->has_words || n_words != h->n_words) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "row map: n_words is not the word count of the last remap");
    if (n_words == 0) return LYNSE_OK;
    if (!out_words) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    LY_HIP(hipSetDevice(h->device));
    LY_HIP(hipMemcpy(out_words, h->d_words, (size_t)n_words * 8, hipMemcpyDeviceToHost));
    return LYNSE_OK;
}

extern "C" int lynse_hip_rowmap_words_device(lynse_hip_rowmap* h, const uint64_t** out_d_words, uint64_t* out_n_words) {
    if (!h || !out_d_words || !out_n_words) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    *out_d_words = h->n_words ? h->d_words : nullptr;
    *out_n_words = h->n_words;
    return LYNSE_OK;
}
