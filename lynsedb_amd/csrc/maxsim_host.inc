// maxsim_host.inc — multi-vector search (MaxSim: score(Q, P) = sum_i max_j <q_i, p_j>): a handle of its own that holds the token rows
// of the records in HBM, append-only.  Included at the end of lynse_hip.hip after mutate_host.inc; the kernel is in maxsim.h.  The
// search is the additive search's shape: one exact scan into S[q][record], then the shared cut (ScoreCut::cut<true>) and order
// (k_pool_select, or select_pool_keys beyond 16,384 keys), descending as for ip.  include/lynse_hip.h, MULTI-VECTOR SEARCH; DESIGN.md §28.
// The rerank entry and a filtered search that leaves few tokens run the candidate kernels instead of the scan (MULTI-VECTOR RERANK; §31).

struct lynse_hip_multivec {
    std::shared_mutex rw;
    int device = 0;
    uint32_t num_cu = 256;
    hipStream_t stream = nullptr;
    uint32_t dim = 0, ld = 0;
    int dtype = 0;                          // 0: f32 rows in `tokens`, k_maxsim_scan; 1: f16 rows in `tokens_h`, k_maxsim_h16 (same pitch in elements)
                                            // 2 (internal, lynse_hip_multivec_create_i8): codes in `tokens_i8` + `scales`, k_maxsim_i8
    DevBuf<uint16_t> tokens_h;
    DevBuf<uint8_t> tokens_i8;
    DevBuf<float> scales;
    uint64_t n = 0, total = 0;              // records (those without tokens included), token rows
    // the records that have tokens, which are all the kernel sees: their token offsets, their record rows, and the wave ranges
    std::vector<uint64_t> cptr{0};
    std::vector<uint32_t> crec, ranges{0};
    DevBuf<float> tokens;
    DevBuf<uint64_t> d_cptr;
    DevBuf<uint32_t> d_crec, d_ranges;
    // the scratch of a search (it runs under the exclusive lock)
    DevBuf<float> q;
    DevBuf<uint64_t> qdesc, mask, cand_ptr;
    DevBuf<uint32_t> cand;                  // the candidate lists of a rerank, or the live records of a routed filtered search
    std::vector<uint32_t> h_cand;
    ScoreCut cut;
    PoolRerank rr;
    std::vector<float> hq, stage;
    std::vector<uint64_t> hdesc, keys, h_out;
    bool profiling = false;
    lynse_hip_profile prof{};
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};   // the scan begins / the scan ends / the last launch of the chunk
};

// Rule 7 for a query of tq tokens against token rows of `dim` floats, host only: the query tiles the LDS holds (a power of two of
// them: one kernel each), the waves of a workgroup that fit next to them (4, 2 or 1) and the bytes.  Each output may be NULL.
extern "C" int lynse_hip_multivec_plan(uint32_t dim, uint32_t tq, uint32_t* out_tiles, uint32_t* out_waves, uint64_t* out_lds_bytes) {
    if (dim == 0) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "multi-vector dimension must be positive");
    if (tq == 0) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "multi-vector queries: a query needs at least one token");
    if (dim > MAXSIM_MAX_DIM) return set_error(LYNSE_ERR_UNSUPPORTED, "multi-vector search: a token dimension above 1024 is not supported");
    if (tq > MAXSIM_MAX_TQ) return set_error(LYNSE_ERR_UNSUPPORTED, "multi-vector search: a query of more than 256 tokens is not supported");
    const uint32_t ld = maxsim_ld(dim);
    uint32_t tiles = 1, waves = MAXSIM_MAX_WAVES;
    while (tiles * 32u < tq) tiles *= 2;
    while (waves > 1 && maxsim_lds_bytes(ld, tiles, waves) > PoolRerank::LDS_MAX) waves /= 2;
    const size_t lds = maxsim_lds_bytes(ld, tiles, waves);
    if (lds > PoolRerank::LDS_MAX)
        return set_error(LYNSE_ERR_UNSUPPORTED, "multi-vector search: " + std::to_string(tiles) + " query tile(s) and two token blocks of dimension " +
                                                    std::to_string(dim) + " do not fit in LDS");
    if (out_tiles) *out_tiles = tiles;
    if (out_waves) *out_waves = waves;
    if (out_lds_bytes) *out_lds_bytes = lds;
    return LYNSE_OK;
}

// The plan by token dtype (0 = f32: the rule above).  f16 (the addendum): the LDS holds the query tiles as halves and 32 flags per
// wave, no token block, so the waves are always 4 and every dimension up to 1024 serves a query of up to 64 tokens.
extern "C" int lynse_hip_multivec_plan_dtype(uint32_t dim, uint32_t tq, int dtype, uint32_t* out_tiles, uint32_t* out_waves, uint64_t* out_lds_bytes) {
    if (dtype == 0) return lynse_hip_multivec_plan(dim, tq, out_tiles, out_waves, out_lds_bytes);
    if (dtype != 1) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "multi-vector dtype must be 0 (f32) or 1 (f16)");
    if (dim == 0) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "multi-vector dimension must be positive");
    if (tq == 0) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "multi-vector queries: a query needs at least one token");
    if (dim > MAXSIM_MAX_DIM) return set_error(LYNSE_ERR_UNSUPPORTED, "multi-vector search: a token dimension above 1024 is not supported");
    if (tq > MAXSIM_MAX_TQ) return set_error(LYNSE_ERR_UNSUPPORTED, "multi-vector search: a query of more than 256 tokens is not supported");
    uint32_t tiles = 1;
    while (tiles * 32u < tq) tiles *= 2;
    const size_t lds = maxsim_h16_lds_bytes(maxsim_ld(dim), tiles);
    if (lds > PoolRerank::LDS_MAX)
        return set_error(LYNSE_ERR_UNSUPPORTED, "multi-vector search: " + std::to_string(tiles) + " query tile(s) of f16 tokens of dimension " +
                                                    std::to_string(dim) + " do not fit in LDS");
    if (out_tiles) *out_tiles = tiles;
    if (out_waves) *out_waves = MAXSIM_MAX_WAVES;
    if (out_lds_bytes) *out_lds_bytes = lds;
    return LYNSE_OK;
}

// Rule 7" of the int8 store, host only: the LDS holds the query tiles as codes at a row pitch of ld + 16 bytes, their scales and 32
// flags per wave; the waves are always 4 and every dimension up to 1024 serves a query of up to 128 tokens.
extern "C" int lynse_hip_multivec_plan_i8(uint32_t dim, uint32_t tq, uint32_t* out_tiles, uint32_t* out_waves, uint64_t* out_lds_bytes) {
    if (dim == 0) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "multi-vector dimension must be positive");
    if (tq == 0) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "multi-vector queries: a query needs at least one token");
    if (dim > MAXSIM_MAX_DIM) return set_error(LYNSE_ERR_UNSUPPORTED, "multi-vector search: a token dimension above 1024 is not supported");
    if (tq > MAXSIM_MAX_TQ) return set_error(LYNSE_ERR_UNSUPPORTED, "multi-vector search: a query of more than 256 tokens is not supported");
    uint32_t tiles = 1;
    while (tiles * 32u < tq) tiles *= 2;
    const size_t lds = maxsim_i8_lds_bytes(maxsim_ld(dim), tiles);
    if (lds > PoolRerank::LDS_MAX)
        return set_error(LYNSE_ERR_UNSUPPORTED, "multi-vector search: " + std::to_string(tiles) + " query tile(s) of int8 tokens of dimension " +
                                                    std::to_string(dim) + " do not fit in LDS");
    if (out_tiles) *out_tiles = tiles;
    if (out_waves) *out_waves = MAXSIM_MAX_WAVES;
    if (out_lds_bytes) *out_lds_bytes = lds;
    return LYNSE_OK;
}

// the plan by the handle's tag: 0 and 1 are the public dtype ids, 2 is the int8 store
static int maxsim_plan(uint32_t dim, uint32_t tq, int tag, uint32_t* out_tiles, uint32_t* out_waves, uint64_t* out_lds_bytes) {
    if (tag == 2) return lynse_hip_multivec_plan_i8(dim, tq, out_tiles, out_waves, out_lds_bytes);
    return lynse_hip_multivec_plan_dtype(dim, tq, tag, out_tiles, out_waves, out_lds_bytes);
}

static int maxsim_create(int device, uint32_t dim, int dtype, lynse_hip_multivec** out);

extern "C" int lynse_hip_multivec_create(int device, uint32_t dim, lynse_hip_multivec** out) { return lynse_hip_multivec_create_dtype(device, dim, 0, out); }

extern "C" int lynse_hip_multivec_create_dtype(int device, uint32_t dim, int dtype, lynse_hip_multivec** out) {
    if (out) *out = nullptr;
    if (out && dtype != 0 && dtype != 1) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "multi-vector dtype must be 0 (f32) or 1 (f16)");
    return maxsim_create(device, dim, dtype, out);
}

extern "C" int lynse_hip_multivec_create_i8(int device, uint32_t dim, lynse_hip_multivec** out) { return maxsim_create(device, dim, 2, out); }

static int maxsim_create(int device, uint32_t dim, int dtype, lynse_hip_multivec** out) {
    if (!out) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    LY_TRY(maxsim_plan(dim, 1, dtype, nullptr, nullptr, nullptr));   // a store no query could ever be answered from is refused here
    int ndev = 0;
    LY_TRY(lynse_hip_device_count(&ndev));
    if (ndev <= 0) return set_error(LYNSE_ERR_DEVICE, "no HIP device available (this library has no CPU fallback)");
    if (device < 0 || device >= ndev) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "device ordinal out of range");
    LY_HIP(hipSetDevice(device));
    auto* h = new lynse_hip_multivec();
    h->device = device;
    h->dim = dim;
    h->dtype = dtype;
    h->ld = maxsim_ld(dim);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) h->num_cu = prop.multiProcessorCount;
    const hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete h;
        return set_error(LYNSE_ERR_DEVICE, std::string("hipStreamCreate: ") + hipGetErrorString(e));
    }
    *out = h;
    return LYNSE_OK;
}

extern "C" int lynse_hip_multivec_destroy(lynse_hip_multivec* h) {
    if (!h) return LYNSE_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    h->rr.release();
    for (hipEvent_t e : h->ev)
        if (e) (void)hipEventDestroy(e);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return LYNSE_OK;
}

// The wave ranges over the records that have tokens: whole records, closed once they hold MAXSIM_RANGE tokens or the next record
// would take them past it — so a record of MAXSIM_RANGE tokens or more stands alone.
static void maxsim_ranges(const std::vector<uint64_t>& cptr, std::vector<uint32_t>& ranges) {
    const uint32_t m = (uint32_t)(cptr.size() - 1);
    ranges.assign(1, 0u);
    uint64_t held = 0;
    for (uint32_t c = 0; c < m; ++c) {
        const uint64_t t = cptr[c + 1] - cptr[c];
        if (held && held + t > MAXSIM_RANGE) {
            ranges.push_back(c);
            held = 0;
        }
        held += t;
        if (held >= MAXSIM_RANGE) {
            ranges.push_back(c + 1);
            held = 0;
        }
    }
    if (ranges.back() != m) ranges.push_back(m);
}

// n_records records more: record i has counts[i] >= 0 token rows of `dim` floats, all of them consecutive in `tokens`.  The token
// array grows by doubling (its rows are copied on the device); a failed call leaves the store as it was.
// `tokens` are f32, or raw halves for an f16 handle (raw_h16): an f16 handle takes either and stores rule 1's image of them.
static int maxsim_append(lynse_hip_multivec* h, const void* tokens, bool raw_h16, const uint64_t* counts, uint64_t n_records) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    if (raw_h16 && h->dtype != 1) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "multi-vector append_f16 is valid on an f16 handle only");
    if (n_records == 0) return LYNSE_OK;
    if (!counts) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    uint64_t add = 0;
    for (uint64_t i = 0; i < n_records; ++i) add += counts[i];
    if (add && !tokens) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    std::unique_lock<std::shared_mutex> lk(h->rw);
    if (h->n + n_records >= (1ull << 32)) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "multi-vector records: a selection key carries a 32-bit row, n must be below 2^32");
    LY_HIP(hipSetDevice(h->device));
    const uint32_t D = h->dim, ld = h->ld;
    const uint64_t total = h->total + add;
    std::vector<uint64_t> cptr = h->cptr;
    std::vector<uint32_t> crec = h->crec, ranges;
    for (uint64_t i = 0; i < n_records; ++i)
        if (counts[i]) {
            cptr.push_back(cptr.back() + counts[i]);
            crec.push_back((uint32_t)(h->n + i));
        }
    maxsim_ranges(cptr, ranges);
    // A call that fails below leaves the handle answering as before: a grown token block holds the old rows and the new ones land
    // past them; the device tables go up into fresh buffers; everything is swapped in only once nothing can fail any more.
    DevBuf<uint64_t> n_cptr;
    DevBuf<uint32_t> n_crec, n_ranges;
    if (add && h->dtype == 1) {
        if (total > h->tokens_h.cap / ld) {   // grow: the rows held move to the new block
            DevBuf<uint16_t> grown;
            LY_TRY(grown.alloc((size_t)std::max<uint64_t>(total, 2 * h->total) * ld));
            if (h->total) LY_HIP(hipMemcpy(grown.p, h->tokens_h.p, (size_t)h->total * ld * 2, hipMemcpyDeviceToDevice));
            LY_HIP(hipStreamSynchronize(nullptr));
            h->tokens_h = std::move(grown);
        }
        // the rows as given go up once; the device writes them at the store's pitch (k_maxsim_store_h16: conversion, flush, zero columns)
        const size_t esz = raw_h16 ? 2 : 4;
        DevBuf<uint8_t> raw;
        LY_TRY(raw.alloc((size_t)add * D * esz));
        LY_TRY(h2d_done(raw.p, tokens, (size_t)add * D * esz));
        uint16_t* dst = h->tokens_h.p + (size_t)h->total * ld;
        const uint64_t step = (1ull << 30) / ld;   // rows of a launch: its grid stays below 2^22 workgroups
        for (uint64_t r0 = 0; r0 < add; r0 += step) {
            const uint64_t rows = std::min<uint64_t>(step, add - r0);
            const dim3 grid((uint32_t)((rows * ld + 255) / 256));
            if (raw_h16) hipLaunchKernelGGL(k_maxsim_store_h16<uint16_t>, grid, dim3(256), 0, nullptr, reinterpret_cast<const uint16_t*>(raw.p) + (size_t)r0 * D, dst + (size_t)r0 * ld, rows, D, ld);
            else hipLaunchKernelGGL(k_maxsim_store_h16<float>, grid, dim3(256), 0, nullptr, reinterpret_cast<const float*>(raw.p) + (size_t)r0 * D, dst + (size_t)r0 * ld, rows, D, ld);
            LY_HIP(hipGetLastError());
        }
        LY_HIP(hipStreamSynchronize(nullptr));   // (`raw` is freed on return)
    }
    if (add && h->dtype == 2) {
        // both arrays grow together; a fresh pair replaces the held one only once both exist
        if (total > h->tokens_i8.cap / ld || total > h->scales.cap) {
            const uint64_t cap = std::max<uint64_t>(total, 2 * h->total);
            DevBuf<uint8_t> grown;
            DevBuf<float> grown_s;
            LY_TRY(grown.alloc((size_t)cap * ld));
            LY_TRY(grown_s.alloc((size_t)cap));
            if (h->total) {
                LY_HIP(hipMemcpy(grown.p, h->tokens_i8.p, (size_t)h->total * ld, hipMemcpyDeviceToDevice));
                LY_HIP(hipMemcpy(grown_s.p, h->scales.p, (size_t)h->total * 4, hipMemcpyDeviceToDevice));
            }
            LY_HIP(hipStreamSynchronize(nullptr));
            h->tokens_i8 = std::move(grown);
            h->scales = std::move(grown_s);
        }
        // the f32 rows as given go up once; the device quantises them at the store's pitch (k_maxsim_store_i8: rule 1", zero columns)
        DevBuf<float> raw;
        LY_TRY(raw.alloc((size_t)add * D));
        LY_TRY(h2d_done(raw.p, tokens, (size_t)add * D * 4));
        const uint64_t step = (1ull << 30) / ld;   // rows of a launch: its grid stays below 2^26 workgroups
        for (uint64_t r0 = 0; r0 < add; r0 += step) {
            const uint64_t rows = std::min<uint64_t>(step, add - r0);
            hipLaunchKernelGGL(k_maxsim_store_i8, dim3((uint32_t)((rows + 15) / 16)), dim3(256), 0, nullptr, raw.p + (size_t)r0 * D,
                               reinterpret_cast<uint32_t*>(h->tokens_i8.p + (size_t)(h->total + r0) * ld), h->scales.p + h->total + r0, rows, D, ld);
            LY_HIP(hipGetLastError());
        }
        LY_HIP(hipStreamSynchronize(nullptr));   // (`raw` is freed on return)
    }
    if (add && h->dtype == 0) {
        if (total > h->tokens.cap / ld) {   // grow: the rows held move to the new block
            DevBuf<float> grown;
            LY_TRY(grown.alloc((size_t)std::max<uint64_t>(total, 2 * h->total) * ld));
            if (h->total) LY_HIP(hipMemcpy(grown.p, h->tokens.p, (size_t)h->total * ld * 4, hipMemcpyDeviceToDevice));
            LY_HIP(hipStreamSynchronize(nullptr));   // (the copy is ordered on the NULL stream: h2d_done)
            h->tokens = std::move(grown);
        }
        h->stage.assign((size_t)add * ld, 0.0f);   // the rows at the device pitch, zero columns past the dimension
        for (uint64_t t = 0; t < add; ++t) memcpy(h->stage.data() + (size_t)t * ld, static_cast<const float*>(tokens) + (size_t)t * D, (size_t)D * 4);
        LY_TRY(h2d_done(h->tokens.p + (size_t)h->total * ld, h->stage.data(), h->stage.size() * 4));
    }
    if (add) {
        LY_TRY(n_cptr.alloc(cptr.size()));
        LY_TRY(n_crec.alloc(crec.size()));
        LY_TRY(n_ranges.alloc(ranges.size()));
        LY_TRY(h2d_done(n_cptr.p, cptr.data(), cptr.size() * 8));
        LY_TRY(h2d_done(n_crec.p, crec.data(), crec.size() * 4));
        LY_TRY(h2d_done(n_ranges.p, ranges.data(), ranges.size() * 4));
        h->d_cptr = std::move(n_cptr);
        h->d_crec = std::move(n_crec);
        h->d_ranges = std::move(n_ranges);
    }
    h->cptr.swap(cptr);
    h->crec.swap(crec);
    h->ranges.swap(ranges);
    h->total = total;
    h->n += n_records;
    return LYNSE_OK;
}

extern "C" int lynse_hip_multivec_append(lynse_hip_multivec* h, const float* tokens, const uint64_t* counts, uint64_t n_records) {
    return maxsim_append(h, tokens, false, counts, n_records);
}

extern "C" int lynse_hip_multivec_append_f16(lynse_hip_multivec* h, const uint16_t* tokens, const uint64_t* counts, uint64_t n_records) {
    return maxsim_append(h, tokens, true, counts, n_records);
}

extern "C" int lynse_hip_multivec_counts(lynse_hip_multivec* h, uint64_t* out_records, uint64_t* out_tokens, uint64_t* out_ranges) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    std::shared_lock<std::shared_mutex> lk(h->rw);
    if (out_records) *out_records = h->n;
    if (out_tokens) *out_tokens = h->total;
    if (out_ranges) *out_ranges = h->ranges.size() - 1;
    return LYNSE_OK;
}

extern "C" int lynse_hip_multivec_profile_enable(lynse_hip_multivec* h, int on) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    std::unique_lock<std::shared_mutex> lk(h->rw);
    h->profiling = on != 0;
    return LYNSE_OK;
}

extern "C" int lynse_hip_multivec_profile_get(lynse_hip_multivec* h, lynse_hip_profile* out, int reset) {
    if (!h || !out) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    std::unique_lock<std::shared_mutex> lk(h->rw);
    *out = h->prof;
    if (reset) h->prof = lynse_hip_profile{};
    return LYNSE_OK;
}

template <int NT>
static int maxsim_launch(const MaxSimArgs& a, dim3 grid, uint32_t waves, size_t lds, hipStream_t st) {
    LY_TRY(ensure_lds<k_maxsim_scan<NT>>(PoolRerank::LDS_MAX));
    hipLaunchKernelGGL(k_maxsim_scan<NT>, grid, dim3(waves * 64u), lds, st, a);
    LY_HIP(hipGetLastError());
    return LYNSE_OK;
}

template <int NT>
static int maxsim_i8_launch(const MaxSimI8Args& a, dim3 grid, size_t lds, hipStream_t st) {
    LY_TRY(ensure_lds<k_maxsim_i8<NT>>(PoolRerank::LDS_MAX));
    hipLaunchKernelGGL(k_maxsim_i8<NT>, grid, dim3(MAXSIM_MAX_WAVES * 64u), lds, st, a);
    LY_HIP(hipGetLastError());
    return LYNSE_OK;
}

template <int NT>
static int maxsim_h16_launch(const MaxSimH16Args& a, dim3 grid, size_t lds, hipStream_t st) {
    LY_TRY(ensure_lds<k_maxsim_h16<NT>>(PoolRerank::LDS_MAX));
    hipLaunchKernelGGL(k_maxsim_h16<NT>, grid, dim3(MAXSIM_MAX_WAVES * 64u), lds, st, a);
    LY_HIP(hipGetLastError());
    return LYNSE_OK;
}

// The candidate kernels (k_maxsim_cand_h16 / k_maxsim_cand_i8): `waves` waves a workgroup, the LDS of the scan's plan.
template <int NT>
static int maxsim_cand_launch(const MaxSimCandArgs& a, bool i8, dim3 grid, uint32_t waves, size_t lds, hipStream_t st) {
    if (i8) {
        LY_TRY(ensure_lds<k_maxsim_cand_i8<NT>>(PoolRerank::LDS_MAX));
        hipLaunchKernelGGL(k_maxsim_cand_i8<NT>, grid, dim3(waves * 64u), lds, st, a);
    } else {
        LY_TRY(ensure_lds<k_maxsim_cand_h16<NT>>(PoolRerank::LDS_MAX));
        hipLaunchKernelGGL(k_maxsim_cand_h16<NT>, grid, dim3(waves * 64u), lds, st, a);
    }
    LY_HIP(hipGetLastError());
    return LYNSE_OK;
}

// The candidate lists of a call that the candidate kernels serve: compact record numbers (indices into cptr / crec), strictly
// ascending within a list — so a slot order is a record-row order and the tie rule of the shared order holds.
struct MaxSimCand {
    const uint32_t* list;
    const uint64_t* ptr;      // nq + 1 offsets into list; NULL: list[0 .. n_shared) is every query's list (a routed filtered search)
    uint64_t n_shared;
    uint64_t len(uint64_t q) const { return ptr ? ptr[q + 1] - ptr[q] : n_shared; }
};

// Routing of the filtered search (RERANK rule 8): the live records' tokens as a share of the store at or below which the candidate
// kernel answers a filtered search: the largest share measured at which it was at least 1.25x faster than the scan (it was 4.7x on
// int8 and 5.4x on f16 there; larger shares were not measured).  DESIGN.md §31 has the table.  f16 stores are routed too: the two
// kernels accumulate a score block with the operand roles swapped and the order inside an MFMA is the hardware's, but their score
// bits were compared on Gaussian data on the MI355X and agree (same section).
constexpr uint64_t MAXSIM_CAND_SHARE_DEN = 4;

// the checks of a call's queries (rule 7 and the pointers), before the lock and any device work
static int maxsim_check_queries(const float* q_tokens, const uint64_t* q_ptr, uint64_t nq, uint32_t k, const uint64_t* out_rows, const float* out_scores,
                                const uint32_t* out_counts, uint32_t* tq_max) {
    if (!q_tokens || !q_ptr || !out_counts || (k && (!out_rows || !out_scores))) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    if (nq >= (1ull << 32)) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "too many queries");
    if (q_ptr[0] != 0) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "multi-vector queries: q_ptr must start at 0");
    *tq_max = 0;
    for (uint64_t i = 0; i < nq; ++i) {
        if (q_ptr[i + 1] <= q_ptr[i]) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "multi-vector queries: a query needs at least one token");
        if (q_ptr[i + 1] - q_ptr[i] > MAXSIM_MAX_TQ) return set_error(LYNSE_ERR_UNSUPPORTED, "multi-vector search: a query of more than 256 tokens is not supported");
        *tq_max = std::max(*tq_max, (uint32_t)(q_ptr[i + 1] - q_ptr[i]));
    }
    return LYNSE_OK;
}

// The search under the handle's exclusive lock, the queries checked.  cand == NULL: the scan over every record, S[q][record], the
// mask applied where a record ends — unless the mask leaves few enough tokens (rule 8), then its live records become one shared
// candidate list.  With candidate lists: the candidate kernel, S[q][slot] at the pitch of the longest list.  The tail is one:
// the cut (ScoreCut::cut<true>), the order (k_pool_select, or select_pool_keys beyond 16,384 keys), compact numbers back to rows.
static int maxsim_search(lynse_hip_multivec* h, const float* q_tokens, const uint64_t* q_ptr, uint64_t nq, uint32_t tq_max, uint32_t k,
                         const uint64_t* bitset_words, uint64_t n_words, const MaxSimCand* cand, uint64_t* out_rows, float* out_scores,
                         uint32_t* out_counts) {
    LY_HIP(hipSetDevice(h->device));
    const uint64_t m = h->crec.size(), n = h->n;
    const uint32_t D = h->dim, ld = h->ld;
    const bool h16 = h->dtype == 1, i8 = h->dtype == 2;
    const uint64_t mask_words = bitset_words && !cand ? std::min<uint64_t>(n_words, (n + 63) / 64) : 0;
    uint64_t live = m;   // the most records any query of the call can return
    MaxSimCand routed{nullptr, nullptr, 0};
    if (cand) {
        live = 0;
        for (uint64_t i = 0; i < nq; ++i) live = std::max(live, cand->len(i));
    } else if (bitset_words) {
        live = 0;
        uint64_t live_tokens = 0;
        for (uint64_t c = 0; c < m; ++c) {
            const uint64_t r = h->crec[c];
            if ((r >> 6) < mask_words && ((bitset_words[r >> 6] >> (r & 63u)) & 1ull)) live += 1, live_tokens += h->cptr[c + 1] - h->cptr[c];
        }
        if (live && (i8 || h16) && live_tokens * MAXSIM_CAND_SHARE_DEN <= h->total) {
            h->h_cand.clear();
            for (uint64_t c = 0; c < m; ++c) {
                const uint64_t r = h->crec[c];
                if ((r >> 6) < mask_words && ((bitset_words[r >> 6] >> (r & 63u)) & 1ull)) h->h_cand.push_back((uint32_t)c);
            }
            routed = MaxSimCand{h->h_cand.data(), nullptr, live};
            cand = &routed;
        }
    }
    if (m == 0 || k == 0 || live == 0) {
        memset(out_counts, 0, nq * 4);
        return LYNSE_OK;
    }
    const bool masked = mask_words && !cand;
    const uint64_t pitch = cand ? live : m;   // slots of a query in S
    uint32_t tiles = 0, waves = 0;
    uint64_t lds = 0;
    LY_TRY(maxsim_plan(D, tq_max, h->dtype, &tiles, &waves, &lds));
    // workgroups a CU can hold by their LDS (the registers allow one wave per SIMD at 8 tiles, two or three below): the grid's width
    uint32_t wg_per_cu = (uint32_t)std::min<uint64_t>(PoolRerank::LDS_MAX / lds, tiles == 8 ? 1u : 2u * (MAXSIM_MAX_WAVES / waves));
    // (k_maxsim_h16, a workgroup = one wave per SIMD: by registers two waves per SIMD at 1 and 2 tiles, one above — resource_usage.txt)
    // (k_maxsim_i8 likewise: 166 + 16 and 196 + 32 registers at 1 and 2 tiles are two waves per SIMD, 236 + 64 and 256 + 245 above are one)
    if (h16 || i8) wg_per_cu = (uint32_t)std::min<uint64_t>(PoolRerank::LDS_MAX / lds, tiles <= 2 ? 2u : 1u);
    const uint32_t N = (uint32_t)std::min<uint64_t>(k, live);
    const uint64_t qc = ScoreCut::chunk(nq, pitch, N);
    const bool sort_dev = N <= 16384;
    if (sort_dev) {
        LY_TRY(ensure_lds<k_pool_select<256>>(PoolRerank::LDS_MAX));
        LY_TRY(ensure_lds<k_pool_select<1024>>(PoolRerank::LDS_MAX));
    }
    hipStream_t st = h->stream;
    if (masked) LY_TRY(h->mask.reserve((size_t)std::max<uint64_t>(1, mask_words)));
    const uint64_t cand_total = cand ? (cand->ptr ? cand->ptr[nq] : cand->n_shared) : 0;
    if (cand) {
        LY_TRY(h->cand.reserve((size_t)cand_total));
        if (cand->ptr) LY_TRY(h->cand_ptr.reserve((size_t)nq + 1));
    }
    LY_TRY(h->q.reserve((size_t)qc * tiles * 32u * ld));
    LY_TRY(h->qdesc.reserve((size_t)qc * 2));
    LY_TRY(h->rr.keys.reserve((size_t)qc * N));
    LY_TRY(h->rr.pcnt.reserve((size_t)qc));
    if (sort_dev) LY_TRY(h->rr.out.reserve(((size_t)qc * N * 12 + (size_t)qc * 4 + 7) / 8));
    LY_TRY(h->cut.grow(qc, pitch));
    // (the caller's words and lists are queued only once nothing before the first launch can fail and return with a copy pending)
    if (masked) LY_HIP(hipMemcpyAsync(h->mask.p, bitset_words, (size_t)mask_words * 8, hipMemcpyHostToDevice, st));
    if (cand) {
        LY_HIP(hipMemcpyAsync(h->cand.p, cand->list, (size_t)cand_total * 4, hipMemcpyHostToDevice, st));
        if (cand->ptr) LY_HIP(hipMemcpyAsync(h->cand_ptr.p, cand->ptr, (size_t)(nq + 1) * 8, hipMemcpyHostToDevice, st));
    }
    const bool timed = h->profiling;
    if (timed) {
        for (hipEvent_t& e : h->ev)
            if (!e) LY_HIP(hipEventCreate(&e));
        h->prof.searches += 1;
    }
    const uint32_t n_ranges = (uint32_t)(h->ranges.size() - 1);
    auto chunks = [&]() -> int {
    for (uint64_t q0 = 0; q0 < nq; q0 += qc) {
        const uint32_t nqc = (uint32_t)std::min<uint64_t>(qc, nq - q0);
        // the chunk's queries at the device pitch: zero columns past the dimension, zero rows up to whole tiles of 32
        h->hdesc.resize((size_t)nqc * 2);
        size_t floats = 0;
        for (uint32_t i = 0; i < nqc; ++i) {
            const uint32_t tq = (uint32_t)(q_ptr[q0 + i + 1] - q_ptr[q0 + i]);
            h->hdesc[2 * i] = floats;
            h->hdesc[2 * i + 1] = tq;
            floats += (size_t)((tq + 31u) / 32u * 32u) * ld;
        }
        h->hq.assign(floats, 0.0f);
        for (uint32_t i = 0; i < nqc; ++i)
            for (uint64_t t = q_ptr[q0 + i]; t < q_ptr[q0 + i + 1]; ++t)
                memcpy(h->hq.data() + h->hdesc[2 * i] + (size_t)(t - q_ptr[q0 + i]) * ld, q_tokens + (size_t)t * D, (size_t)D * 4);
        LY_HIP(hipMemcpyAsync(h->q.p, h->hq.data(), floats * 4, hipMemcpyHostToDevice, st));
        LY_HIP(hipMemcpyAsync(h->qdesc.p, h->hdesc.data(), h->hdesc.size() * 8, hipMemcpyHostToDevice, st));
        if (timed) LY_HIP(hipEventRecord(h->ev[0], st));
        if (cand) {
            // a wave per (query, candidate): workgroups of up to 4 waves, as many of them a query as fill the part once over the chunk
            const uint32_t cw = (uint32_t)std::min<uint64_t>(MAXSIM_MAX_WAVES, live);
            const uint32_t per_q = std::max<uint32_t>(1u, h->num_cu * wg_per_cu / nqc);
            const dim3 grid((uint32_t)std::min<uint64_t>((live + cw - 1) / cw, per_q), nqc);
            const MaxSimCandArgs ac{i8 ? h->tokens_i8.p : reinterpret_cast<const unsigned char*>(h->tokens_h.p), h->scales.p, ld, h->d_cptr.p, h->cand.p,
                                    cand->ptr ? h->cand_ptr.p + q0 : nullptr, (uint32_t)cand->n_shared, (uint32_t)pitch, h->q.p, h->qdesc.p, h->cut.S.p};
            switch (tiles) {
            case 1: LY_TRY(maxsim_cand_launch<1>(ac, i8, grid, cw, lds, st)); break;
            case 2: LY_TRY(maxsim_cand_launch<2>(ac, i8, grid, cw, lds, st)); break;
            case 4: LY_TRY(maxsim_cand_launch<4>(ac, i8, grid, cw, lds, st)); break;
            default: LY_TRY(maxsim_cand_launch<8>(ac, i8, grid, cw, lds, st)); break;
            }
        } else {
        const MaxSimArgs a{h->tokens.p, ld, h->d_cptr.p, h->d_crec.p, m, h->d_ranges.p, n_ranges, h->q.p, h->qdesc.p,
                           masked ? h->mask.p : nullptr, mask_words, h->cut.S.p};
        const dim3 grid(std::min<uint32_t>((n_ranges + waves - 1) / waves, h->num_cu * wg_per_cu), nqc);
        if (i8) {   // the same tables and queries, the token rows as codes with a scale each
            const MaxSimI8Args ai{{reinterpret_cast<const int8_t*>(h->tokens_i8.p), ld, a.cptr, a.crec, m, a.ranges, n_ranges, a.Q, a.qdesc, a.mask, mask_words, a.S}, h->scales.p};
            switch (tiles) {
            case 1: LY_TRY(maxsim_i8_launch<1>(ai, grid, lds, st)); break;
            case 2: LY_TRY(maxsim_i8_launch<2>(ai, grid, lds, st)); break;
            case 4: LY_TRY(maxsim_i8_launch<4>(ai, grid, lds, st)); break;
            default: LY_TRY(maxsim_i8_launch<8>(ai, grid, lds, st)); break;
            }
        } else if (h16) {   // the same tables and queries, the token rows as halves
            const MaxSimH16Args ah{reinterpret_cast<const _Float16*>(h->tokens_h.p), ld, a.cptr, a.crec, m, a.ranges, n_ranges, a.Q, a.qdesc, a.mask, mask_words, a.S};
            switch (tiles) {
            case 1: LY_TRY(maxsim_h16_launch<1>(ah, grid, lds, st)); break;
            case 2: LY_TRY(maxsim_h16_launch<2>(ah, grid, lds, st)); break;
            case 4: LY_TRY(maxsim_h16_launch<4>(ah, grid, lds, st)); break;
            default: LY_TRY(maxsim_h16_launch<8>(ah, grid, lds, st)); break;
            }
        } else {
            switch (tiles) {
            case 1: LY_TRY(maxsim_launch<1>(a, grid, waves, lds, st)); break;
            case 2: LY_TRY(maxsim_launch<2>(a, grid, waves, lds, st)); break;
            case 4: LY_TRY(maxsim_launch<4>(a, grid, waves, lds, st)); break;
            default: LY_TRY(maxsim_launch<8>(a, grid, waves, lds, st)); break;
            }
        }
        }
        if (timed) {
            LY_HIP(hipEventRecord(h->ev[1], st));
            const uint64_t row_bytes = i8 ? ld + 4 : ld * (h16 ? 2 : 4);
            h->prof.scan_launches += 1;
            h->prof.last_plan = cand ? 1 : 0;
            if (cand) {   // the rows and bytes the candidate kernel read: the listed records' tokens, their list entries and extents
                for (uint32_t i = 0; i < nqc; ++i) {
                    const uint32_t* l = cand->list + (cand->ptr ? cand->ptr[q0 + i] : 0);
                    uint64_t rows = 0;
                    for (uint64_t j = 0; j < cand->len(q0 + i); ++j) rows += h->cptr[l[j] + 1] - h->cptr[l[j]];
                    h->prof.scan_rows += rows;
                    h->prof.scan_bytes += rows * row_bytes + cand->len(q0 + i) * 20;
                }
            } else {
                h->prof.scan_rows += h->total * nqc;
                h->prof.scan_bytes += (h->total * row_bytes + (m + 1) * 8) * nqc;
            }
        }
        // more candidates than N: the radix selection of the N best keys; else every key below RANGE_FAIL (a state that starts done)
        const PqSel sel_n{0ull, 64u, N, 0u, 0u}, sel_all{(uint64_t)(RANGE_FAIL - 1u), 32u, 0u, 1u, 0u};
        bool select = false;
        h->cut.sel0.resize(nqc);
        for (uint32_t i = 0; i < nqc; ++i) {
            const bool sel = (cand ? cand->len(q0 + i) : live) > N;
            h->cut.sel0[i] = sel ? sel_n : sel_all;
            select |= sel;
        }
        LY_TRY(h->cut.cut<true>(nqc, pitch, N, select, h->rr.keys.p, h->rr.pcnt.p, st));
        const size_t o_dist = (size_t)nqc * N * 8, o_cnt = (size_t)nqc * N * 12, o_all = o_cnt + (size_t)nqc * 4;
        if (sort_dev) {   // sorted in LDS (k_pool_select), rows | scores | counts of the chunk back in one copy
            uint32_t p2 = 2;
            while (p2 < N) p2 <<= 1;
            uint8_t* ob = reinterpret_cast<uint8_t*>(h->rr.out.p);
            PoolRerankArgs x{};
            x.pool_cnt = h->rr.pcnt.p;
            x.pool_ld = N;
            x.p2 = p2;
            x.metric = M_IP;
            x.k = N;
            x.out_k = N;
            x.out_rows = h->rr.out.p;
            x.out_dists = reinterpret_cast<float*>(ob + o_dist);
            x.out_counts = reinterpret_cast<uint32_t*>(ob + o_cnt);
            x.keys_out = h->rr.keys.p;
            if (p2 >= 2048) hipLaunchKernelGGL(k_pool_select<1024>, dim3(nqc), dim3(1024), (size_t)p2 * 8, st, x);
            else hipLaunchKernelGGL(k_pool_select<256>, dim3(nqc), dim3(256), (size_t)p2 * 8, st, x);
            LY_HIP(hipGetLastError());
        }
        if (timed) {
            LY_HIP(hipEventRecord(h->ev[2], st));
            LY_HIP(hipEventSynchronize(h->ev[2]));
            float scan_ms = 0.f, all_ms = 0.f;
            LY_HIP(hipEventElapsedTime(&scan_ms, h->ev[0], h->ev[1]));
            LY_HIP(hipEventElapsedTime(&all_ms, h->ev[0], h->ev[2]));
            h->prof.scan_us += (double)scan_ms * 1000.0;
            h->prof.total_us += (double)all_ms * 1000.0;
        }
        // what a query returns: the N best of its own candidates (every query of a scan has `live` of them)
        auto count_of = [&](uint32_t i) { return (uint32_t)std::min<uint64_t>(N, cand ? cand->len(q0 + i) : live); };
        if (sort_dev) {
            h->h_out.resize((o_all + 7) / 8);
            LY_HIP(hipMemcpyAsync(h->h_out.data(), h->rr.out.p, o_all, hipMemcpyDeviceToHost, st));
            LY_TRY(stream_wait(st));
            const uint8_t* hb = reinterpret_cast<const uint8_t*>(h->h_out.data());
            for (uint32_t i = 0; i < nqc; ++i) {   // (k_pool_select padded a shorter result up to N)
                memcpy(out_rows + (q0 + i) * k, hb + (size_t)i * N * 8, (size_t)N * 8);
                memcpy(out_scores + (q0 + i) * k, hb + o_dist + (size_t)i * N * 4, (size_t)N * 4);
                out_counts[q0 + i] = count_of(i);
            }
        } else {   // beyond the 16,384 keys of the LDS sort: sorted on the host
            h->keys.resize((size_t)nqc * N);
            LY_HIP(hipMemcpyAsync(h->keys.data(), h->rr.keys.p, h->keys.size() * 8, hipMemcpyDeviceToHost, st));
            LY_TRY(stream_wait(st));
            for (uint32_t i = 0; i < nqc; ++i)
                out_counts[q0 + i] = select_pool_keys(h->keys.data() + (size_t)i * N, count_of(i), N, N, false, out_rows + (q0 + i) * k, out_scores + (q0 + i) * k);
        }
        // the kernels number the records that have tokens, the candidate kernel the slots of a list of those numbers: back to record
        // rows (ascending with either, so the order of ties holds)
        for (uint32_t i = 0; i < nqc; ++i) {
            const uint32_t* l = cand ? cand->list + (cand->ptr ? cand->ptr[q0 + i] : 0) : nullptr;
            for (uint32_t j = 0; j < out_counts[q0 + i]; ++j) {
                const uint64_t c = out_rows[(q0 + i) * k + j];
                out_rows[(q0 + i) * k + j] = h->crec[(size_t)(l ? l[c] : c)];
            }
        }
    }
    return LYNSE_OK;
    };
    const int rc = chunks();
    if (rc != LYNSE_OK && (masked || cand)) (void)hipStreamSynchronize(st);   // (the copies of the caller's words and lists must not outlive the call)
    return rc;
}

// nq queries, query i with q_ptr[i + 1] - q_ptr[i] token rows of `dim` floats in q_tokens: the best min(k, live) records of each
// by (score descending, record row ascending) at stride k, out_counts[q] entries valid.  Live = has tokens and is in the mask.
extern "C" int lynse_hip_multivec_search_bitset_f32(lynse_hip_multivec* h, const float* q_tokens, const uint64_t* q_ptr, uint64_t nq, uint32_t k,
                                                    const uint64_t* bitset_words, uint64_t n_words, uint64_t* out_rows, float* out_scores,
                                                    uint32_t* out_counts) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    if (nq == 0) return LYNSE_OK;
    uint32_t tq_max = 0;
    LY_TRY(maxsim_check_queries(q_tokens, q_ptr, nq, k, out_rows, out_scores, out_counts, &tq_max));
    std::unique_lock<std::shared_mutex> lk(h->rw);
    return maxsim_search(h, q_tokens, q_ptr, nq, tq_max, k, bitset_words, n_words, nullptr, out_rows, out_scores, out_counts);
}

extern "C" int lynse_hip_multivec_search_f32(lynse_hip_multivec* h, const float* q_tokens, const uint64_t* q_ptr, uint64_t nq, uint32_t k,
                                             uint64_t* out_rows, float* out_scores, uint32_t* out_counts) {
    return lynse_hip_multivec_search_bitset_f32(h, q_tokens, q_ptr, nq, k, nullptr, 0, out_rows, out_scores, out_counts);
}

// MULTI-VECTOR RERANK: query i scored against the records cand_rows[cand_ptr[i] .. cand_ptr[i + 1]) only.  The checks that need no
// store come first (rule 2), then the handle, then the rows against n — all before any device work.
extern "C" int lynse_hip_multivec_rerank_f32(lynse_hip_multivec* h, const float* q_tokens, const uint64_t* q_ptr, uint64_t nq, uint32_t k,
                                             const uint64_t* cand_rows, const uint64_t* cand_ptr, uint64_t* out_rows, float* out_scores,
                                             uint32_t* out_counts) {
    if (nq == 0) return h ? LYNSE_OK : set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    uint32_t tq_max = 0;
    LY_TRY(maxsim_check_queries(q_tokens, q_ptr, nq, k, out_rows, out_scores, out_counts, &tq_max));
    if (!cand_ptr) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    if (cand_ptr[0] != 0) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "multi-vector rerank: cand_ptr must start at 0");
    for (uint64_t i = 0; i < nq; ++i)
        if (cand_ptr[i + 1] < cand_ptr[i]) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "multi-vector rerank: cand_ptr must not descend");
    if (cand_ptr[nq] && !cand_rows) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    for (uint64_t i = 0; i < nq; ++i)
        for (uint64_t j = cand_ptr[i] + 1; j < cand_ptr[i + 1]; ++j)
            if (cand_rows[j] <= cand_rows[j - 1])
                return set_error(LYNSE_ERR_INVALID_ARGUMENT, "multi-vector rerank: the candidate rows of a query must be strictly ascending");
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    std::unique_lock<std::shared_mutex> lk(h->rw);
    for (uint64_t i = 0; i < nq; ++i)
        if (cand_ptr[i + 1] > cand_ptr[i] && cand_rows[cand_ptr[i + 1] - 1] >= h->n)
            return set_error(LYNSE_ERR_INVALID_ARGUMENT, "multi-vector rerank: candidate row " + std::to_string(cand_rows[cand_ptr[i + 1] - 1]) + " is not a record (n = " +
                                                             std::to_string(h->n) + ")");
    LY_TRY(maxsim_plan(h->dim, tq_max, h->dtype, nullptr, nullptr, nullptr));
    if (h->dtype == 0) {
        // an f32 store has no candidate kernel: the scan once per query with the query's candidates as its BitSet — the same
        // results at the scan's cost
        std::vector<uint64_t> words((h->n + 63) / 64 + 1);
        for (uint64_t i = 0; i < nq; ++i) {
            std::fill(words.begin(), words.end(), 0ull);
            for (uint64_t j = cand_ptr[i]; j < cand_ptr[i + 1]; ++j) words[cand_rows[j] >> 6] |= 1ull << (cand_rows[j] & 63u);
            const uint64_t qp[2] = {0, q_ptr[i + 1] - q_ptr[i]};
            LY_TRY(maxsim_search(h, q_tokens + (size_t)q_ptr[i] * h->dim, qp, 1, (uint32_t)qp[1], k, words.data(), words.size(), nullptr,
                                 out_rows + i * k, out_scores + i * k, out_counts + i));
        }
        return LYNSE_OK;
    }
    // records without tokens drop out here: the lists as compact record numbers (a binary search in crec), still ascending
    std::vector<uint32_t> list;
    std::vector<uint64_t> ptr(nq + 1, 0);
    list.reserve((size_t)cand_ptr[nq]);
    for (uint64_t i = 0; i < nq; ++i) {
        for (uint64_t j = cand_ptr[i]; j < cand_ptr[i + 1]; ++j) {
            const auto it = std::lower_bound(h->crec.begin(), h->crec.end(), (uint32_t)cand_rows[j]);
            if (it != h->crec.end() && *it == cand_rows[j]) list.push_back((uint32_t)(it - h->crec.begin()));
        }
        ptr[i + 1] = list.size();
    }
    const MaxSimCand cand{list.data(), ptr.data(), 0};
    return maxsim_search(h, q_tokens, q_ptr, nq, tq_max, k, nullptr, 0, &cand, out_rows, out_scores, out_counts);
}
