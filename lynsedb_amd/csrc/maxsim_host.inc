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
    int dtype = 0;                          // the tag of MAXSIM_DTYPES: 0 f32 (k_maxsim_scan), 1 f16 (k_maxsim_h16), 2 int8 codes (internal,
                                            // lynse_hip_multivec_create_i8: k_maxsim_i8), 3 MXFP4 codes (lynse_hip_multivec_create_mxfp4: k_maxsim_mx4)
    DevBuf<uint8_t> tokens;                 // the token rows, ld elements of the dtype each (cap counts bytes)
    DevBuf<uint8_t> scales;                 // int8: one f32 a token row; MXFP4: the E8M0 bytes of its blocks (cap counts bytes)
    uint64_t n = 0, total = 0;              // records (those without tokens included), token rows
    // the records that have tokens, which are all the kernel sees: their token offsets, their record rows, and the wave ranges
    std::vector<uint64_t> cptr{0};
    std::vector<uint32_t> crec, ranges{0};
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

// What the host code knows of a token dtype, by the handle's tag: 0 and 1 are the public dtype ids, 2 is the int8 store, 3 the MXFP4 one.
struct MaxSimDtype {
    uint32_t hb;         // half-bytes of a stored element
    uint32_t (*scale_bytes)(uint32_t ld);   // the bytes a token row has in `scales`; NULL: the dtype has no scales
    bool shrink;         // the waves of a workgroup go 4, 2, 1 until the LDS fits: only the f32 kernel keeps token blocks there
    bool cand;           // the dtype has candidate kernels (k_maxsim_cand_*)
    uint32_t two_tiles;  // the most query tiles at which the kernel's registers still let two of its waves share a SIMD
    const char* what;    // what does not fit, in the refusal of a plan
    size_t (*lds)(uint32_t ld, uint32_t tiles, uint32_t waves);
    // Workgroups a CU holds by the kernels' registers (resource_usage.txt).  k_maxsim_scan: one wave per SIMD at 8 tiles, two or
    // three below.  k_maxsim_h16, k_maxsim_i8 (a workgroup = one wave per SIMD): two waves per SIMD at 1 and 2 tiles, one above;
    // k_maxsim_mx4 (232 registers at 4 tiles, its ring being half the size): two up to 4 tiles.
    size_t row_bytes(uint32_t ld) const { return (size_t)ld * hb / 2; }
    size_t srow_bytes(uint32_t ld) const { return scale_bytes ? scale_bytes(ld) : 0; }
    uint32_t wg_cap(uint32_t tiles, uint32_t waves) const { return shrink ? (tiles == 8 ? 1u : 2u * (MAXSIM_MAX_WAVES / waves)) : (tiles <= two_tiles ? 2u : 1u); }
};
constexpr MaxSimDtype MAXSIM_DTYPES[4] = {
    {8, nullptr, true, false, 0, "and two token blocks", [](uint32_t ld, uint32_t tiles, uint32_t waves) { return maxsim_lds_bytes(ld, tiles, waves); }},
    {4, nullptr, false, true, 2, "of f16 tokens", [](uint32_t ld, uint32_t tiles, uint32_t) { return maxsim_h16_lds_bytes(ld, tiles); }},
    {2, [](uint32_t) { return 4u; }, false, true, 2, "of int8 tokens", [](uint32_t ld, uint32_t tiles, uint32_t) { return maxsim_i8_lds_bytes(ld, tiles); }},
    {1, [](uint32_t ld) { return maxsim_mx4_scale_pitch(ld); }, false, false, 4, "of MXFP4 tokens",
     [](uint32_t ld, uint32_t tiles, uint32_t) { return maxsim_mx4_lds_bytes(ld, tiles); }},
};

struct MaxSimPlan {
    uint32_t tiles, waves;
    uint64_t lds;
    uint32_t wg_per_cu;   // workgroups a CU can hold, by their LDS and by their registers: the grid's width
};

// The plan of a query of tq tokens against token rows of `dim` elements, host only: the query tiles the LDS holds (a power of two of
// them: one kernel each), the waves of a workgroup and the LDS bytes.  f32 (rule 7): the LDS holds the query tiles and two token
// blocks a wave, so the waves are those that fit next to the tiles (4, 2 or 1).  f16 (the addendum): the query tiles as halves and
// 32 flags per wave, no token block, so the waves are always 4 and every dimension up to 1024 serves a query of up to 64 tokens.
// int8 (rule 7"): the query tiles as codes at a row pitch of ld + 16 bytes, their scales and the flags; 4 waves, and every
// dimension up to 1024 serves a query of up to 128 tokens.  MXFP4 (rule 7'''): the query tiles as E4M3 bytes at the same pitch, ld / 32
// scale bytes a query row and the flags; 4 waves, and again every dimension serves 128 query tokens.  `out` may be NULL.
static int maxsim_plan(uint32_t dim, uint32_t tq, int tag, MaxSimPlan* out) {
    if (dim == 0) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "multi-vector dimension must be positive");
    if (tq == 0) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "multi-vector queries: a query needs at least one token");
    if (dim > MAXSIM_MAX_DIM) return set_error(LYNSE_ERR_UNSUPPORTED, "multi-vector search: a token dimension above 1024 is not supported");
    if (tq > MAXSIM_MAX_TQ) return set_error(LYNSE_ERR_UNSUPPORTED, "multi-vector search: a query of more than 256 tokens is not supported");
    const MaxSimDtype& dt = MAXSIM_DTYPES[tag];
    const uint32_t ld = maxsim_ld(dim);
    uint32_t tiles = 1, waves = MAXSIM_MAX_WAVES;
    while (tiles * 32u < tq) tiles *= 2;
    while (dt.shrink && waves > 1 && dt.lds(ld, tiles, waves) > PoolRerank::LDS_MAX) waves /= 2;
    const size_t lds = dt.lds(ld, tiles, waves);
    if (lds > PoolRerank::LDS_MAX)
        return set_error(LYNSE_ERR_UNSUPPORTED, "multi-vector search: " + std::to_string(tiles) + " query tile(s) " + dt.what + " of dimension " +
                                                    std::to_string(dim) + " do not fit in LDS");
    if (out) *out = MaxSimPlan{tiles, waves, lds, (uint32_t)std::min<uint64_t>(PoolRerank::LDS_MAX / lds, dt.wg_cap(tiles, waves))};
    return LYNSE_OK;
}

// the C face of the plan: each output may be NULL
static int maxsim_plan_out(uint32_t dim, uint32_t tq, int tag, uint32_t* out_tiles, uint32_t* out_waves, uint64_t* out_lds_bytes) {
    MaxSimPlan p;
    LY_TRY(maxsim_plan(dim, tq, tag, &p));
    if (out_tiles) *out_tiles = p.tiles;
    if (out_waves) *out_waves = p.waves;
    if (out_lds_bytes) *out_lds_bytes = p.lds;
    return LYNSE_OK;
}

extern "C" int lynse_hip_multivec_plan(uint32_t dim, uint32_t tq, uint32_t* out_tiles, uint32_t* out_waves, uint64_t* out_lds_bytes) {
    return maxsim_plan_out(dim, tq, 0, out_tiles, out_waves, out_lds_bytes);
}

extern "C" int lynse_hip_multivec_plan_dtype(uint32_t dim, uint32_t tq, int dtype, uint32_t* out_tiles, uint32_t* out_waves, uint64_t* out_lds_bytes) {
    if (dtype != 0 && dtype != 1) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "multi-vector dtype must be 0 (f32) or 1 (f16)");
    return maxsim_plan_out(dim, tq, dtype, out_tiles, out_waves, out_lds_bytes);
}

extern "C" int lynse_hip_multivec_plan_i8(uint32_t dim, uint32_t tq, uint32_t* out_tiles, uint32_t* out_waves, uint64_t* out_lds_bytes) {
    return maxsim_plan_out(dim, tq, 2, out_tiles, out_waves, out_lds_bytes);
}

extern "C" int lynse_hip_multivec_plan_mxfp4(uint32_t dim, uint32_t tq, uint32_t* out_tiles, uint32_t* out_waves, uint64_t* out_lds_bytes) {
    return maxsim_plan_out(dim, tq, 3, out_tiles, out_waves, out_lds_bytes);
}

static int maxsim_create(int device, uint32_t dim, int dtype, lynse_hip_multivec** out);

extern "C" int lynse_hip_multivec_create(int device, uint32_t dim, lynse_hip_multivec** out) { return lynse_hip_multivec_create_dtype(device, dim, 0, out); }

extern "C" int lynse_hip_multivec_create_dtype(int device, uint32_t dim, int dtype, lynse_hip_multivec** out) {
    if (out) *out = nullptr;
    if (out && dtype != 0 && dtype != 1) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "multi-vector dtype must be 0 (f32) or 1 (f16)");
    return maxsim_create(device, dim, dtype, out);
}

extern "C" int lynse_hip_multivec_create_i8(int device, uint32_t dim, lynse_hip_multivec** out) { return maxsim_create(device, dim, 2, out); }

extern "C" int lynse_hip_multivec_create_mxfp4(int device, uint32_t dim, lynse_hip_multivec** out) { return maxsim_create(device, dim, 3, out); }

static int maxsim_create(int device, uint32_t dim, int dtype, lynse_hip_multivec** out) {
    if (!out) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    LY_TRY(maxsim_plan(dim, 1, dtype, nullptr));   // a store no query could ever be answered from is refused here
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

// Room for `total` token rows: where the block (or, for a dtype that has them, the scales) is too small, a new one of max(total,
// twice the rows held) rows, the rows held copied on the device.  The new arrays replace the held ones only once every allocation
// exists and the copies are done, so a failed call leaves the store answering as before.
static int maxsim_grow(lynse_hip_multivec* h, uint64_t total) {
    const MaxSimDtype& dt = MAXSIM_DTYPES[h->dtype];
    const size_t rb = dt.row_bytes(h->ld), sb = dt.srow_bytes(h->ld);
    if (total <= h->tokens.cap / rb && (!sb || total <= h->scales.cap / sb)) return LYNSE_OK;
    const uint64_t cap = std::max<uint64_t>(total, 2 * h->total);
    DevBuf<uint8_t> grown, grown_s;
    LY_TRY(grown.alloc((size_t)cap * rb));
    if (sb) LY_TRY(grown_s.alloc((size_t)cap * sb));
    if (h->total) {
        LY_HIP(hipMemcpy(grown.p, h->tokens.p, (size_t)h->total * rb, hipMemcpyDeviceToDevice));
        if (sb) LY_HIP(hipMemcpy(grown_s.p, h->scales.p, (size_t)h->total * sb, hipMemcpyDeviceToDevice));
    }
    LY_HIP(hipStreamSynchronize(nullptr));   // (the copies are ordered on the NULL stream: h2d_done)
    h->tokens = std::move(grown);
    if (sb) h->scales = std::move(grown_s);
    return LYNSE_OK;
}

// n_records records more: record i has counts[i] >= 0 token rows of `dim` floats, all of them consecutive in `tokens`.  The token
// array grows by doubling (maxsim_grow); a failed call leaves the store as it was.
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
    const MaxSimDtype& dt = MAXSIM_DTYPES[h->dtype];
    const uint32_t D = h->dim, ld = h->ld;
    const size_t rb = dt.row_bytes(ld), sb = dt.srow_bytes(ld);
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
    if (add) {
        LY_TRY(maxsim_grow(h, total));
        uint8_t* dst = h->tokens.p + (size_t)h->total * rb;
        if (h->dtype == 0) {   // f32 rows are laid out on the host and go up in one copy
            h->stage.assign((size_t)add * ld, 0.0f);   // the rows at the device pitch, zero columns past the dimension
            for (uint64_t t = 0; t < add; ++t) memcpy(h->stage.data() + (size_t)t * ld, static_cast<const float*>(tokens) + (size_t)t * D, (size_t)D * 4);
            LY_TRY(h2d_done(dst, h->stage.data(), h->stage.size() * 4));
        } else {
            // the rows as given go up once; the device writes them at the store's pitch (k_maxsim_store_h16: conversion, flush, zero
            // columns; k_maxsim_store_i8: rule 1", zero columns; k_maxsim_store_mx4: rule 1''', zero columns)
            const size_t src_rb = (size_t)D * (raw_h16 ? 2 : 4);
            DevBuf<uint8_t> raw;
            LY_TRY(raw.alloc((size_t)add * src_rb));
            LY_TRY(h2d_done(raw.p, tokens, (size_t)add * src_rb));
            // rows of a launch: rows * ld <= 2^30, so k_maxsim_store_h16 (a thread a stored half) has at most 2^22 workgroups and
            // k_maxsim_store_i8 (16 rows a workgroup, ld >= 32) at most 2^21, k_maxsim_store_mx4 (64 blocks of 32 elements) 2^19
            const uint64_t step = (1ull << 30) / ld;
            for (uint64_t r0 = 0; r0 < add; r0 += step) {
                const uint64_t rows = std::min<uint64_t>(step, add - r0);
                const uint8_t* src = raw.p + (size_t)r0 * src_rb;
                uint8_t* out = dst + (size_t)r0 * rb;
                const dim3 grid_h((uint32_t)((rows * ld + 255) / 256));
                uint8_t* out_s = sb ? h->scales.p + (size_t)(h->total + r0) * sb : nullptr;
                if (h->dtype == 3)
                    hipLaunchKernelGGL(k_maxsim_store_mx4, dim3((uint32_t)((rows * (ld / 32u) + 63) / 64)), dim3(256), 0, nullptr, reinterpret_cast<const float*>(src),
                                       reinterpret_cast<uint32_t*>(out), out_s, rows, D, ld);
                else if (h->dtype == 2)
                    hipLaunchKernelGGL(k_maxsim_store_i8, dim3((uint32_t)((rows + 15) / 16)), dim3(256), 0, nullptr, reinterpret_cast<const float*>(src),
                                       reinterpret_cast<uint32_t*>(out), reinterpret_cast<float*>(out_s), rows, D, ld);
                else if (raw_h16)
                    hipLaunchKernelGGL(k_maxsim_store_h16<uint16_t>, grid_h, dim3(256), 0, nullptr, reinterpret_cast<const uint16_t*>(src), reinterpret_cast<uint16_t*>(out), rows, D, ld);
                else
                    hipLaunchKernelGGL(k_maxsim_store_h16<float>, grid_h, dim3(256), 0, nullptr, reinterpret_cast<const float*>(src), reinterpret_cast<uint16_t*>(out), rows, D, ld);
                LY_HIP(hipGetLastError());
            }
            LY_HIP(hipStreamSynchronize(nullptr));   // (`raw` is freed on return)
        }
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

// f(std::integral_constant<int, NT>) for the plan's tiles (1, 2, 4 or 8): a kernel instantiation each
template <typename F>
static int maxsim_by_tiles(uint32_t tiles, F&& f) {
    switch (tiles) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    default: return f(std::integral_constant<int, 8>{});
    }
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
    const MaxSimDtype& dt = MAXSIM_DTYPES[h->dtype];
    const uint64_t mask_words = bitset_words && !cand ? std::min<uint64_t>(n_words, (n + 63) / 64) : 0;
    uint64_t live = m;   // the most records any query of the call can return
    MaxSimCand routed{nullptr, nullptr, 0};
    if (cand) {
        live = 0;
        for (uint64_t i = 0; i < nq; ++i) live = std::max(live, cand->len(i));
    } else if (bitset_words) {
        // the live records as compact numbers and their tokens, then the routing
        uint64_t live_tokens = 0;
        h->h_cand.clear();
        for (uint64_t c = 0; c < m; ++c) {
            const uint64_t r = h->crec[c];
            if ((r >> 6) < mask_words && ((bitset_words[r >> 6] >> (r & 63u)) & 1ull)) h->h_cand.push_back((uint32_t)c), live_tokens += h->cptr[c + 1] - h->cptr[c];
        }
        live = h->h_cand.size();
        if (live && dt.cand && live_tokens * MAXSIM_CAND_SHARE_DEN <= h->total) {
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
    MaxSimPlan plan;
    LY_TRY(maxsim_plan(D, tq_max, h->dtype, &plan));
    const uint32_t tiles = plan.tiles, waves = plan.waves, wg_per_cu = plan.wg_per_cu;
    const size_t lds = plan.lds;
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
        // The scan: a wave per range, `waves` of them a workgroup.  The candidate kernels: a wave per (query, candidate), workgroups of
        // up to 4 waves, as many of them a query as fill the part once over the chunk.  The LDS is the plan's for both.
        const uint32_t cw = (uint32_t)std::min<uint64_t>(MAXSIM_MAX_WAVES, live);
        const uint32_t per_q = std::max<uint32_t>(1u, h->num_cu * wg_per_cu / nqc);
        const dim3 grid(cand ? (uint32_t)std::min<uint64_t>((live + cw - 1) / cw, per_q) : std::min<uint32_t>((n_ranges + waves - 1) / waves, h->num_cu * wg_per_cu), nqc);
        const dim3 block((cand ? cw : waves) * 64u);
        // the scans' arguments are the same tables and queries for every dtype: only the type of a token row differs
        auto scan_args = [&]<typename T>(const T* rows) {
            return MaxSimArgsT<T>{rows, ld, h->d_cptr.p, h->d_crec.p, m, h->d_ranges.p, n_ranges, h->q.p, h->qdesc.p, masked ? h->mask.p : nullptr, mask_words, h->cut.S.p};
        };
        LY_TRY(maxsim_by_tiles(tiles, [&](auto nt) -> int {
            constexpr int NT = decltype(nt)::value;
            if (cand) {
                const MaxSimCandArgs ac{h->tokens.p, reinterpret_cast<const float*>(h->scales.p), ld, h->d_cptr.p, h->cand.p, cand->ptr ? h->cand_ptr.p + q0 : nullptr, (uint32_t)cand->n_shared,
                                        (uint32_t)pitch, h->q.p, h->qdesc.p, h->cut.S.p};
                return h->dtype == 2 ? launch_lds<k_maxsim_cand_i8<NT>>(grid, block, lds, st, ac) : launch_lds<k_maxsim_cand_h16<NT>>(grid, block, lds, st, ac);
            }
            switch (h->dtype) {
            case 0: return launch_lds<k_maxsim_scan<NT>>(grid, block, lds, st, scan_args(reinterpret_cast<const float*>(h->tokens.p)));
            case 1: return launch_lds<k_maxsim_h16<NT>>(grid, block, lds, st, scan_args(reinterpret_cast<const _Float16*>(h->tokens.p)));
            case 2: return launch_lds<k_maxsim_i8<NT>>(grid, block, lds, st, MaxSimI8Args{scan_args(reinterpret_cast<const int8_t*>(h->tokens.p)), reinterpret_cast<const float*>(h->scales.p)});
            default: return launch_lds<k_maxsim_mx4<NT>>(grid, block, lds, st, MaxSimMx4Args{scan_args(h->tokens.p), h->scales.p});
            }
        }));
        if (timed) {
            LY_HIP(hipEventRecord(h->ev[1], st));
            const uint64_t row_bytes = dt.row_bytes(ld) + dt.srow_bytes(ld);
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
    LY_TRY(maxsim_plan(h->dim, tq_max, h->dtype, nullptr));
    if (!MAXSIM_DTYPES[h->dtype].cand) {
        // an f32 or MXFP4 store has no candidate kernel: the scan once per query with the query's candidates as its BitSet — the same
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
