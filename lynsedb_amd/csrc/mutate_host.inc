// mutate_host.inc — row mutation of a FLAT handle: lynse_hip_flat_update_rows_f32 (rows rewritten in place), lynse_hip_flat_compact_rows
// (rows dropped in place, the rest renumbered), lynse_hip_flat_gather_rows (rows read by index) and the host-only plan of a compaction,
// lynse_hip_compact_plan.  Included last from lynse_hip.hip (it releases every auxiliary index); kernels in mutate.h.  The ROW MUTATION
// block of include/lynse_hip.h states the contract, DESIGN.md §22 the reasoning.

// Everything derived from the rows goes back to what a handle that has just been given the rows holds: nothing.  The lazy builders
// (finalize_locked, ensure_shadow_locked, ensure_packed_locked, ensure_bpm_locked, ensure_codes_locked, ensure_sq7_locked) then
// recompute it over ALL rows at the next search.  Two things an emptied scratch shard (lynse_hip_top_k_search) does not need and a
// mutated shard does:
//  - the collection statistics (amax, vmax, vmin, cos_degenerate, rows_integer, rows_nonneg) are maxima and flags k_row_stats only ever
//    moves one way: they and their device words start again, and the norms are cleared up to their capacity;
//  - a code set with n = 0 that keeps its min / max table is not a new fit for a builder that merges rows into that table: the four
//    sets are released, so the next build fits, allocates and counts (sq8_fit) as on a fresh handle.
// The auxiliary indexes cover "the first n rows" as they were: released, and so are the derived copies of the approximate search.  Locked by the caller (exclusive); synchronises the stream.
static int reset_derived_locked(lynse_hip_flat* h) {
    hipStream_t st = cur(h).stream;
    h->n_stats = 0; h->n16 = 0; h->n_packed = 0; h->n_bpm = 0;
    for (CodeSet* s : {&h->sq8, &h->sq8a, &h->sq8c, &h->sq7}) s->release();
    h->sq7_fit = 0;   // (never equal to a later sq8_fit: that counter only grows and a built SQ8 set has bumped it)
    h->sq7_strikes.store(0); h->predict_strikes.store(0); h->i8c_strikes.store(0); h->i8c_strikes_l2.store(0); h->i8c_strikes_cos.store(0);
    h->amax = h->vmax = h->vmin = 0.f; h->sv = 1.f; h->cos_degenerate = 0; h->rows_integer = 0; h->rows_nonneg = 0;
    static const uint32_t init[5] = {0u, 0u, 0x7f800000u, 0u, 0u};
    LY_HIP(hipMemcpyAsync(h->d_stats, init, sizeof init, hipMemcpyHostToDevice, st));
    if (h->vn2) LY_HIP(hipMemsetAsync(h->vn2, 0, ((size_t)h->stats_capacity + 256) * sizeof(float), st));
    if (h->vrinv) LY_HIP(hipMemsetAsync(h->vrinv, 0, ((size_t)h->stats_capacity + 256) * sizeof(float), st));
    LY_HIP(hipStreamSynchronize(st));
    coded_release(h);
    hnsw_release(h);
    diskann_release(h);
    approx_release(h);
    return LYNSE_OK;
}

static inline uint64_t shard_row_bytes(const lynse_hip_flat* h) { return is_f16(h) ? (uint64_t)h->ld16 * 2 : (uint64_t)h->ld * 4; }

// ------------------------------------------------------------------------------------------------ the plan of a compaction ----
enum { COMPACT_UNTOUCHED = 0, COMPACT_DIRECT = 1, COMPACT_STAGED = 2 };
struct CompactWindow { uint64_t src, dst, live, path; };   // (four u64: the layout of lynse_hip_compact_plan's out_windows)
struct CompactPlan {
    uint64_t live = 0;
    uint32_t window_rows = 0;
    std::vector<uint64_t> keep;       // ceil(n / 64) words, bits at or beyond n cleared
    std::vector<uint32_t> word_base;  // per word: kept rows before it = the destination of its first kept row
    std::vector<CompactWindow> windows;
};

static uint32_t compact_default_window(uint64_t row_bytes) {
    const uint64_t w = STAGE_BYTES / std::max<uint64_t>(row_bytes, 1) / 64 * 64;
    return (uint32_t)std::max<uint64_t>(64, std::min<uint64_t>(w, 0xffffffc0ull));
}

static int compact_plan(const uint64_t* keep_words, uint64_t n_words, uint64_t n, uint32_t window_rows, uint64_t row_bytes, CompactPlan& p) {
    const uint64_t need = (n + 63) / 64;
    if (n > 0xfffffff0ull) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "row count exceeds the u32 id capacity of one shard");
    if (need && !keep_words) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "keep_words is NULL");
    if (n_words < need) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "keep_words holds fewer than ceil(len / 64) words");
    if (window_rows % 64) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "window_rows must be a multiple of 64 (0 = the default)");
    const uint64_t W = window_rows ? window_rows : compact_default_window(row_bytes);
    p.window_rows = (uint32_t)W;
    p.keep.assign(keep_words, keep_words + need);
    if (n % 64) p.keep[need - 1] &= (1ull << (n % 64)) - 1ull;
    p.word_base.resize(need);
    uint64_t run = 0;
    for (uint64_t w = 0; w < need; ++w) {
        p.word_base[w] = (uint32_t)run;
        run += (uint64_t)__builtin_popcountll(p.keep[w]);
    }
    p.live = run;
    p.windows.clear();
    for (uint64_t s = 0; s < n; s += W) {
        const uint64_t rows = std::min<uint64_t>(W, n - s), w0 = s / 64, w1 = (s + rows + 63) / 64;
        const uint64_t d = p.word_base[w0];
        const uint64_t end = w1 < need ? p.word_base[w1] : p.live;
        const uint64_t live = end - d;
        const uint64_t path = (d == s && live == rows) ? COMPACT_UNTOUCHED : (d + live <= s ? COMPACT_DIRECT : COMPACT_STAGED);
        p.windows.push_back({s, d, live, path});
    }
    return LYNSE_OK;
}

extern "C" int lynse_hip_compact_plan(const uint64_t* keep_words, uint64_t n_words, uint64_t n, uint32_t window_rows, uint64_t row_bytes,
                                      uint64_t* out_live, uint32_t* out_window_rows, uint64_t* out_n_windows, uint32_t* out_word_base,
                                      uint64_t* out_windows) {
    if (!out_live || !out_window_rows || !out_n_windows) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    CompactPlan p;
    LY_TRY(compact_plan(keep_words, n_words, n, window_rows, row_bytes, p));
    *out_live = p.live;
    *out_window_rows = p.window_rows;
    *out_n_windows = p.windows.size();
    if (out_word_base && !p.word_base.empty()) memcpy(out_word_base, p.word_base.data(), p.word_base.size() * 4);
    if (out_windows && !p.windows.empty()) memcpy(out_windows, p.windows.data(), p.windows.size() * sizeof(CompactWindow));
    return LYNSE_OK;
}

// --------------------------------------------------------------------------------------------------------------- compaction ----
template <typename U>
static int launch_compact_window(lynse_hip_flat* h, char* dst, const char* src, uint64_t row_bytes, const uint64_t* d_keep,
                                 const uint32_t* d_base, uint32_t rank0, uint64_t nrows) {
    const uint32_t units = (uint32_t)(row_bytes / sizeof(U));
    const uint64_t total = nrows * units;
    // full occupancy (8 workgroups of 4 waves per CU), two pieces in flight per lane; the rest of the window by the grid's stride
    const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((total + 511) / 512, (uint64_t)h->num_cu * 8));
    hipLaunchKernelGGL(k_compact_rows<U>, dim3(grid), dim3(256), 0, cur(h).stream, reinterpret_cast<U*>(dst), reinterpret_cast<const U*>(src),
                       units, d_keep, d_base, rank0, nrows);
    LY_HIP(hipGetLastError());
    return LYNSE_OK;
}

static int compact_rows_locked(lynse_hip_flat* h, const CompactPlan& p) {
    hipStream_t st = cur(h).stream;
    const uint64_t rb = shard_row_bytes(h);
    if (rb / 4 > 0xffffffffull) return set_error(LYNSE_ERR_UNSUPPORTED, "row too wide to compact");
    char* rows = is_f16(h) ? reinterpret_cast<char*>(h->rows_h) : reinterpret_cast<char*>(h->rows);
    const bool wide = rb % 16 == 0;   // (every pitch this library produces: round_up(dim, 4) floats, round_up(dim, 8) halves)
    uint64_t* d_keep = nullptr;
    uint32_t* d_base = nullptr;
    char* scratch = nullptr;
    auto run = [&]() -> int {
        uint64_t staged_rows = 0;
        for (const CompactWindow& w : p.windows)
            if (w.path == COMPACT_STAGED) staged_rows = std::max(staged_rows, w.live);
        LY_HIP(hipMalloc(&d_keep, p.keep.size() * 8));
        LY_HIP(hipMalloc(&d_base, p.word_base.size() * 4));
        if (staged_rows) LY_HIP(hipMalloc(&scratch, (size_t)(staged_rows * rb)));
        LY_HIP(hipMemcpyAsync(d_keep, p.keep.data(), p.keep.size() * 8, hipMemcpyHostToDevice, st));
        LY_HIP(hipMemcpyAsync(d_base, p.word_base.data(), p.word_base.size() * 4, hipMemcpyHostToDevice, st));
        for (const CompactWindow& w : p.windows) {
            if (w.path == COMPACT_UNTOUCHED || w.live == 0) continue;
            const uint64_t nrows = std::min<uint64_t>(p.window_rows, h->n - w.src);
            const bool staged = w.path == COMPACT_STAGED;
            char* dst = staged ? scratch : rows + (size_t)(w.dst * rb);
            const char* src = rows + (size_t)(w.src * rb);
            if (wide) LY_TRY(launch_compact_window<uint4>(h, dst, src, rb, d_keep + w.src / 64, d_base + w.src / 64, (uint32_t)w.dst, nrows));
            else LY_TRY(launch_compact_window<uint32_t>(h, dst, src, rb, d_keep + w.src / 64, d_base + w.src / 64, (uint32_t)w.dst, nrows));
            // staged: the copy writes rows [dst, dst + live), all below the window's end — every one of them has been read by this
            // launch or an earlier one, and the stream keeps the order
            if (staged) LY_HIP(hipMemcpyAsync(rows + (size_t)(w.dst * rb), scratch, (size_t)(w.live * rb), hipMemcpyDeviceToDevice, st));
        }
        LY_HIP(hipStreamSynchronize(st));
        return LYNSE_OK;
    };
    const int rc = run();
    if (rc != LYNSE_OK) (void)hipStreamSynchronize(st);
    for (void* q : {(void*)d_keep, (void*)d_base, (void*)scratch})
        if (q) (void)hipFree(q);
    return rc;
}

extern "C" int lynse_hip_flat_compact_rows(lynse_hip_flat* h, const uint64_t* keep_words, uint64_t n_words, uint32_t window_rows,
                                           uint64_t* out_len) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    LY_WRITER(h, lk);
    if (h->packed_only) return set_error(LYNSE_ERR_UNSUPPORTED, "compaction of a packed-only handle is not supported");
    if (h->row_stride != 1 || h->row_offset != 0)
        return set_error(LYNSE_ERR_UNSUPPORTED, "compaction renumbers rows: not supported on a row-mapped handle (set_row_map)");
    CompactPlan p;
    LY_TRY(compact_plan(keep_words, n_words, h->n, window_rows, shard_row_bytes(h), p));
    if (p.live != h->n) {   // (nothing deleted: nothing changes, derived state and auxiliary indexes included)
        LY_TRY(use_device(h));
        if (p.live) LY_TRY(compact_rows_locked(h, p));
        h->n = p.live;
        LY_TRY(reset_derived_locked(h));
    }
    if (out_len) *out_len = h->n;
    return LYNSE_OK;
}

// ------------------------------------------------------------------------------------------------------------------ update ----
// the row list on the device, after the host has checked every row against `len` (and, for an update, against the others)
static int upload_row_list(lynse_hip_flat* h, const uint64_t* rows, uint64_t n, bool distinct, uint64_t** d_rows) {
    for (uint64_t i = 0; i < n; ++i)
        if (rows[i] >= h->n) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "row " + std::to_string(rows[i]) + " is out of bounds (len " + std::to_string(h->n) + ")");
    if (distinct) {
        std::vector<uint64_t> s(rows, rows + n);
        std::sort(s.begin(), s.end());
        const auto dup = std::adjacent_find(s.begin(), s.end());
        if (dup != s.end()) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "row " + std::to_string(*dup) + " is named twice in one update");
    }
    LY_TRY(use_device(h));
    LY_HIP(hipMalloc(d_rows, (size_t)n * 8));
    if (hipMemcpyAsync(*d_rows, rows, (size_t)n * 8, hipMemcpyHostToDevice, cur(h).stream) != hipSuccess ||
        hipStreamSynchronize(cur(h).stream) != hipSuccess) {
        (void)hipFree(*d_rows);
        *d_rows = nullptr;
        return set_error(LYNSE_ERR_DEVICE, "host-to-device copy of the row list failed");
    }
    return LYNSE_OK;
}

extern "C" int lynse_hip_flat_update_rows_f32(lynse_hip_flat* h, const uint64_t* rows, const float* data, uint64_t n) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    if (n && (!rows || !data)) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    LY_WRITER(h, lk);
    if (h->packed_only) return set_error(LYNSE_ERR_UNSUPPORTED, "store holds packed rows only: no f32 rows to update");
    if (n == 0) return LYNSE_OK;
    uint64_t* d_rows = nullptr;
    LY_TRY(upload_row_list(h, rows, n, true, &d_rows));   // (nothing has been written when it refuses)
    hipStream_t st = cur(h).stream;
    const uint64_t chunk = std::max<uint64_t>(1, STAGE_BYTES / ((uint64_t)h->dim * 4));
    float* stage = nullptr;
    int rc = hipMalloc(&stage, (size_t)std::min<uint64_t>(chunk, n) * h->dim * 4) == hipSuccess ? LYNSE_OK : set_error(LYNSE_ERR_OUT_OF_MEMORY, "hipMalloc(stage)");
    for (uint64_t r = 0; rc == LYNSE_OK && r < n; r += chunk) {
        const uint64_t nr = std::min<uint64_t>(chunk, n - r);
        if (hipMemcpyAsync(stage, data + r * h->dim, (size_t)nr * h->dim * 4, hipMemcpyHostToDevice, st) != hipSuccess) {
            rc = set_error(LYNSE_ERR_DEVICE, "host-to-device copy failed");
            break;
        }
        const uint32_t pitch = is_f16(h) ? h->ld16 : h->ld;
        const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((nr * pitch + 255) / 256, (uint64_t)h->num_cu * 32));
        if (is_f16(h)) hipLaunchKernelGGL(k_scatter_rows<_Float16>, dim3(grid), dim3(256), 0, st, h->rows_h, pitch, d_rows + r, stage, h->dim, nr);
        else hipLaunchKernelGGL(k_scatter_rows<float>, dim3(grid), dim3(256), 0, st, h->rows, pitch, d_rows + r, stage, h->dim, nr);
        if (hipGetLastError() != hipSuccess) rc = set_error(LYNSE_ERR_DEVICE, "k_scatter_rows launch failed");
        else if (hipStreamSynchronize(st) != hipSuccess) rc = set_error(LYNSE_ERR_DEVICE, "stream sync failed");   // (the stage is reused)
    }
    if (stage) (void)hipFree(stage);
    (void)hipFree(d_rows);
    const int rc2 = reset_derived_locked(h);   // (after a failure too: some rows may have been written)
    return rc != LYNSE_OK ? rc : rc2;
}

// ------------------------------------------------------------------------------------------------------------------ gather ----
extern "C" int lynse_hip_flat_gather_rows(const lynse_hip_flat* hc, const uint64_t* rows, uint64_t n, float* out) {
    auto* h = const_cast<lynse_hip_flat*>(hc);
    if (!h || (n && (!rows || !out))) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    std::unique_lock<std::shared_mutex> lk(h->rw);   // (the discipline of lynse_hip_flat_read_rows)
    if (h->packed_only) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "store holds packed rows only");
    if (n == 0) return LYNSE_OK;
    uint64_t* d_rows = nullptr;
    LY_TRY(upload_row_list(h, rows, n, false, &d_rows));
    hipStream_t st = cur(h).stream;
    const uint64_t chunk = std::max<uint64_t>(1, STAGE_BYTES / ((uint64_t)h->dim * 4));
    float* stage = nullptr;
    int rc = hipMalloc(&stage, (size_t)std::min<uint64_t>(chunk, n) * h->dim * 4) == hipSuccess ? LYNSE_OK : set_error(LYNSE_ERR_OUT_OF_MEMORY, "hipMalloc(stage)");
    for (uint64_t r = 0; rc == LYNSE_OK && r < n; r += chunk) {
        const uint64_t nr = std::min<uint64_t>(chunk, n - r);
        const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((nr * h->dim + 255) / 256, (uint64_t)h->num_cu * 32));
        if (is_f16(h)) hipLaunchKernelGGL(k_gather_rows<_Float16>, dim3(grid), dim3(256), 0, st, stage, h->rows_h, h->ld16, d_rows + r, h->dim, nr);
        else hipLaunchKernelGGL(k_gather_rows<float>, dim3(grid), dim3(256), 0, st, stage, h->rows, h->ld, d_rows + r, h->dim, nr);
        if (hipGetLastError() != hipSuccess) rc = set_error(LYNSE_ERR_DEVICE, "k_gather_rows launch failed");
        else if (hipMemcpyAsync(out + r * h->dim, stage, (size_t)nr * h->dim * 4, hipMemcpyDeviceToHost, st) != hipSuccess)
            rc = set_error(LYNSE_ERR_DEVICE, "device-to-host copy failed");
        else if (hipStreamSynchronize(st) != hipSuccess) rc = set_error(LYNSE_ERR_DEVICE, "stream sync failed");
    }
    if (stage) (void)hipFree(stage);
    (void)hipFree(d_rows);
    return rc;
}
