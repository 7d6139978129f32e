// lynse_hip.hip — host side of liblynse_hip.so: handles, HBM layout, stage planning, launches and
// the C ABI declared in include/lynse_hip.h.  gfx950 only; there is no CPU fallback anywhere in
// this file — every compute entry needs a HIP device.
//
// Reference call path replaced:
//   Collection::search / batch_search (engine.rs:4697-4833, :5352-5498)
//     -> VectorStore::search (vector_store.rs:972-1004) -> FlatMmap::search (flat_mmap.rs:824-923)
//     -> exact_flat_search / packed_binary_search (:1173-1230, :1345-1409) -> simd kernels.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>
#include <sched.h>

#include "kernels.h"
#include "scan_qs.h"
#include "scan_qh.h"
#include "ivf.h"
#include "pq.h"
#include "rabitq.h"
#include "polarvec.h"
#include "hnsw.h"
#include "diskann.h"
#include "range.h"
#include "additive.h"
#include "approx.h"
#include "sparse.h"
#include "text.h"
#include "fields.h"
#include "spann.h"
#include "mutate.h"
#include "predict.h"

using namespace lynse;

// ------------------------------------------------------------------------------------ errors ----
static thread_local std::string g_last_error;

static int set_error(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}

#define LY_HIP(expr)                                                                          \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess) {                                                               \
            int _code = (_e == hipErrorOutOfMemory) ? LYNSE_ERR_OUT_OF_MEMORY : LYNSE_ERR_DEVICE; \
            return set_error(_code, std::string(#expr) + ": " + hipGetErrorString(_e));       \
        }                                                                                     \
    } while (0)

#define LY_TRY(expr)                  \
    do {                              \
        int _rc = (expr);             \
        if (_rc != LYNSE_OK) return _rc; \
    } while (0)

// hipMemset on device memory may return before the fill has run (it is ordered on the NULL stream), and the search contexts'
// streams are created hipStreamNonBlocking: they do NOT wait for the null stream.  A kernel on a context stream could therefore
// start before the one-time clears of a fresh workspace had landed — seen as a first search on a new index that came back with
// zero results, once in ~10^5 cases (the arrival counter of k_small_search held garbage).  Every synchronous fill waits here.
static int memset_done(void* p, int v, size_t n) {
    LY_HIP(hipMemset(p, v, n));
    LY_HIP(hipStreamSynchronize(nullptr));
    return LYNSE_OK;
}

// ... and the same for blocking host-to-device copies of set-up data (a pageable source is staged and the DMA may still be in
// flight when hipMemcpy returns; the kernels that read the data run on non-blocking streams)
static int h2d_done(void* dst, const void* src, size_t n) {
    LY_HIP(hipMemcpy(dst, src, n, hipMemcpyHostToDevice));
    LY_HIP(hipStreamSynchronize(nullptr));
    return LYNSE_OK;
}

// The end of a blocking search: hipStreamSynchronize spins on the completion signal for ~100 us and then parks the thread on an
// interrupt (ROCclr) — a batch over 10M rows runs 1.8 ms, so every blocking step paid the wake-up (~20-25 us between k_select_final
// and the next batch's first kernel in the kernel trace).  Poll the stream instead: a tight poll for the first 200 us (the latency-shaped
// searches end inside it), then a poll with sched_yield() between the queries — a thread that has something to enqueue, or another
// blocked reader of the same handle, gets the core (eight blocked readers were eight spinning cores) — for up to
// LYNSE_HIP_SPIN_US in all (default 5 ms: any batch this library answers at the BASELINE sizes), then block as before.
static int stream_wait(hipStream_t st) {
    static const int64_t spin_us = []() { const char* e = env_str("LYNSE_HIP_SPIN_US"); return e ? (int64_t)atoll(e) : (int64_t)5000; }();
    if (spin_us > 0) {
        const auto t0 = std::chrono::steady_clock::now();
        bool polite = false;
        for (uint32_t it = 0;; ++it) {
            const hipError_t q = hipStreamQuery(st);
            if (q == hipSuccess) return LYNSE_OK;
            if (q != hipErrorNotReady) return set_error(LYNSE_ERR_DEVICE, std::string("hipStreamQuery: ") + hipGetErrorString(q));
            if (polite) sched_yield();
            if (polite || (it & 15u) == 15u) {
                const int64_t us = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
                if (us > spin_us) break;
                if (us > 200) polite = true;
            }
        }
    }
    LY_HIP(hipStreamSynchronize(st));
    return LYNSE_OK;
}

extern "C" int lynse_hip_abi_version(void) { return LYNSE_HIP_ABI_VERSION; }

extern "C" size_t lynse_hip_last_error(char* buf, size_t cap) {
    if (buf && cap) {
        size_t n = std::min(cap - 1, g_last_error.size());
        memcpy(buf, g_last_error.data(), n);
        buf[n] = 0;
    }
    return g_last_error.size();
}

extern "C" int lynse_hip_device_count(int* out) {
    if (!out) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "out_count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *out = 0;
        return set_error(LYNSE_ERR_DEVICE, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
    }
    *out = n;
    return LYNSE_OK;
}

// ----------------------------------------------------------------------------------- metrics ----
static std::string lower(const char* s) {
    std::string r(s ? s : "");
    for (auto& c : r) c = (char)tolower((unsigned char)c);
    return r;
}

extern "C" int lynse_hip_metric_from_str(const char* name, int* out) {  // distance/mod.rs:39-63
    if (!name || !out) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    const std::string s = lower(name);
    static const struct { const char* n; int m; } tab[] = {
        {"ip", M_IP}, {"inner_product", M_IP}, {"inner", M_IP}, {"dot", M_IP},
        {"l2", M_L2}, {"l2sq", M_L2}, {"l2_squared", M_L2}, {"euclidean", M_L2},
        {"cosine", M_COS}, {"cos", M_COS}, {"cosine_distance", M_COS},
        {"hamming", M_HAMMING}, {"jaccard", M_JACCARD},
        {"dice", M_DICE}, {"sorensen", M_DICE}, {"sorensen_dice", M_DICE}, {"sorensen-dice", M_DICE},
        {"tanimoto", M_TANIMOTO},
        {"l1", M_L1}, {"manhattan", M_L1}, {"cityblock", M_L1},
        {"chebyshev", M_CHEBYSHEV}, {"chebychev", M_CHEBYSHEV}, {"linf", M_CHEBYSHEV}, {"l_inf", M_CHEBYSHEV}, {"l-infinity", M_CHEBYSHEV},
        {"canberra", M_CANBERRA},
        {"bray_curtis", M_BRAY_CURTIS}, {"bray-curtis", M_BRAY_CURTIS}, {"braycurtis", M_BRAY_CURTIS},
    };
    for (auto& t : tab)
        if (s == t.n) { *out = t.m; return LYNSE_OK; }
    // valid names of the reference's other six metrics (distance/mod.rs:46-60): recognised, but not part of this path
    for (const char* o : {"haversine", "haversine_m", "haversine-m", "geo", "correlation", "pearson", "hellinger", "wasserstein",
                          "wasserstein1d", "wasserstein_1d", "wasserstein-1d", "emd", "jensen_shannon", "jensen-shannon", "jensenshannon", "js"})
        if (s == o)
            return set_error(LYNSE_ERR_UNSUPPORTED, std::string("metric '") + name + "' is a LynseDB metric outside the GPU FLAT / IVF path "
                                                    "(supported: ip, l2, cosine, hamming, jaccard, dice, tanimoto, l1, chebyshev, canberra, bray_curtis)");
    return set_error(LYNSE_ERR_UNKNOWN_METRIC, std::string("Unknown metric: ") + name);
}

extern "C" int lynse_hip_metric_from_index_mode(const char* mode, int* out) {  // distance/mod.rs:67-107
    if (!mode || !out) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    std::string up(mode);
    for (auto& c : up) c = (char)toupper((unsigned char)c);
    std::vector<std::string> tok;
    size_t p = 0;
    while (p <= up.size()) {
        size_t e = up.find('-', p);
        if (e == std::string::npos) e = up.size();
        tok.push_back(up.substr(p, e - p));
        p = e + 1;
    }
    auto has = [&](const char* v) { return std::find(tok.begin(), tok.end(), v) != tok.end(); };
    // the reference's chain order: Jensen-Shannon (outside this path), the additive metrics but L1, the binary metrics, the
    // other metrics outside this path, L1, then l2 / cos / ip
    auto outside = [&]() { return set_error(LYNSE_ERR_UNSUPPORTED, std::string("index mode names a LynseDB metric outside the GPU FLAT / IVF path: ") + mode); };
    if ((has("JENSEN") && has("SHANNON")) || has("JENSENSHANNON") || has("JS")) return outside();
    int m = -1;
    if (has("CHEBYSHEV") || has("CHEBYCHEV") || has("LINF")) m = M_CHEBYSHEV;
    else if (has("CANBERRA")) m = M_CANBERRA;
    else if (has("BRAYCURTIS") || (has("BRAY") && has("CURTIS"))) m = M_BRAY_CURTIS;
    else if (has("TANIMOTO")) m = M_TANIMOTO;
    else if (has("JACCARD")) m = M_JACCARD;
    else if (has("HAMMING")) m = M_HAMMING;
    else if (has("DICE") || has("SORENSEN")) m = M_DICE;
    else {
        for (const char* o : {"HAVERSINE", "GEO", "CORRELATION", "PEARSON", "HELLINGER", "WASSERSTEIN", "WASSERSTEIN1D", "EMD"})
            if (has(o)) return outside();
        if (has("L1") || has("MANHATTAN") || has("CITYBLOCK")) m = M_L1;
        else if (has("L2") || has("L2SQ")) m = M_L2;
        else if (has("COS") || has("COSINE")) m = M_COS;
        else if (has("IP")) m = M_IP;
    }
    if (m < 0) return set_error(LYNSE_ERR_UNKNOWN_METRIC, std::string("Unknown index mode: ") + mode);
    *out = m;
    return LYNSE_OK;
}

extern "C" int lynse_hip_metric_is_ascending(int metric) { return metric_ascending(metric) ? 1 : 0; }
extern "C" int lynse_hip_metric_is_binary(int metric) { return metric_binary(metric) ? 1 : 0; }

static bool metric_valid(int m) { return m >= M_IP && m <= M_BRAY_CURTIS; }   // every id of the header
// ... for the entries the additive metrics (ids 7-10) are not built for: every one but the exact FLAT searches (additive_host.inc)
static int metric_check(int m) {
    if (metric_additive(m))
        return set_error(LYNSE_ERR_UNSUPPORTED, "l1 / chebyshev / canberra / bray_curtis are served by the exact FLAT searches only "
                                                "(lynse_hip_flat_search_f32, its filtered forms and the range search)");
    if (!metric_valid(m)) return set_error(LYNSE_ERR_UNKNOWN_METRIC, "Unknown metric id");
    return LYNSE_OK;
}

// ------------------------------------------------------------------------------------ handle ----
constexpr size_t H_OUT_BYTES = 96 * 1024;  // results up to this size come back through pinned memory (no pageable-copy stalls)

struct Workspace {
    uint32_t qcap = 0, cap = 0, D = 0, W = 0, kcap = 0;
    uint64_t* cand = nullptr;
    uint64_t* candB = nullptr;   // segmented emission: [QCHUNK][SEG_KEYS] keys (ScanArgs::candB)
    uint8_t* segcnt = nullptr;   // [QCHUNK][SEG_MAX] per-segment key counts
    uint32_t *count = nullptr, *overflow = nullptr;
    float *thr = nullptr, *qinv = nullptr, *qn2 = nullptr, *qrinv = nullptr, *marg2 = nullptr;
    float* pred_chk = nullptr;   // predicted plan: the value each query's final cut must reach (I8cPrepArgs::pred_chk)
    double* pred_dbg = nullptr;  // [qcap][2] m_q, v_q of the last predicted chunk (diagnostics)
    _Float16* Q16 = nullptr;
    size_t q16_halves = 0;
    float* Qf = nullptr;
    uint64_t* QW = nullptr;
    uint64_t* QWp = nullptr;  // queries padded to a power-of-two word count (k_scan_binary_rows)
    uint64_t* out_rows = nullptr;
    float* out_dists = nullptr;
    uint32_t* out_counts = nullptr;  // out_counts[QCHUNK] and overflow[QCHUNK] share one allocation: one readback for both
    uint32_t* h_hdr = nullptr;       // pinned host mirror of that pair
    uint8_t* h_out = nullptr;        // pinned staging for small host-API results (rows then dists), H_OUT_BYTES
    unsigned long long* pool_total = nullptr;
    uint32_t* gsync = nullptr;        // hand-over words of the fused sample stage (ScanArgs::gsync)
    int* dyn = nullptr;               // self-tightening scan (ScanArgs::dyn_*): [qcap] tau, [qcap] margin, [qcap][32] partition maxima
    uint64_t* small_part = nullptr;   // k_small_search: [workgroups][SMALL_MAX_Q][SMALL_MAX_K] keys
    uint32_t* small_ticket = nullptr;
    void release() {
        if (h_hdr) (void)hipHostFree(h_hdr);
        if (h_out) (void)hipHostFree(h_out);
        for (void* p : {(void*)cand, (void*)candB, (void*)segcnt, (void*)count, (void*)thr, (void*)qinv, (void*)qn2,
                        (void*)qrinv, (void*)marg2, (void*)Q16, (void*)Qf, (void*)QW, (void*)QWp, (void*)out_rows,
                        (void*)out_dists, (void*)out_counts, (void*)pool_total, (void*)small_part, (void*)small_ticket, (void*)gsync, (void*)dyn, (void*)pred_chk, (void*)pred_dbg})
            if (p) (void)hipFree(p);
        *this = Workspace();
    }
};

struct PqState;   // FLAT-*-PQ quantiser + search scratch (pq_host.inc)
struct RbqState;  // FLAT-*-RABITQ codes + search scratch (rabitq_host.inc)
struct PlvState;  // FLAT-*-POLARVEC<b> codes + search scratch (polarvec_host.inc)
struct RangeState;  // range search scratch (range_host.inc)
struct HnswState;  // HNSW-* graph + search scratch (hnsw_host.inc)
struct DiskannState;  // DISKANN-* graph + search scratch (diskann_host.inc)
struct ApproxState;  // approximate flat search: row sums, norms, sum orders (approx_host.inc)

// One int8 copy of a shard's rows for the certified coarse pass (lynse_hip_flat::sq8 / sq8a / sq8c / sq7) with what the prep kernel needs
// to certify a bound over it.
struct CodeSet {
    int8_t* codes = nullptr;     // cap x ld signed bytes
    uint64_t n = 0, cap = 0;     // rows covered / row capacity
    float *mins = nullptr, *scales = nullptr;   // per column
    uint32_t* mm = nullptr;      // 2 x cols ordered-int min / max
    uint32_t* stats = nullptr;   // 4 words of k_sq8_quantize: [0] max row L1 of the codes, [1] non-finite elements, [2] max row sum of squares, [3] eps2
    uint32_t a1 = 0, a2sq = 0;   // max row L1 / sum of squares of the codes
    float eps2 = 0.0f;           // bound of the max row sum of squared quantisation residuals
    bool finite = false;
    uint32_t cols = 0, ld = 0;   // columns coded / pitch in bytes
    int *sum = nullptr, *sum2 = nullptr;   // per-row sums of the codes and their squares (the plain set only: FLAT-*-SQ8)
    // Column statistics of the stored codes for the predicted first threshold (predict.h; the plain, unit-row and SQ7 sets): the exact
    // 64-bit sums of c_d and c_d^2 over rows [0, colsum_n) on the device, and mu_d / sigma_d^2 formed from them on the host (f64) and
    // uploaded.  colsum_n == n: up to date (code_stats_locked); 0: not collected.
    unsigned long long* colsum = nullptr;  // 2 x cols
    double *mu = nullptr, *var = nullptr;  // cols each
    uint64_t colsum_n = 0;
    std::vector<double> h_mu, h_var;       // host copies (lynse_hip_flat_predict_debug)
    bool ready(uint64_t rows) const { return codes && n == rows; }
    bool stats_ready() const { return codes && mu && colsum_n == n && n != 0; }
    uint64_t hbm_bytes() const { return codes ? cap * ld + (sum ? 2ull * (cap + 256) * 4 : 0ull) : 0ull; }
    void release() {
        for (void* p : {(void*)codes, (void*)mins, (void*)scales, (void*)mm, (void*)stats, (void*)sum, (void*)sum2, (void*)colsum, (void*)mu, (void*)var})
            if (p) (void)hipFree(p);
        codes = nullptr; mins = scales = nullptr; mm = stats = nullptr; sum = sum2 = nullptr;
        colsum = nullptr; mu = var = nullptr; colsum_n = 0;
        n = cap = 0;
    }
};

struct lynse_hip_flat {
    uint32_t dim = 0, ld = 0, words = 0;
    int device = 0;
    int num_cu = 256;
    // Reader / writer discipline (VectorIndex: Send + Sync, Arc<RwLock<Collection>> with inner.read() on the search path,
    // src/python/mod.rs:950, :1187): unfiltered searches hold `rw` SHARED and run concurrently, each on its own search
    // context (workspace + stream + event pool) taken from `ctx`; append / finalize / lazy builds / the subset-filtered
    // paths (they borrow per-handle scratch) hold it EXCLUSIVE and use context 0.  The context of the calling thread is
    // selected by a thread-local slot (cur()), so the helpers below keep reading h->ws / cur(h).stream through it.
    std::shared_mutex rw;
    struct Ctx {
        hipStream_t stream = nullptr;
        Workspace ws;
        std::vector<hipEvent_t> ev_pool;
        // filtered search: row bitmask of the subset + staging for the subset ids — per context, so that masked filtered
        // searches run under the shared lock like unfiltered ones (the gathered-rows strategy swaps handle fields: exclusive)
        uint32_t* d_mask = nullptr;
        uint64_t mask_words = 0;
        uint64_t* d_subset = nullptr;
        uint64_t subset_cap = 0;
    };
    static constexpr int MAX_CTX = 8;
    Ctx ctx[MAX_CTX];
    int n_ctx = 4;                       // LYNSE_HIP_CONTEXTS (1..8): searches in flight per handle
    std::mutex ctx_mu;
    std::condition_variable ctx_cv;
    uint32_t ctx_busy = 0;               // bit s: context s is taken
    std::mutex prof_mu;                  // profile counters are shared by the contexts
    std::atomic<int> inflight{0};        // tickets of lynse_hip_flat_search_submit_* not yet waited for (async_host.inc)

    uint64_t n = 0, capacity = 0;
    float* rows = nullptr;       // capacity x ld f32, row-major (pad columns zero); nullptr for an F16 shard
    // VectorDtype::F16 shards (src/storage/dtype.rs, flat_mmap.rs:187-221) keep their rows as f16 bits ONLY: capacity x ld16
    // halves, pad columns zero — the bytes of an F16 segment file, the source of every exact score (sequential f32 sums over
    // the exactly decoded halves, simd.rs:805-846).  With sv == 1 the coarse-pass shadow rows16 is this very buffer.
    _Float16* rows_h = nullptr;
    bool shadow_alias = false;   // rows16 == rows_h (not separately owned)
    // f16 shadow of the rows for the coarse scan (k_scan_h16): (half)(v * sv16), pitch ld16 halves, built at finalize
    _Float16* rows16 = nullptr;
    uint32_t ld16 = 0;
    uint64_t n16 = 0, cap16 = 0;
    float sv16 = 0.0f;
    uint64_t n_packed = 0, packed_capacity = 0;
    uint64_t* packed = nullptr;  // n x words u64
    bool packed_only = false;

    uint64_t n_stats = 0;        // rows covered by vn2/vrinv/stats
    uint64_t stats_capacity = 0;
    float *vn2 = nullptr, *vrinv = nullptr;
    uint32_t* d_stats = nullptr;  // 5 words, see k_row_stats
    int rows_integer = 0, rows_nonneg = 0;   // every element of the shard is an integer / non-negative (k_row_stats stats[4]; k_prep_queries' exactness rule)
    float amax = 0.f, vmax = 0.f, vmin = 0.f, sv = 1.f;
    int cos_degenerate = 0;

    uint64_t row_stride = 1, row_offset = 0;
    int ip_form = LYNSE_IPFORM_AUTO;
    int no_fused = 0;            // lynse_hip_flat_set_fused_search(h, 0): always the staged pipeline (tests, A/B)
    uint32_t qchunk = 256;       // queries per pipeline pass (QCHUNK); the k-means assignment step widens it on its centroid store:
                                 // thousands of rows per launch against <= cap centroids (k_scan_h16's blockIdx.y)
    int dtype = LYNSE_DTYPE_F32;  // F16: rows hold f16-representable values, distances use the f16 kernels' sequential sums
    uint32_t stage0_rows = 4096, growth = 8, cap = 16384;

    // The int8 copies of the rows (CodeSet above), each built lazily and kept up to date by ensure_codes_locked (sq7: ensure_sq7_locked):
    // sq8:  SQ8 two-pass mode (FLAT-*-SQ8) and the IP / plain-L2 forms of the certified int8 pass: signed codes (code - 128), per-dimension
    //       min / scale, per-row sums; pitch ld8
    // sq8a: the L2 form of the certified int8 pass: codes of the AUGMENTED rows [v, |v|^2] (k_i8c_prep_queries, aug = 1), pitch
    //       ld8a = round_up(dim + 1, 128) (whole 128-column slabs: the non-ragged scan kernels), first L2 batch of 33..256 queries
    // sq8c: the cosine form: codes of the UNIT rows fl(v_d * rinv[row]) (pitch ld8), first cosine batch of 33..256 queries
    // sq7:  the NON-NEGATIVE 7-bit copy of the codes (scale 127 / range, codes [0, 127] stored without the offset; layout and pitch of `sq8`,
    //       whose minima and min / max table it borrows: its own mins / mm stay null) the 129..256-query IP scan streams instead of `sq8` when
    //       rows — and with them, presumably, queries — are non-negative: every MAC of the int8 pipe is then non-negative and the
    //       power-capped scan holds a higher clock.  Follows the SQ8 life cycle; a1 / a2sq are those of the (uncentred) codes.
    CodeSet sq8, sq8a, sq8c, sq7;
    uint32_t ld8 = 0, ld8a = 0, aug_cols = 1;     // aug_cols: columns carrying |v|^2 (a power of two <= 32 that fits the slab padding)
    uint32_t* sq8_mm_prev = nullptr;  // scratch of the incremental append: the min / max table before the new rows were merged + a flag word
    uint64_t sq8_fit = 0;   // counts the fits of the min / max table of `sq8` (a new fit recodes every row: ensure_codes_locked)
    uint64_t sq7_fit = 0;   // the sq8_fit the SQ7 copy was coded under
    std::atomic<int> sq7_strikes{0};       // overflows of the SQ7 scan (each re-answered on the SQ8 codes); 3 switch it off for the handle
    std::atomic<int> predict_strikes{0};   // chunks the predicted first threshold missed or overflowed on (each re-answered on the sampled plan); 3 switch it off until the codes are fitted again
    // overflow strikes of the certified int8 pass, per METRIC (plain-code L2 reads `sq8` but strikes i8c_strikes_l2)
    std::atomic<int> i8c_strikes_l2{0};
    std::atomic<int> i8c_strikes_cos{0};
    // certified int8 coarse pass (FLAT-IP batches of 33..256 queries): -1 = off (env / strikes), else overflow strikes so far
    std::atomic<int> i8c_strikes{0};     // (searches under the SHARED lock bump it)
    // batched Hamming on the matrix pipe: one signed byte per bit (+1 / -1) of the packed rows, pitch ld8; built lazily on the
    // first Hamming batch of >= bin_mfma_minq() queries (4x the packed words: the price of feeding the matrix pipe from HBM)
    uint8_t* bpm = nullptr;              // FP4 nibbles (+1.0 / -1.0 per bit), pitch ld_bpm = round_up(dim, 256) / 2 bytes
    uint32_t ld_bpm = 0;
    uint64_t n_bpm = 0, bpm_cap = 0;
    bool bpm_failed = false;             // the copy did not fit: the popcount kernels answer
    // gathered ("few matches") filtered path: compact copy of the listed shadow rows, their norms and 32-bit ids
    _Float16* g_rows16 = nullptr;
    float *g_vn2 = nullptr, *g_vrinv = nullptr;
    uint32_t* g_ids32 = nullptr;
    uint64_t g_cap = 0;

    PqState* pq = nullptr;                // FLAT-{IP,L2,COS}-PQ index over the first pq->n rows (pq_host.inc); NULL = none
    RbqState* rbq = nullptr;              // FLAT-{IP,L2,COS}-RABITQ index over the first rbq->n rows (rabitq_host.inc); NULL = none
    PlvState* plv = nullptr;              // FLAT-{IP,L2,COS}-POLARVEC<b> index over the first plv->n rows (polarvec_host.inc); NULL = none
    RangeState* range = nullptr;          // scratch of lynse_hip_flat_search_range_f32 (range_host.inc); NULL until the first one
    HnswState* hnsw = nullptr;            // HNSW-{IP,L2,COS} graph over the first hnsw->n rows (hnsw_host.inc); NULL = none
    DiskannState* diskann = nullptr;      // DISKANN-{L2,COS} graph over the first diskann->n rows (diskann_host.inc); NULL = none
    ApproxState* approx = nullptr;        // derived copies of the approximate flat search over approx->n rows (approx_host.inc); NULL = none

    std::atomic<bool> profiling{false};   // (read by searches without the lock: atomics)
    std::atomic<uint32_t> prof_rate{1};              // every prof_rate-th search records its events (lynse_hip_flat_profile_enable(h, n))
    std::atomic<uint32_t> prof_seq{0};
    lynse_hip_profile prof{};
};

static void coded_release(lynse_hip_flat* h);   // pq, rbq and plv (polarvec_host.inc, the last of the three)
static void range_release(lynse_hip_flat* h);
static void hnsw_release(lynse_hip_flat* h);
static void diskann_release(lynse_hip_flat* h);
static void approx_release(lynse_hip_flat* h);

static inline bool is_f16(const lynse_hip_flat* h) { return h->dtype == LYNSE_DTYPE_F16; }
// the row matrix the exact-scoring kernels read: f32 rows, or the f16 bits of an F16 shard handed in as float* with a pitch
// of ld16 / 2 floats (exact_score_f16seq turns the pointer back; LYNSE_IPFORM_F16SEQ goes with it)
static inline const float* score_rows(const lynse_hip_flat* h) { return is_f16(h) ? reinterpret_cast<const float*>(h->rows_h) : h->rows; }
static inline uint32_t score_ld(const lynse_hip_flat* h) { return is_f16(h) ? h->ld16 / 2 : h->ld; }

static thread_local bool tl_prof = false;   // the search running on this thread records profile events (profile_begin_search)
static thread_local int tl_ctx_slot = 0;   // the search context of the calling thread (0 outside a concurrent search)
static inline lynse_hip_flat::Ctx& cur(lynse_hip_flat* h) { return h->ctx[tl_ctx_slot]; }
static inline const lynse_hip_flat::Ctx& cur(const lynse_hip_flat* h) { return h->ctx[tl_ctx_slot]; }

// Takes a free search context for the calling thread (blocks while all n_ctx are busy); context 0's stream is created with
// the handle, the others on first use.
struct CtxLease {
    lynse_hip_flat* h = nullptr;
    int slot = 0, prev = 0;
    int acquire(lynse_hip_flat* hh) {
        h = hh;
        {
            std::unique_lock<std::mutex> lk(h->ctx_mu);
            for (;;) {
                int s = 0;
                while (s < h->n_ctx && ((h->ctx_busy >> s) & 1u)) ++s;
                if (s < h->n_ctx) { slot = s; h->ctx_busy |= 1u << s; break; }
                // every context leased by a TICKET (only a wait() of the caller frees those): an error, not a deadlock
                if (h->inflight.load(std::memory_order_acquire) >= h->n_ctx) {
                    h = nullptr;
                    return set_error(LYNSE_ERR_INVALID_ARGUMENT, "every search context of the handle is held by a ticket: wait for one first (LYNSE_HIP_CONTEXTS)");
                }
                h->ctx_cv.wait(lk);
            }
        }
        prev = tl_ctx_slot;
        tl_ctx_slot = slot;
        if (!h->ctx[slot].stream && hipStreamCreateWithFlags(&h->ctx[slot].stream, hipStreamNonBlocking) != hipSuccess) {
            release();
            return set_error(LYNSE_ERR_DEVICE, "hipStreamCreate failed");
        }
        return LYNSE_OK;
    }
    void release() {
        if (!h) return;
        tl_ctx_slot = prev;
        {
            std::lock_guard<std::mutex> lk(h->ctx_mu);
            h->ctx_busy &= ~(1u << slot);
        }
        h->ctx_cv.notify_one();
        h = nullptr;
    }
    ~CtxLease() { release(); }
};


// Writers — append / finalize / lazy builds / setters / the subset-filtered and large-k searches — hold `rw` EXCLUSIVE and
// refuse to start while tickets of lynse_hip_flat_search_submit_* are outstanding: a ticket does not keep the reader lock
// (it may be waited for by another thread, and one thread may hold several), it is counted in `inflight` under the
// shared lock, so a writer that owns the lock sees every ticket submitted before it.
static int writer_lock(lynse_hip_flat* h, std::unique_lock<std::shared_mutex>& lk) {
    lk = std::unique_lock<std::shared_mutex>(h->rw);
    if (h->inflight.load(std::memory_order_acquire) != 0) {
        lk.unlock();
        return set_error(LYNSE_ERR_INVALID_ARGUMENT, "searches are in flight on this handle: wait for the outstanding tickets first");
    }
    return LYNSE_OK;
}
#define LY_WRITER(h, lk) std::unique_lock<std::shared_mutex> lk; LY_TRY(writer_lock((h), lk))

// decides whether the search starting on this thread is a timed one (profiling on, and its turn at the sampling rate)
static bool profile_begin_search(lynse_hip_flat* h) {
    const uint32_t rate = h->prof_rate.load();
    tl_prof = h->profiling.load() && (rate <= 1 || h->prof_seq.fetch_add(1) % rate == 0);
    return tl_prof;
}

static int use_device(const lynse_hip_flat* h) {
    LY_HIP(hipSetDevice(h->device));
    return LYNSE_OK;
}

static uint32_t round_up(uint32_t x, uint32_t m) { return (x + m - 1) / m * m; }

extern "C" int lynse_hip_flat_create(uint32_t dim, int device, lynse_hip_flat** out) {
    if (!out) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    if (dim == 0) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "dimension must be greater than zero");
    int ndev = 0;
    LY_TRY(lynse_hip_device_count(&ndev));
    if (ndev <= 0) return set_error(LYNSE_ERR_DEVICE, "no HIP device available (this library has no CPU fallback)");
    if (device < 0 || device >= ndev) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "device ordinal out of range");
    LY_HIP(hipSetDevice(device));
    auto* h = new lynse_hip_flat();
    h->dim = dim;
    h->ld = round_up(dim, 4);
    h->ld16 = round_up(dim, 8);
    // 48..63 and 96..127 columns: the f16 rows are padded (zeros) to a whole 64-element slab — at most a third more shadow bytes, and the
    // float batches of such a shard (deep-96, GloVe-100 ...) run the whole-slab kernels: k_scan_qh (scan_qh.h) and the non-ragged
    // k_scan_h16 variants.  LYNSE_HIP_SHADOW_PAD=0: the 8-element pitch (A/B, tests; read when the handle is created)
    if (((dim >= 48 && dim < 64) || (dim >= 96 && dim < 128)) && env_on("LYNSE_HIP_SHADOW_PAD", true))
        h->ld16 = round_up(dim, 64);
    h->ld8 = round_up(dim, 16);
    h->ld_bpm = round_up(dim, 256) / 2;
    h->ld8a = round_up(dim + 1, 128);
    while (h->aug_cols * 2 <= 32 && dim + h->aug_cols * 2 <= h->ld8a) h->aug_cols *= 2;
    h->sq8.cols = h->sq8c.cols = h->sq7.cols = dim;
    h->sq8.ld = h->sq8c.ld = h->sq7.ld = h->ld8;
    h->sq8a.cols = dim + h->aug_cols;
    h->sq8a.ld = h->ld8a;
    h->words = (dim + 63) / 64;
    h->device = device;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
        h->num_cu = prop.multiProcessorCount;
    if (const char* ce = env_str("LYNSE_HIP_CONTEXTS")) h->n_ctx = std::max(1, std::min((int)lynse_hip_flat::MAX_CTX, atoi(ce)));
    hipError_t e = hipStreamCreateWithFlags(&h->ctx[0].stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete h;
        return set_error(LYNSE_ERR_DEVICE, std::string("hipStreamCreate: ") + hipGetErrorString(e));
    }
    e = hipMalloc(&h->d_stats, 5 * sizeof(uint32_t));
    if (e != hipSuccess) {
        (void)hipStreamDestroy(cur(h).stream);
        delete h;
        return set_error(LYNSE_ERR_OUT_OF_MEMORY, "hipMalloc(stats)");
    }
    const uint32_t init[5] = {0u, 0u, 0x7f800000u, 0u, 0u};
    (void)h2d_done(h->d_stats, init, sizeof init);
    *out = h;
    return LYNSE_OK;
}

extern "C" int lynse_hip_flat_destroy(lynse_hip_flat* h) {
    if (!h) return LYNSE_OK;
    (void)hipSetDevice(h->device);
    coded_release(h);
    range_release(h);
    hnsw_release(h);
    diskann_release(h);
    approx_release(h);
    for (auto& c : h->ctx) {
        if (c.stream) (void)hipStreamSynchronize(c.stream);
        c.ws.release();
        if (c.d_mask) (void)hipFree(c.d_mask);
        if (c.d_subset) (void)hipFree(c.d_subset);
        for (auto e : c.ev_pool) (void)hipEventDestroy(e);
    }
    if (h->shadow_alias) h->rows16 = nullptr;
    for (void* p : {(void*)h->rows, (void*)h->rows_h, (void*)h->rows16, (void*)h->packed, (void*)h->vn2, (void*)h->vrinv, (void*)h->d_stats,
                    (void*)h->g_rows16, (void*)h->g_vn2, (void*)h->g_vrinv, (void*)h->g_ids32,
                    (void*)h->bpm, (void*)h->sq8_mm_prev})
        if (p) (void)hipFree(p);
    for (CodeSet* s : {&h->sq8, &h->sq8a, &h->sq8c, &h->sq7}) s->release();
    for (auto& c : h->ctx)
        if (c.stream) (void)hipStreamDestroy(c.stream);
    delete h;
    return LYNSE_OK;
}

static int realloc_rows_h(lynse_hip_flat* h, uint64_t cap) {   // F16 shard: capacity of the f16 row matrix
    _Float16* nr = nullptr;
    LY_HIP(hipMalloc(&nr, (size_t)cap * h->ld16 * sizeof(_Float16) + 256));
    if (h->rows_h && h->n)
        LY_HIP(hipMemcpyAsync(nr, h->rows_h, (size_t)h->n * h->ld16 * sizeof(_Float16), hipMemcpyDeviceToDevice, cur(h).stream));
    LY_HIP(hipStreamSynchronize(cur(h).stream));
    if (h->rows_h) (void)hipFree(h->rows_h);
    h->rows_h = nr;
    h->capacity = cap;
    if (h->shadow_alias) { h->rows16 = h->rows_h; h->cap16 = cap; }
    return LYNSE_OK;
}

static int grow_rows(lynse_hip_flat* h, uint64_t need) {
    if (need <= h->capacity) return LYNSE_OK;
    uint64_t cap = std::max<uint64_t>(need, h->capacity + h->capacity / 2);
    cap = std::max<uint64_t>(cap, 1024);
    if (is_f16(h)) return realloc_rows_h(h, cap);
    float* nr = nullptr;
    LY_HIP(hipMalloc(&nr, (size_t)cap * h->ld * sizeof(float)));
    if (h->rows && h->n)
        LY_HIP(hipMemcpyAsync(nr, h->rows, (size_t)h->n * h->ld * sizeof(float), hipMemcpyDeviceToDevice, cur(h).stream));
    LY_HIP(hipStreamSynchronize(cur(h).stream));
    if (h->rows) (void)hipFree(h->rows);
    h->rows = nr;
    h->capacity = cap;
    return LYNSE_OK;
}

static int grow_packed(lynse_hip_flat* h, uint64_t need) {
    if (need <= h->packed_capacity) return LYNSE_OK;
    uint64_t cap = std::max<uint64_t>(need, h->packed_capacity + h->packed_capacity / 2);
    cap = std::max<uint64_t>(cap, 1024);
    uint64_t* np = nullptr;
    LY_HIP(hipMalloc(&np, (size_t)cap * h->words * sizeof(uint64_t)));
    if (h->packed && h->n_packed)
        LY_HIP(hipMemcpyAsync(np, h->packed, (size_t)h->n_packed * h->words * 8, hipMemcpyDeviceToDevice, cur(h).stream));
    LY_HIP(hipStreamSynchronize(cur(h).stream));
    if (h->packed) (void)hipFree(h->packed);
    h->packed = np;
    h->packed_capacity = cap;
    return LYNSE_OK;
}

extern "C" int lynse_hip_flat_reserve(lynse_hip_flat* h, uint64_t rows) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    LY_WRITER(h, lk);
    LY_TRY(use_device(h));
    if (rows > 0xfffffff0ull) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "row count exceeds the u32 id capacity of one shard");
    if (h->packed_only) return grow_packed(h, rows);
    if (rows > h->capacity && is_f16(h)) return realloc_rows_h(h, rows);
    if (rows > h->capacity) {
        // exact reservation (no 1.5x slack): callers reserve to size a shard to its HBM budget
        float* nr = nullptr;
        LY_HIP(hipMalloc(&nr, (size_t)rows * h->ld * sizeof(float)));
        if (h->rows && h->n)
            LY_HIP(hipMemcpyAsync(nr, h->rows, (size_t)h->n * h->ld * sizeof(float), hipMemcpyDeviceToDevice, cur(h).stream));
        LY_HIP(hipStreamSynchronize(cur(h).stream));
        if (h->rows) (void)hipFree(h->rows);
        h->rows = nr;
        h->capacity = rows;
    }
    return LYNSE_OK;
}

static int copy_rows_kernel(lynse_hip_flat* h, float* dst, uint32_t dp, const float* src, uint32_t sp, uint32_t width,
                            uint64_t n, int zero_pad) {
    const uint64_t total = n * (zero_pad ? dp : width);
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((total + 255) / 256, (uint64_t)h->num_cu * 32);
    hipLaunchKernelGGL(k_copy_rows, dim3(std::max<uint32_t>(blocks, 1)), dim3(256), 0, cur(h).stream, dst, dp, src, sp, width, n, zero_pad);
    LY_HIP(hipGetLastError());
    return LYNSE_OK;
}

// F16 shard: rows [first, first + n) decoded to f32 (exact) into dst (pitch dp floats)
static int decode_rows_kernel(lynse_hip_flat* h, float* dst, uint32_t dp, uint64_t first, uint64_t n) {
    const uint64_t total = n * h->dim;
    hipLaunchKernelGGL(k_f16_to_f32_rows, dim3((uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((total + 255) / 256, (uint64_t)h->num_cu * 32))), dim3(256), 0,
                       cur(h).stream, dst, dp, h->rows_h + (size_t)first * h->ld16, h->ld16, h->dim, n);
    LY_HIP(hipGetLastError());
    return LYNSE_OK;
}

constexpr uint64_t STAGE_BYTES = 64ull << 20;  // dense staging buffer for padded-layout host transfers

static int append_f32_impl(lynse_hip_flat* h, const float* src, uint64_t n, hipMemcpyKind kind) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    if (n == 0) return LYNSE_OK;
    if (!src) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "rows is NULL");
    LY_WRITER(h, lk);
    LY_TRY(use_device(h));
    if (h->packed_only) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "store holds packed rows; cannot append f32 rows");
    if (h->n + n > 0xfffffff0ull) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "row count exceeds the u32 id capacity of one shard");
    LY_TRY(grow_rows(h, h->n + n));
    if (is_f16(h)) {
        // f32 in (host or device) -> f16 bits (RNE): device rows are converted in place, host rows through a staging buffer
        _Float16* dsth = h->rows_h + (size_t)h->n * h->ld16;
        auto convert = [&](const float* d_src, uint64_t nr, uint64_t r) -> int {
            const uint64_t total = nr * h->ld16;
            hipLaunchKernelGGL(k_f32_to_f16_rows, dim3((uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((total + 255) / 256, (uint64_t)h->num_cu * 32))), dim3(256), 0,
                               cur(h).stream, dsth + r * h->ld16, h->ld16, d_src, h->dim, h->dim, nr);
            LY_HIP(hipGetLastError());
            return LYNSE_OK;
        };
        if (kind == hipMemcpyDeviceToDevice) {
            LY_TRY(convert(src, n, 0));
        } else {
            const uint64_t chunk = std::max<uint64_t>(1, STAGE_BYTES / ((uint64_t)h->dim * 4));
            float* stage = nullptr;
            LY_HIP(hipMalloc(&stage, (size_t)std::min<uint64_t>(chunk, n) * h->dim * 4));
            for (uint64_t r = 0; r < n; r += chunk) {
                const uint64_t nr = std::min<uint64_t>(chunk, n - r);
                int rc = hipMemcpyAsync(stage, src + r * h->dim, (size_t)nr * h->dim * 4, kind, cur(h).stream) == hipSuccess ? convert(stage, nr, r)
                                                                                                                       : set_error(LYNSE_ERR_DEVICE, "host-to-device copy failed");
                if (rc == LYNSE_OK && hipStreamSynchronize(cur(h).stream) != hipSuccess) rc = set_error(LYNSE_ERR_DEVICE, "stream sync failed");
                if (rc != LYNSE_OK) { (void)hipFree(stage); return rc; }
            }
            (void)hipFree(stage);
        }
        LY_HIP(hipStreamSynchronize(cur(h).stream));
        h->n += n;
        return LYNSE_OK;
    }
    float* dst = h->rows + (size_t)h->n * h->ld;
    if (h->ld == h->dim) {
        LY_HIP(hipMemcpyAsync(dst, src, (size_t)n * h->dim * sizeof(float), kind, cur(h).stream));
    } else if (kind == hipMemcpyDeviceToDevice) {
        LY_TRY(copy_rows_kernel(h, dst, h->ld, src, h->dim, h->dim, n, 1));
    } else {
        const uint64_t chunk = std::max<uint64_t>(1, STAGE_BYTES / ((uint64_t)h->dim * 4));
        float* stage = nullptr;
        LY_HIP(hipMalloc(&stage, (size_t)std::min<uint64_t>(chunk, n) * h->dim * 4));
        for (uint64_t r = 0; r < n; r += chunk) {
            const uint64_t nr = std::min<uint64_t>(chunk, n - r);
            hipError_t e = hipMemcpyAsync(stage, src + r * h->dim, (size_t)nr * h->dim * 4, kind, cur(h).stream);
            int rc = e == hipSuccess ? copy_rows_kernel(h, dst + r * h->ld, h->ld, stage, h->dim, h->dim, nr, 1)
                                     : set_error(LYNSE_ERR_DEVICE, hipGetErrorString(e));
            if (rc == LYNSE_OK && hipStreamSynchronize(cur(h).stream) != hipSuccess) rc = set_error(LYNSE_ERR_DEVICE, "stream sync failed");
            if (rc != LYNSE_OK) { (void)hipFree(stage); return rc; }
        }
        (void)hipFree(stage);
    }
    LY_HIP(hipStreamSynchronize(cur(h).stream));   // (F16 shards returned above: they keep their rows as f16 bits only)
    h->n += n;
    return LYNSE_OK;
}

extern "C" int lynse_hip_flat_set_dtype(lynse_hip_flat* h, int dtype) {
    if (!h || (dtype != LYNSE_DTYPE_F32 && dtype != LYNSE_DTYPE_F16)) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "bad dtype");
    LY_WRITER(h, lk);
    if (h->n || h->packed_only) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "the dtype is fixed once rows are stored");
    h->dtype = dtype;
    return LYNSE_OK;
}

extern "C" int lynse_hip_flat_append_f16_bits(lynse_hip_flat* h, const uint16_t* rows, uint64_t n) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    if (h->dtype != LYNSE_DTYPE_F16) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "append_f16_bits needs an F16 shard (lynse_hip_flat_set_dtype)");
    if (n == 0) return LYNSE_OK;
    if (!rows) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "rows is NULL");
    // decode on the host in bounded chunks (f16 -> f32 is exact), then the ordinary append
    const uint64_t chunk = std::max<uint64_t>(1, (64ull << 20) / ((uint64_t)h->dim * 4));
    std::vector<float> buf((size_t)std::min<uint64_t>(chunk, n) * h->dim);
    for (uint64_t r = 0; r < n; r += chunk) {
        const uint64_t nr = std::min<uint64_t>(chunk, n - r);
        const _Float16* src = reinterpret_cast<const _Float16*>(rows + r * h->dim);
        for (uint64_t i = 0; i < nr * h->dim; ++i) buf[i] = (float)src[i];
        LY_TRY(append_f32_impl(h, buf.data(), nr, hipMemcpyHostToDevice));
    }
    return LYNSE_OK;
}

extern "C" int lynse_hip_flat_append_f32(lynse_hip_flat* h, const float* rows, uint64_t n) {
    return append_f32_impl(h, rows, n, hipMemcpyHostToDevice);
}
extern "C" int lynse_hip_flat_append_f32_device(lynse_hip_flat* h, const float* d_rows, uint64_t n) {
    return append_f32_impl(h, d_rows, n, hipMemcpyDeviceToDevice);
}

static int append_packed_impl(lynse_hip_flat* h, const uint64_t* src, uint64_t n, hipMemcpyKind kind) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    if (n == 0) return LYNSE_OK;
    if (!src) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "words is NULL");
    LY_WRITER(h, lk);
    LY_TRY(use_device(h));
    if (h->n > 0 && !h->packed_only) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "store holds f32 rows; cannot append packed rows");
    if (h->n + n > 0xfffffff0ull) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "row count exceeds the u32 id capacity of one shard");
    h->packed_only = true;
    LY_TRY(grow_packed(h, h->n + n));
    LY_HIP(hipMemcpyAsync(h->packed + (size_t)h->n * h->words, src, (size_t)n * h->words * 8, kind, cur(h).stream));
    LY_HIP(hipStreamSynchronize(cur(h).stream));
    h->n += n;
    h->n_packed = h->n;
    return LYNSE_OK;
}

extern "C" int lynse_hip_flat_append_packed_u64(lynse_hip_flat* h, const uint64_t* words, uint64_t n) {
    return append_packed_impl(h, words, n, hipMemcpyHostToDevice);
}
extern "C" int lynse_hip_flat_append_packed_u64_device(lynse_hip_flat* h, const uint64_t* d_words, uint64_t n) {
    return append_packed_impl(h, d_words, n, hipMemcpyDeviceToDevice);
}

// Row statistics for rows [n_stats, n): norms + collection stats (locked by caller).
static int ensure_shadow_locked(lynse_hip_flat* h);
static bool shadow_ready(const lynse_hip_flat* h) { return h->packed_only || h->n == 0 || (h->rows16 && h->n16 == h->n && h->sv16 == h->sv); }
constexpr int LY_RESTART_EXCLUSIVE = 10001;   // search_impl_once: the f16 shadow is missing and only a shared lock is held — run again under the writer lock

static int finalize_locked(lynse_hip_flat* h) {
    if (h->packed_only || h->n_stats == h->n) return LYNSE_OK;
    if (h->n > h->stats_capacity) {
        uint64_t cap = std::max<uint64_t>(h->n, h->capacity);
        float *a = nullptr, *b = nullptr;
        // +256: the scan kernel's per-tile norm DMA reads a whole 256-row window
        LY_HIP(hipMalloc(&a, ((size_t)cap + 256) * sizeof(float)));
        LY_HIP(hipMalloc(&b, ((size_t)cap + 256) * sizeof(float)));
        LY_HIP(hipMemsetAsync(a, 0, ((size_t)cap + 256) * sizeof(float), cur(h).stream));
        LY_HIP(hipMemsetAsync(b, 0, ((size_t)cap + 256) * sizeof(float), cur(h).stream));
        if (h->n_stats) {
            LY_HIP(hipMemcpyAsync(a, h->vn2, (size_t)h->n_stats * 4, hipMemcpyDeviceToDevice, cur(h).stream));
            LY_HIP(hipMemcpyAsync(b, h->vrinv, (size_t)h->n_stats * 4, hipMemcpyDeviceToDevice, cur(h).stream));
            LY_HIP(hipStreamSynchronize(cur(h).stream));
        }
        if (h->vn2) (void)hipFree(h->vn2);
        if (h->vrinv) (void)hipFree(h->vrinv);
        h->vn2 = a;
        h->vrinv = b;
        h->stats_capacity = cap;
    }
    const uint64_t nnew = h->n - h->n_stats;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((nnew + 3) / 4, (uint64_t)h->num_cu * 16);
    if (is_f16(h))
        hipLaunchKernelGGL(k_row_stats<_Float16>, dim3(blocks), dim3(256), 0, cur(h).stream, h->rows_h, h->ld16, h->dim,
                           (uint32_t)h->n_stats, (uint32_t)h->n, h->vn2, h->vrinv, h->d_stats);
    else
        hipLaunchKernelGGL(k_row_stats<float>, dim3(blocks), dim3(256), 0, cur(h).stream, h->rows, h->ld, h->dim,
                           (uint32_t)h->n_stats, (uint32_t)h->n, h->vn2, h->vrinv, h->d_stats);
    LY_HIP(hipGetLastError());
    uint32_t st[5];
    LY_HIP(hipMemcpyAsync(st, h->d_stats, sizeof st, hipMemcpyDeviceToHost, cur(h).stream));
    LY_HIP(hipStreamSynchronize(cur(h).stream));
    float f[3];
    memcpy(f, st, sizeof f);
    h->amax = f[0];
    h->vmax = std::sqrt(f[1]);
    h->vmin = (st[2] == 0x7f800000u) ? 0.0f : std::sqrt(f[2]);
    h->cos_degenerate = st[3] ? 1 : 0;
    h->rows_integer = ((st[4] & 1u) == 0u && env_str("LYNSE_HIP_NO_EXACT_INT") == nullptr) ? 1 : 0;
    h->rows_nonneg = (st[4] & 2u) == 0u ? 1 : 0;
    int e = (h->amax > 0.0f && std::isfinite(h->amax)) ? std::ilogb(h->amax) : 13;
    e = std::max(-100, std::min(100, e));
    // no scaling when max|v| in [2^-6, 2^15): the f16 subnormal floor (2^-25 absolute) is then far
    // below u*|v| for every element that matters, and the hot loop saves the multiply
    h->sv = (e >= -6 && e <= 14) ? 1.0f : std::ldexp(1.0f, 13 - e);
    h->n_stats = h->n;
    // (the f16 shadow is a LAZY copy since round 4 — ensure_shadow_locked, built by the first search that runs the f16 coarse pass: a
    // shard whose batches all take the certified int8 pass never pays its 2 B per element: 10M x 768 = 15.4 GB of the 53.9 GB)
    return LYNSE_OK;
}

extern "C" int lynse_hip_flat_finalize(lynse_hip_flat* h) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    LY_WRITER(h, lk);
    LY_TRY(use_device(h));
    return finalize_locked(h);
}

// ensure_binary (flat_mmap.rs:388-401): lazily pack f32 rows [n_packed, n).
static int ensure_packed_locked(lynse_hip_flat* h) {
    if (h->packed_only || h->n_packed == h->n) return LYNSE_OK;
    LY_TRY(grow_packed(h, std::max<uint64_t>(h->n, h->capacity)));
    const uint64_t nnew = h->n - h->n_packed;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((nnew + 3) / 4, (uint64_t)h->num_cu * 16);
    if (is_f16(h))
        hipLaunchKernelGGL(k_pack_bits<_Float16>, dim3(blocks), dim3(256), 0, cur(h).stream,
                           h->rows_h + (size_t)h->n_packed * h->ld16, h->ld16, h->dim, (uint32_t)nnew,
                           h->packed + (size_t)h->n_packed * h->words, h->words);
    else
        hipLaunchKernelGGL(k_pack_bits<float>, dim3(blocks), dim3(256), 0, cur(h).stream,
                           h->rows + (size_t)h->n_packed * h->ld, h->ld, h->dim, (uint32_t)nnew,
                           h->packed + (size_t)h->n_packed * h->words, h->words);
    LY_HIP(hipGetLastError());
    LY_HIP(hipStreamSynchronize(cur(h).stream));
    h->n_packed = h->n;
    return LYNSE_OK;
}

// Batched Hamming on the int8 MFMA (kernels.h, k_bits_to_pm1): batches of at least LYNSE_HIP_BIN_MFMA_MINQ (default 72)
// queries, unfiltered, Hamming only (Jaccard / Dice need the row popcounts in the score: the popcount kernels keep them).
static uint32_t bin_mfma_minq() {
    static const uint32_t v = (uint32_t)env_int("LYNSE_HIP_BIN_MFMA_MINQ", 72);
    return v;   // (the MFMA pass costs the same for 33 or 256 queries — 1.9 ms at 12.5M x 1024 bits —, the popcount kernel ~27 us per query: they cross near 70)
}
static bool bin_mfma_eligible(const lynse_hip_flat* h, int metric, bool filtered, uint64_t nq) {
    return metric == M_HAMMING && !filtered && bin_mfma_minq() > 0 && nq >= bin_mfma_minq() && nq > SCAN_BQ_SMALL && !h->bpm_failed &&
           h->n >= 65536;
}
static int ensure_bpm_locked(lynse_hip_flat* h) {
    if (h->bpm_failed || (h->bpm && h->n_bpm == h->n)) return LYNSE_OK;
    LY_TRY(ensure_packed_locked(h));
    if (h->bpm_cap < h->n) {
        const uint64_t cap = std::max<uint64_t>(h->n, std::max<uint64_t>(h->capacity, h->packed_capacity));
        uint8_t* nb = nullptr;
        if (hipMalloc(&nb, (size_t)cap * h->ld_bpm + 256) != hipSuccess) {  // no room for the 4x copy: not an error
            (void)hipGetLastError();
            h->bpm_failed = true;
            return LYNSE_OK;
        }
        if (h->bpm && h->n_bpm)
            LY_HIP(hipMemcpyAsync(nb, h->bpm, (size_t)h->n_bpm * h->ld_bpm, hipMemcpyDeviceToDevice, cur(h).stream));
        LY_HIP(hipStreamSynchronize(cur(h).stream));
        if (h->bpm) (void)hipFree(h->bpm);
        h->bpm = nb;
        h->bpm_cap = cap;
    }
    const uint64_t pieces = (h->n - h->n_bpm) * (h->ld_bpm / 16);
    hipLaunchKernelGGL(k_bits_to_fp4, dim3((uint32_t)std::min<uint64_t>((pieces + 255) / 256, (uint64_t)h->num_cu * 32)), dim3(256), 0, cur(h).stream,
                       h->packed, h->words, h->dim, h->n_bpm, h->n, h->bpm, h->ld_bpm);
    LY_HIP(hipGetLastError());
    LY_HIP(hipStreamSynchronize(cur(h).stream));
    h->n_bpm = h->n;
    return LYNSE_OK;
}

extern "C" int lynse_hip_flat_set_row_map(lynse_hip_flat* h, uint64_t stride, uint64_t offset) {
    if (!h || stride == 0) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "bad row map");
    LY_WRITER(h, lk);
    h->row_stride = stride;
    h->row_offset = offset;
    return LYNSE_OK;
}

extern "C" int lynse_hip_flat_set_ip_form(lynse_hip_flat* h, int f) {
    if (!h || f < LYNSE_IPFORM_AUTO || f > LYNSE_IPFORM_BATCH8) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "bad ip form");
    LY_WRITER(h, lk);
    h->ip_form = f;
    return LYNSE_OK;
}

extern "C" int lynse_hip_flat_set_fused_search(lynse_hip_flat* h, int on) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    LY_WRITER(h, lk);
    h->no_fused = on ? 0 : 1;
    return LYNSE_OK;
}

extern "C" int lynse_hip_flat_set_plan(lynse_hip_flat* h, uint32_t stage0_rows, uint32_t growth, uint32_t cap) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    if (cap < 256 || cap > 16384 || (cap & (cap - 1))) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "cap must be a power of two in [256,16384]");
    if (stage0_rows == 0 || stage0_rows > cap || growth < 2) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "bad stage plan");
    LY_WRITER(h, lk);
    (void)hipSetDevice(h->device);
    if (cap != h->cap)
        for (auto& c : h->ctx) c.ws.release();
    h->stage0_rows = stage0_rows;
    h->growth = growth;
    h->cap = cap;
    return LYNSE_OK;
}

extern "C" uint64_t lynse_hip_flat_len(const lynse_hip_flat* h) { return h ? h->n : 0; }
extern "C" uint32_t lynse_hip_flat_dim(const lynse_hip_flat* h) { return h ? h->dim : 0; }
extern "C" int lynse_hip_flat_device(const lynse_hip_flat* h) { return h ? h->device : -1; }

extern "C" int lynse_hip_flat_read_rows(const lynse_hip_flat* hc, uint64_t first, uint64_t n, float* out) {
    auto* h = const_cast<lynse_hip_flat*>(hc);
    if (!h || (!out && n)) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    std::unique_lock<std::shared_mutex> lk(h->rw);
    LY_TRY(use_device(h));
    if (h->packed_only) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "store holds packed rows only");
    if (first + n > h->n) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "row range out of bounds");
    if (n == 0) return LYNSE_OK;
    if (!is_f16(h) && h->ld == h->dim) {
        LY_HIP(hipMemcpyAsync(out, h->rows + (size_t)first * h->ld, (size_t)n * h->dim * 4, hipMemcpyDeviceToHost, cur(h).stream));
        LY_HIP(hipStreamSynchronize(cur(h).stream));
        return LYNSE_OK;
    }
    const uint64_t chunk = std::max<uint64_t>(1, STAGE_BYTES / ((uint64_t)h->dim * 4));
    float* stage = nullptr;
    LY_HIP(hipMalloc(&stage, (size_t)std::min<uint64_t>(chunk, n) * h->dim * 4));
    for (uint64_t r = 0; r < n; r += chunk) {
        const uint64_t nr = std::min<uint64_t>(chunk, n - r);
        int rc = is_f16(h) ? decode_rows_kernel(h, stage, h->dim, first + r, nr)
                           : copy_rows_kernel(h, stage, h->dim, h->rows + (size_t)(first + r) * h->ld, h->ld, h->dim, nr, 0);
        if (rc == LYNSE_OK && hipMemcpyAsync(out + r * h->dim, stage, (size_t)nr * h->dim * 4, hipMemcpyDeviceToHost, cur(h).stream) != hipSuccess)
            rc = set_error(LYNSE_ERR_DEVICE, "device-to-host copy failed");
        if (rc == LYNSE_OK && hipStreamSynchronize(cur(h).stream) != hipSuccess) rc = set_error(LYNSE_ERR_DEVICE, "stream sync failed");
        if (rc != LYNSE_OK) { (void)hipFree(stage); return rc; }
    }
    (void)hipFree(stage);
    return LYNSE_OK;
}

extern "C" int lynse_hip_flat_copy_rows_device(const lynse_hip_flat* hc, uint64_t first, uint64_t n, float* d_out) {
    auto* h = const_cast<lynse_hip_flat*>(hc);
    if (!h || (!d_out && n)) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    std::unique_lock<std::shared_mutex> lk(h->rw);
    LY_TRY(use_device(h));
    if (h->packed_only) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "store holds packed rows only");
    if (first + n > h->n) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "row range out of bounds");
    if (n == 0) return LYNSE_OK;
    if (is_f16(h))
        LY_TRY(decode_rows_kernel(h, d_out, h->dim, first, n));
    else if (h->ld == h->dim)
        LY_HIP(hipMemcpyAsync(d_out, h->rows + (size_t)first * h->ld, (size_t)n * h->dim * 4, hipMemcpyDeviceToDevice, cur(h).stream));
    else
        LY_TRY(copy_rows_kernel(h, d_out, h->dim, h->rows + (size_t)first * h->ld, h->ld, h->dim, n, 0));
    LY_HIP(hipStreamSynchronize(cur(h).stream));
    return LYNSE_OK;
}

extern "C" int lynse_hip_flat_read_packed(lynse_hip_flat* h, uint64_t first, uint64_t n, uint64_t* out) {
    if (!h || (!out && n)) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    LY_WRITER(h, lk);
    LY_TRY(use_device(h));
    if (first + n > h->n) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "row range out of bounds");
    LY_TRY(ensure_packed_locked(h));
    if (n == 0) return LYNSE_OK;
    LY_HIP(hipMemcpyAsync(out, h->packed + (size_t)first * h->words, (size_t)n * h->words * 8, hipMemcpyDeviceToHost, cur(h).stream));
    LY_HIP(hipStreamSynchronize(cur(h).stream));
    return LYNSE_OK;
}

// ---------------------------------------------------------------------------------- profiling ----
extern "C" int lynse_hip_flat_profile_enable(lynse_hip_flat* h, int on) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    std::unique_lock<std::shared_mutex> lk(h->rw);
    h->profiling = on != 0;
    h->prof_rate = on > 1 ? (uint32_t)on : 1u;   // on = n > 1: every n-th search is timed (HIP events between the kernels cost a few us each)
    h->prof_seq.store(0);
    return LYNSE_OK;
}

extern "C" int lynse_hip_flat_profile_get(lynse_hip_flat* h, lynse_hip_profile* out, int reset) {
    if (!h || !out) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    std::unique_lock<std::shared_mutex> lk(h->rw);
    LY_TRY(use_device(h));
    unsigned long long pool_sum = 0;
    for (auto& c : h->ctx) {  // every search context counts its own rescored candidates
        if (!c.ws.pool_total) continue;
        unsigned long long pool = 0;
        LY_HIP(hipStreamSynchronize(c.stream));
        LY_HIP(hipMemcpy(&pool, c.ws.pool_total, 8, hipMemcpyDeviceToHost));
        pool_sum += pool;
        if (reset) LY_TRY(memset_done(c.ws.pool_total, 0, 8));
    }
    h->prof.pool_entries = pool_sum;
    *out = h->prof;
    if (reset) h->prof = lynse_hip_profile{};
    return LYNSE_OK;
}

// ------------------------------------------------------------------------------------- search ----
constexpr uint32_t QCHUNK = 256;
constexpr int SEL_NT = 512;
constexpr uint32_t SEG_KEYS = 32768;  // keys per query in the segmented-emission buffer
constexpr uint32_t SEG_MAX = 2048;    // most segments per query (grid x row-waves: 512 x 4 for the <= 32-query kernel)

// segments of one scan launch: grid x WR of min(255, SEG_KEYS / nseg) slots
static void seg_geometry(uint32_t grid, uint32_t wr, uint32_t* nseg, uint32_t* seg) {
    *nseg = grid * wr;
    *seg = 0;
    if (*nseg == 0 || *nseg > SEG_MAX) { *nseg = 0; return; }
    *seg = std::min<uint32_t>(255u, SEG_KEYS / *nseg);
}

template <typename K>
static int set_max_lds(K kernel, size_t bytes) {
    LY_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return LYNSE_OK;
}
// The opt-in to more than 64 KiB of dynamic LDS, one record per kernel instantiation K: the size already granted, raised when a launch
// asks for more (every site that launches K shares the record, and a later one may need more than the first).  The record is per
// process, not per device: the library's model is one process per device.  Two threads racing on the first call both set the attribute;
// the one whose record update finds that the other got in between sets the larger of the two sizes again, so that once both have
// returned the attribute and the record agree on the maximum (a plain store could leave the record above the attribute).  That holds
// only after the racers have returned: while one of them is between its two steps the attribute can be below the record, and a third
// thread launching K then would skip the opt-in.  No lock is taken for it, since no site can get there: every instantiation is launched
// with one size or is granted its maximum up front.
template <auto K>
static int ensure_lds(size_t bytes) {
    static std::atomic<size_t> granted{0};
    size_t seen = granted.load(std::memory_order_acquire);
    if (bytes <= seen) return LYNSE_OK;
    for (;;) {
        LY_TRY(set_max_lds(K, bytes));
        if (granted.compare_exchange_strong(seen, bytes, std::memory_order_acq_rel, std::memory_order_acquire)) return LYNSE_OK;
        bytes = std::max(bytes, seen);   // (the record moved under us: our call may have lowered the attribute below it)
    }
}
template <auto K, typename... Args>
static int launch_lds(dim3 grid, dim3 block, size_t lds, hipStream_t st, const Args&... a) {
    LY_TRY(ensure_lds<K>(lds));
    hipLaunchKernelGGL(K, grid, block, lds, st, a...);
    LY_HIP(hipGetLastError());
    return LYNSE_OK;
}

// ---- the three MFMA scan kernels, launched by name ----------------------------------------------------------------------------------
// A site names an instantiation as a config value (H16Cfg, QsCfg, QhCfg: next to each kernel); these helpers are the one place that maps
// a config to the kernel's positional template arguments, and the block size and LDS bytes of the launch follow from the config.
template <H16Cfg C>
static int launch_h16(dim3 grid, hipStream_t st, const ScanArgs& a) {
    return launch_lds<k_scan_h16<C.wq, C.wr, C.tq, C.tr, C.metric, C.nsv, C.nsq, C.nt_hint, C.tiled, C.rag, 0, C.filt, C.i8q, C.emit, C.dense, C.qcreg, C.fs>>(
        grid, h16_threads(C), h16_lds_bytes(C), st, a);
}
template <QsCfg C>
static int launch_qs(dim3 grid, hipStream_t st, const ScanArgs& a) {
    return launch_lds<k_scan_qs<C.nslab, C.rb, C.sl, C.ns, C.xpf, C.nbuf, C.dbg, C.ping, C.sts, C.met, C.smp, C.msk, C.f4, C.m16>>(grid, QS_THREADS, qs_lds_bytes(C), st, a);
}
template <QhCfg C>
static int launch_qh(dim3 grid, hipStream_t st, const ScanArgs& a) {
    return launch_lds<k_scan_qh<C.nslab, C.met, C.ns, C.nbuf, C.qb, C.smp>>(grid, QH_THREADS, qh_lds_bytes(C), st, a);
}
// A copy of config c with some members set: with(I8C_256, &H16Cfg::emit, 1, &H16Cfg::rag, true).
template <class C, class T, class V, class... More>
constexpr C with(C c, T C::*member, V value, More... more) {
    c.*member = value;
    if constexpr (sizeof...(more) > 0) return with(c, more...);
    else return c;
}
// f(std::integral_constant<int, M>{}) for the run-time metric of a float scan (IP, squared L2, everything else scores as cosine)
template <class F>
static int with_metric(int metric, F&& f) {
    switch (metric) {
    case M_IP: return f(std::integral_constant<int, M_IP>{});
    case M_L2: return f(std::integral_constant<int, M_L2>{});
    default: return f(std::integral_constant<int, M_COS>{});
    }
}
static int ensure_workspace(lynse_hip_flat* h, uint32_t k /* caller's k = output stride */) {
    Workspace& w = cur(h).ws;
    const uint32_t nslab = (h->dim + SCAN_BK - 1) / SCAN_BK;
    const uint32_t QC = std::max<uint32_t>(h->qchunk, QCHUNK);
    if (w.cand && w.cap == h->cap && w.D == h->dim && w.kcap >= k && w.qcap == QC) return LYNSE_OK;
    w.release();
    w.qcap = QC;
    w.cap = h->cap;
    w.D = h->dim;
    w.W = h->words;
    w.kcap = std::max<uint32_t>(k, 128);
    LY_HIP(hipMalloc(&w.cand, (size_t)QC * w.cap * 8));
    LY_HIP(hipMalloc(&w.candB, (size_t)QCHUNK * SEG_KEYS * 8));
    LY_HIP(hipMalloc(&w.segcnt, (size_t)QCHUNK * SEG_MAX));
    LY_HIP(hipMalloc(&w.count, (size_t)QC * 4));
    LY_HIP(hipMalloc(&w.thr, (size_t)QC * 4));
    LY_HIP(hipMalloc(&w.qinv, (size_t)QC * 4));
    LY_HIP(hipMalloc(&w.qn2, (size_t)QC * 4));
    LY_HIP(hipMalloc(&w.qrinv, (size_t)QC * 4));
    LY_HIP(hipMalloc(&w.marg2, (size_t)QC * 4));
    LY_HIP(hipMalloc(&w.pred_chk, (size_t)QC * 4));
    LY_HIP(hipMalloc(&w.pred_dbg, (size_t)QC * 16));
    w.q16_halves = (size_t)nslab * QC * SCAN_LDK;
    LY_HIP(hipMalloc(&w.Q16, w.q16_halves * sizeof(_Float16)));
    LY_TRY(memset_done(w.Q16, 0, w.q16_halves * sizeof(_Float16)));
    LY_HIP(hipMalloc(&w.Qf, (size_t)QC * h->dim * 4));
    LY_HIP(hipMalloc(&w.QW, (size_t)QCHUNK * h->words * 8));
    {
        uint32_t wcap = 1;
        while (wcap < h->words) wcap <<= 1;
        LY_HIP(hipMalloc(&w.QWp, (size_t)QCHUNK * wcap * 8));
    }
    LY_HIP(hipMalloc(&w.out_rows, (size_t)QC * w.kcap * 8));
    LY_HIP(hipMalloc(&w.out_dists, (size_t)QC * w.kcap * 4));
    LY_HIP(hipMalloc(&w.out_counts, (size_t)2 * QC * 4));
    w.overflow = w.out_counts + QC;
    LY_HIP(hipHostMalloc(&w.h_hdr, (size_t)2 * QC * 4, hipHostMallocDefault));
    LY_HIP(hipHostMalloc(&w.h_out, H_OUT_BYTES, hipHostMallocDefault));
    LY_HIP(hipMalloc(&w.pool_total, 8));
    LY_TRY(memset_done(w.pool_total, 0, 8));
    LY_HIP(hipMalloc(&w.dyn, (size_t)QC * 34 * sizeof(int)));
    LY_HIP(hipMalloc(&w.gsync, 256 + 1024 * 64));   // hand-over words
    LY_TRY(memset_done(w.gsync, 0, 256 + 1024 * 64));
    LY_HIP(hipMalloc(&w.small_part, (size_t)SMALL_NT * SMALL_MAX_Q * SMALL_MAX_K * 8));
    LY_HIP(hipMalloc(&w.small_ticket, 16));
    LY_TRY(memset_done(w.small_ticket, 0, 16));
    return LYNSE_OK;
}

struct Stage {
    uint32_t r0, r1;
    uint32_t sample_tiles = 0, sample_stride = 0;  // sample stage: sample_tiles tiles of tile_rows rows at t * sample_stride
};

// level 0: sampled plan (k_scan_h16 only) — stage 0 scans `cap/2` rows taken as evenly spread tiles, so the first
//          threshold is representative of the whole shard whatever the insertion order (a collection sorted by
//          similarity to the query would overflow every stage of the contiguous plan); the following stages grow
//          by min(16, cap/(8k)) — measured best on 10M and 1.25M rows (larger growth: fewer launches but thousands
//          of emitted keys per query in the first full stage);
// level 1: contiguous plan [0,S0) [S0,8*S0) ... (all other kernels; retry after an overflow of level 0);
// level 2: exhaustive plan, stages of cap/2 rows — cannot overflow.
static std::vector<Stage> make_plan(const lynse_hip_flat* h, uint32_t k, int level, uint32_t tile_rows, bool threshold_only_sample = false, uint32_t growth_hint = 0) {
    std::vector<Stage> plan;
    const uint64_t n = h->n;
    if (n == 0) return plan;
    if (level >= 2) {
        const uint32_t step = h->cap / 2;
        for (uint64_t r = 0; r < n; r += step) plan.push_back({(uint32_t)r, (uint32_t)std::min<uint64_t>(n, r + step)});
        return plan;
    }
    if (level == 0 && tile_rows && n > 4ull * h->cap) {
        // emit-all sample: every sample row becomes a key (S <= cap / 2).  Threshold-only sample: 16 keys per tile, and a
        // tile per CU costs the same latency as 32 tiles — a larger sample gives a tighter first threshold for free
        // (its rows are scanned again: keep it <= n / 16).
        uint32_t S = h->cap / 2;
        if (threshold_only_sample) {
            const uint64_t want = (uint64_t)h->num_cu * tile_rows;
            S = (uint32_t)std::max<uint64_t>(S, std::min<uint64_t>(std::min<uint64_t>(want, n / 16), (uint64_t)h->cap / 16 * tile_rows));
            S = S / tile_rows * tile_rows;
        }
        const uint32_t nt = S / tile_rows;
        const uint64_t stride = (n - tile_rows) / (nt - 1) / tile_rows * tile_rows;
        if (stride > tile_rows) {
            Stage s0{0u, (uint32_t)n};
            s0.sample_tiles = nt;
            s0.sample_stride = (uint32_t)stride;
            plan.push_back(s0);
            const uint64_t gmax = growth_hint ? growth_hint : (threshold_only_sample ? 32ull : 16ull);  // measured best on 10M and 1.25M rows
            const uint64_t g = std::max<uint64_t>(2, std::min<uint64_t>(gmax, h->cap / (8ull * std::max<uint32_t>(k, 1))));
            uint64_t seen = S, b = 0;
            while (b < n) {
                uint64_t nb = std::min<uint64_t>(n, (seen * g + tile_rows - 1) / tile_rows * tile_rows);
                if (n - nb < nb / 8) nb = n;  // do not leave a sliver for an extra launch
                plan.push_back({(uint32_t)b, (uint32_t)nb});
                seen = nb;
                b = nb;
            }
            return plan;
        }
    }
    uint64_t s0 = std::max<uint64_t>(h->stage0_rows, std::min<uint64_t>(h->cap, 4ull * k));
    s0 = (s0 + 255) / 256 * 256;  // stage boundaries on 256-row tiles (mask words, tile grid of the sample stage)
    s0 = std::min<uint64_t>(std::min<uint64_t>(s0, h->cap), n);
    uint64_t g = std::max<uint64_t>(2, std::min<uint64_t>(h->growth, h->cap / (4ull * std::max<uint32_t>(k, 1))));
    uint64_t b = s0;
    plan.push_back({0u, (uint32_t)b});
    while (b < n) {
        uint64_t nb = std::min<uint64_t>(n, b * g);
        plan.push_back({(uint32_t)b, (uint32_t)nb});
        b = nb;
    }
    return plan;
}

// Named tilings of the float scan over the f16 shadow (launch_scan_h16 sets the metric and the ragged / filter / emission fields per
// call).  nt_hint = 2 everywhere: the rows are streamed once.
constexpr H16Cfg F16_SMALL{.wq = 1, .wr = 4, .tq = 1, .tr = 1, .metric = M_IP, .nsv = 3, .nsq = 3, .nt_hint = 2};      // 128 rows x 32 queries
constexpr H16Cfg F16_IP_256{.wq = 2, .wr = 4, .tq = 4, .tr = 2, .metric = M_IP, .nsv = 3, .nsq = 2, .nt_hint = 2};     // 256 x 256, 3 + 2 stages
constexpr H16Cfg F16_L2_256{.wq = 4, .wr = 2, .tq = 2, .tr = 4, .metric = M_L2, .nsv = 2, .nsq = 2, .nt_hint = 2};     // 256 x 256, 2 + 2 stages + norms

// k_scan_h16 launcher for the tiling BASE.
// The 256 x 256 tilings compile ONE epilogue per emission mode (EMIT template parameter: 0 threshold stages, 1 emit-all
// first stage, 2 lane-max sample stage — one body with all three spills, kernels.h) and only the tiling / metric pairs
// the product path uses: <2,4,4,2> for unfiltered IP, <4,2,2,4> for L2 / cosine and every subset-filtered scan.
// The <= 32-query kernel and the IVF work-list kernel (<1,4,1,1>) keep the runtime emission switch (no spills there).
template <H16Cfg BASE>
static int launch_scan_h16(const ScanArgs& a, int metric, uint32_t grid, hipStream_t st, uint32_t grid_y = 1) {
    const dim3 g(grid, grid_y);
    const bool filt = a.mask != nullptr || a.row_ids != nullptr;
    const bool ragged = a.ld16 % HK != 0;
    if constexpr (BASE.wq * BASE.wr == 8 && !BASE.tiled) {
        // one kernel per (metric, ragged / filter variant, emission mode)
        auto by_emit = [&](auto mtag, auto ragtag, auto filtag) -> int {
            constexpr H16Cfg C = with(BASE, &H16Cfg::metric, decltype(mtag)::value, &H16Cfg::rag, decltype(ragtag)::value, &H16Cfg::filt, decltype(filtag)::value, &H16Cfg::emit, 0);
            if constexpr (C.wr < 4 && !C.filt && C.metric != M_IP) {  // many survivors per block expected: one-pass epilogue (kernels.h, DENSE)
                if (a.emit_all == 0 && a.dense) return launch_h16<with(C, &H16Cfg::dense, true)>(g, st, a);
            }
            if (a.emit_all == 0) return launch_h16<C>(g, st, a);
            if constexpr (!C.filt) {  // (the lane-max sample stage exists for the unfiltered tilings only)
                if (a.emit_all == 2) return launch_h16<with(C, &H16Cfg::emit, 2)>(g, st, a);
            }
            return launch_h16<with(C, &H16Cfg::emit, 1)>(g, st, a);
        };
        auto by_variant = [&](auto mtag) -> int {
            if (filt) {  // subset filter compiled in (always the ragged-capable variant)
                if constexpr (BASE.wr >= 4) return set_error(LYNSE_ERR_INTERNAL, "subset-filtered scans run on the <4,2,2,4> tiling");
                else return by_emit(mtag, std::true_type{}, std::true_type{});
            }
            if (ragged) return by_emit(mtag, std::true_type{}, std::false_type{});
            return by_emit(mtag, std::false_type{}, std::false_type{});  // no ragged last slab: branch-free DMA issue
        };
        if constexpr (BASE.wr >= 4) {  // <2,4,4,2>: unfiltered IP only
            if (metric != M_IP) return set_error(LYNSE_ERR_INTERNAL, "the <2,4,4,2> tiling is compiled for IP only");
            return by_variant(std::integral_constant<int, M_IP>{});
        } else {
            switch (metric) {
            case M_IP:
                if (!filt) return set_error(LYNSE_ERR_INTERNAL, "unfiltered IP scans run on the <2,4,4,2> tiling");
                return by_emit(std::integral_constant<int, M_IP>{}, std::true_type{}, std::true_type{});
            case M_L2: return by_variant(std::integral_constant<int, M_L2>{});
            default: return by_variant(std::integral_constant<int, M_COS>{});
            }
        }
    } else {
        auto by_metric = [&](auto ragtag, auto filtag) -> int {
            constexpr H16Cfg C = with(BASE, &H16Cfg::rag, decltype(ragtag)::value, &H16Cfg::filt, decltype(filtag)::value);
            return with_metric(metric, [&](auto mtag) { return launch_h16<with(C, &H16Cfg::metric, decltype(mtag)::value)>(g, st, a); });
        };
        if (!ragged && !filt) return by_metric(std::false_type{}, std::false_type{});
        if (filt) return by_metric(std::true_type{}, std::true_type{});  // subset filter compiled in (always the ragged-capable variant: one instantiation per metric)
        return by_metric(std::true_type{}, std::false_type{});
    }
}

// certified int8 coarse pass for batches of <= 32 queries: the 128-row x 32-query tiling (two workgroups per CU, 3 + 3-stage
// rings) over the SQ8 codes — HBM-bound like its f16 twin, at half the bytes; emission mode at run time (EMIT = -1)
constexpr H16Cfg I8C_SMALL = with(F16_SMALL, &H16Cfg::rag, false, &H16Cfg::i8q, 2);
static int launch_scan_i8c_small(const ScanArgs& a, uint32_t grid, hipStream_t st, bool l2n = false, bool filt = false) {
    if (filt) {   // masked scan of a small batch (row bitmask in the epilogue): whole slabs
        if (a.ld16 % 128 != 0 || a.row_ids || l2n) return set_error(LYNSE_ERR_INTERNAL, "the masked int8 scan needs whole 128-column slabs and a row bitmask");
        return launch_h16<with(I8C_SMALL, &H16Cfg::filt, true)>(grid, st, a);
    }
    if (l2n)   // plain-code L2 (I8Q = 4): with the norm ring
        return launch_h16<with(I8C_SMALL, &H16Cfg::metric, M_L2, &H16Cfg::i8q, 4)>(grid, st, a);
    if (a.ld16 % 128 == 0) return launch_h16<I8C_SMALL>(grid, st, a);
    return launch_h16<with(I8C_SMALL, &H16Cfg::rag, true)>(grid, st, a);
}

// The query-stationary tiling of the certified int8 pass (scan_qs.h): threshold stages of an unfiltered FLAT batch over whole
// 768-byte code rows — 8 waves x 32 register-resident queries, 64-row tiles, rows-only LDS ring.  LYNSE_HIP_QS=0: the 256 x 256
// tile of k_scan_h16 (A/B, tests; read per call).
// LYNSE_HIP_QS selects the instantiation (A/B; the default is the fastest measured): 1 = 64-row tiles, whole-K stages, 3-stage ring,
// ping-pong roles; 2 = 32-row tiles, 6-stage ring, fragments prefetched across the barrier; 3 = as 1 without the ping-pong roles.
static int qs_variant() { return env_int("LYNSE_HIP_QS", 1); }
static uint32_t qs_rows(int v) { return v == 2 ? 32u : 64u; }   // rows per tile
// LYNSE_HIP_QS_WIDTHS=0: the query-stationary tiling for 768 columns only (A/B; read per call)
static bool qs_widths_on() { return env_on("LYNSE_HIP_QS_WIDTHS", true); }
// LYNSE_HIP_QS_MASKED=0: the masked threshold stages on the DENSE masked epilogue of k_scan_h16 (A/B; read per call)
static bool qs_masked_on() { return env_on("LYNSE_HIP_QS_MASKED", true); }
// LYNSE_HIP_AG=1: the threshold stages of the certified int8 pass with one wave per SIMD (kernels.h, AG; A/B, tests; read per call)
static int ag_env() { return env_int("LYNSE_HIP_AG", 0); }

// The tilings of k_scan_qs: 64-row tiles, whole-K stages of NSLAB slabs of 128 code columns, 3-stage ring, ping-pong roles (2..6 slabs); 1024
// columns run 32-row tiles on a 4-stage ring (B = 128 registers).
constexpr QsCfg qs_64(int nslab) { return {.nslab = nslab, .rb = 2, .sl = nslab, .ns = 3, .xpf = false, .nbuf = 8, .ping = 1}; }
constexpr QsCfg QS_768 = qs_64(6);
constexpr QsCfg QS_1024{.nslab = 8, .rb = 1, .sl = 8, .ns = 4, .xpf = false, .nbuf = 8, .ping = 1};
// f(std::integral_constant<int, NSLAB>{}) for the 2..5-slab code rows of qs_64; every other count is the 6 slabs of 768 columns
template <class F>
static int with_qs_slabs(uint32_t nslab, F&& f) {
    switch (nslab) {
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 5: return f(std::integral_constant<int, 5>{});
    default: return f(std::integral_constant<int, 6>{});
    }
}

// Squared L2 on the query-stationary tiling (scan_qs.h, MET = 1): threshold stages of unfiltered batches of 129..256 queries over code
// rows of 768 bytes (64-row tiles).  Rows per tile, or 0.
static uint32_t qs_l2_rows(const ScanArgs& a) {
    const int v = qs_variant();
    if (v == 0) return 0;
    if (a.emit_all != 0 || a.qpad != 256 || a.nq > 256 || a.tile_stride != 0 || a.skip_stride != 0 || a.mask || a.row_ids || a.row1 <= a.row0) return 0;
    if (a.ld16 == 768 && a.nslab == 6) return 64;
    // 256 / 384 / 512 / 640 columns (LYNSE_HIP_QS_WIDTHS=0 or an A/B variant of LYNSE_HIP_QS: 768 only)
    if (!qs_widths_on() || v != 1) return 0;
    // (6M rows, 256 queries: 256 / 384 columns 0.772 / 0.916 ms on the <4,2,2,4> tiling against 0.773 / 0.929 here — the float epilogue weighs more the
    // fewer MFMAs a tile has; 512 / 640 columns 1.125 / 1.347 -> 1.106 / 1.307; 100 queries: 0.65 / 0.80 / 0.94 / 1.11 -> 0.61 / 0.72 / 0.83 / 0.94)
    if (a.nslab >= 2 && a.nslab <= 5 && a.ld16 == a.nslab * 128u && (a.nslab >= 4 || a.nq <= 128)) return 64;
    return 0;
}
static int launch_scan_qs_l2(const ScanArgs& a, uint32_t grid, hipStream_t st) {
    return with_qs_slabs(a.nslab, [&](auto n) { return launch_qs<with(qs_64(decltype(n)::value), &QsCfg::met, 1)>(grid, st, a); });
}

// squared L2 on the plain SQ8 codes (kernels.h, I8Q = 4): the <4,2,2,4> L2 tiling with 2 + 2-stage rings and the norm ring, int8
// operands, float epilogue; whole 128-column slabs
constexpr H16Cfg L2_PLAIN = with(F16_L2_256, &H16Cfg::rag, false, &H16Cfg::i8q, 4, &H16Cfg::emit, 0);
static int launch_scan_i8l2(const ScanArgs& a, uint32_t grid, hipStream_t st, bool qs = false) {
    if (qs) return launch_scan_qs_l2(a, grid, st);
    if (a.ld16 % 128 != 0) return set_error(LYNSE_ERR_INTERNAL, "the plain-code L2 scan needs whole 128-column slabs");
    if (a.emit_all == 1) return launch_h16<with(L2_PLAIN, &H16Cfg::emit, 1)>(grid, st, a);
    if (a.emit_all == 2) return launch_h16<with(L2_PLAIN, &H16Cfg::emit, 2)>(grid, st, a);
    if (a.dense) return launch_h16<with(L2_PLAIN, &H16Cfg::dense, true)>(grid, st, a);
    return launch_h16<L2_PLAIN>(grid, st, a);
}

// certified int8 coarse pass for batches of 33..64 queries (128 rows x 64 queries, 4 waves, two workgroups per CU, 3 + 3 stages)
// and of 65..128 queries (256 rows x 128 queries, 8 waves as 2 x 4, 3 + 2 stages): per row byte they do a quarter / half of the
// MFMA and fragment-read work of the 256-query tiling, which a batch of 40 or 100 queries would otherwise pay in full
constexpr H16Cfg I8C_MID{.wq = 1, .wr = 4, .tq = 2, .tr = 1, .metric = M_IP, .nsv = 3, .nsq = 3, .nt_hint = 2, .rag = false, .i8q = 2};
constexpr H16Cfg I8C_MID_WIDE{.wq = 2, .wr = 4, .tq = 2, .tr = 2, .metric = M_IP, .nsv = 3, .nsq = 2, .nt_hint = 2, .rag = false, .i8q = 2};
static int launch_scan_i8c_mid(const ScanArgs& a, uint32_t grid, hipStream_t st, bool wide, bool l2n = false, bool filt = false) {
    const bool rag = a.ld16 % 128 != 0;
    if (filt) {   // masked scan (row bitmask in the epilogue): whole slabs
        if (rag || a.row_ids || l2n) return set_error(LYNSE_ERR_INTERNAL, "the masked int8 scan needs whole 128-column slabs and a row bitmask");
        if (!wide) return launch_h16<with(I8C_MID, &H16Cfg::filt, true)>(grid, st, a);
        return launch_h16<with(I8C_MID_WIDE, &H16Cfg::filt, true)>(grid, st, a);
    }
    if (l2n) {   // plain-code L2 (I8Q = 4): whole slabs, with the norm ring
        if (!wide) return launch_h16<with(I8C_MID, &H16Cfg::metric, M_L2, &H16Cfg::i8q, 4)>(grid, st, a);
        return launch_h16<with(I8C_MID_WIDE, &H16Cfg::metric, M_L2, &H16Cfg::i8q, 4)>(grid, st, a);
    }
    if (!wide) {
        if (!rag) return launch_h16<I8C_MID>(grid, st, a);
        return launch_h16<with(I8C_MID, &H16Cfg::rag, true)>(grid, st, a);
    }
    if (!rag) return launch_h16<I8C_MID_WIDE>(grid, st, a);
    return launch_h16<with(I8C_MID_WIDE, &H16Cfg::rag, true)>(grid, st, a);
}

// certified int8 coarse pass: the 256 x 256 IP tiling with 3 + 2-stage rings over 128-element slabs, one kernel per
// (ragged last slab, emission mode)
// Self-tightening single-launch scan (scan_qs.h, STS; LYNSE_HIP_STS=1 — OFF by default): unfiltered FLAT batches of 129..256 queries on
// the certified int8 pass (IP, cosine) over whole 768-byte code rows, k <= 32 (one partition maximum per wanted neighbour), shards
// large enough that every workgroup helper covers a query (8 grid >= nq) — first plan level only, the overflow ladder keeps the
// staged plans.  Bit-identical results (tests), and MEASURED no faster than the staged plan it replaces (MI355X, 10M x 768 x 256,
// scripts/qs_microbench.hip at the margin the benchmark data has, 2E = 0.76 sd of the scores): one launch 1986 us + query image +
// final select against 37 + 31 + ~1880 + 31 us of sample stage, selects and threshold stages.  Without the exact-rescored
// threshold the selects of the staged plan compute (tau_x - E instead of tau - 2E) the band of rows that must be kept is ~5x wider:
// ~4800 keys per query are emitted (10,000 for the unluckiest query; the cap is 16,384 — 6 of 256 queries of the C2 test overflowed
// and went down the ladder), 15-20 % of all tile epilogues take the slow path.
// Row widths the query-stationary tiling is instantiated for: whole 128-column slabs, 2..6 of them (256 / 384 / 512 / 640 / 768 columns of
// codes: the B operand of a wave is NSLAB x 16 registers).  The masked (MSK) and plain-L2 (MET) forms and the A/B variants exist for 768
// columns only.  LYNSE_HIP_QS_WIDTHS=0: 768 columns only (A/B; read per call).
static bool qs_width_ok(uint32_t ld, uint32_t nslab, bool only768 = false) {
    if (ld == 768 && nslab == 6) return true;
    if (only768 || qs_variant() != 1) return false;
    if (!qs_widths_on()) return false;
    return ((nslab >= 2 && nslab <= 5) || nslab == 8) && ld == nslab * 128u;   // (8 slabs = 1024 columns: 32-row tiles, B = 128 registers)
}
static bool sts_env_on() { return env_on("LYNSE_HIP_STS", false); }
static bool qs_scan_ok(const ScanArgs& a, bool fs, bool filt, bool f4) {
    const int v = qs_variant();
    if (v < 1 || v > 3) return false;
    // filt: the MASKED threshold stages of a subset-filtered search (row bitmask; k_scan_qs<.., MSK>) — LYNSE_HIP_QS_MASKED=0: the DENSE
    // masked epilogue of k_scan_h16 (A/B; read per call)
    if (filt && (!qs_masked_on() || v == 2 || !a.mask || a.row_ids)) return false;
    // f4: batched Hamming on the FP4 MFMA (k_scan_qs<.., F4>): 1024-bit fingerprints = 512 B of nibbles = 4 slabs; its plans carry an emit-all
    // sample whose tiles the kernel skips (a.skip_stride).  LYNSE_HIP_QS_F4=0: the 256 x 256 tile of k_scan_h16<.., I8Q = 3> (A/B; read per call)
    if (f4) {
        return env_on("LYNSE_HIP_QS_F4", true) && v == 1 && !fs && !filt && a.emit_all == 0 && (a.nslab == 2 || a.nslab == 4 || a.nslab == 8) && a.ld16 == a.nslab * 128u &&   // 512 / 1024 / 2048-bit rows
               a.qpad == 256 && a.nq <= 256 &&
               a.tile_stride == 0 && !a.mask && !a.row_ids && a.row1 > a.row0;
    }
    return !fs && a.emit_all == 0 && qs_width_ok(a.ld16, a.nslab, filt) && a.qpad == 256 && a.nq <= 256 && a.tile_stride == 0 &&
           (filt || (a.skip_stride == 0 && !a.mask)) && !a.row_ids && a.row1 > a.row0;
}
// Workgroups of the persistent threshold-stage scans: one 144-KB workgroup per CU, on every CU (the scan is bound by the power the chip
// may draw, not by its CU count: leaving a few CUs free for the short kernels of another batch in flight gained nothing).
static uint32_t qs_grid(const ScanArgs& a, uint32_t num_cu) {
    const uint32_t rt = a.nslab == 8 ? 32u : qs_rows(qs_variant());   // (1024 columns: 32-row tiles)
    return std::min<uint32_t>((a.row1 - a.row0 + rt - 1) / rt, num_cu);
}
// LYNSE_HIP_QS_M16: the MFMA shape of the plain threshold stages on the 64-row tilings (scan_qs.h, M16): 1 / unset (auto) =
// v_mfma_i32_16x16x64_i8, 0 = v_mfma_i32_32x32x32_i8 (A/B, tests; read per call).  Same wave tile, fragment reads, registers and key sets;
// the chip holds a higher clock on the smaller shape (profiles/qs16_microbench.txt, profiles/qs16_bench_ab.json).
static int qs_m16_env() { return env_int("LYNSE_HIP_QS_M16", -1); }
// Does this query-stationary threshold stage run the 16x16x64 form?  Plain stages of the default variant only: the sample stage, the
// masked and self-tightening stages, squared L2, FP4 Hamming and the 32-row tiles of 1024 columns keep the 32x32x32 form.  The caller
// sizes the segments by it (four per workgroup and query instead of two), and every threshold stage of a batch gets the same answer.
static bool qs_m16_stage(const ScanArgs& a, bool sts, bool filt, bool f4) {
    if (qs_m16_env() == 0 || qs_variant() != 1) return false;
    return !sts && !filt && !f4 && !a.mask && !a.dyn_thr && a.nslab >= 2 && a.nslab <= 6;
}
static int launch_scan_qs(const ScanArgs& a, uint32_t grid, hipStream_t st, bool m16 = false) {
    if (a.dyn_thr)   // self-tightening thresholds: the whole shard in one launch (scan_qs.h, STS)
        return launch_qs<with(QS_768, &QsCfg::ping, 0, &QsCfg::sts, 1)>(grid, st, a);
    if (a.mask) return launch_qs<with(QS_768, &QsCfg::msk, 1)>(grid, st, a);   // masked threshold stages (MSK)
    if (m16) {   // (qs_m16_stage: 2..6 slabs, the default variant)
        if (a.nseg != 0 && a.nseg != grid * 4u) return set_error(LYNSE_ERR_INTERNAL, "the 16x16x64 scan needs four segments per workgroup and query");
        return with_qs_slabs(a.nslab, [&](auto n) { return launch_qs<with(qs_64(decltype(n)::value), &QsCfg::m16, 1)>(grid, st, a); });
    }
    if (a.nslab >= 2 && a.nslab <= 5)   // the narrower code rows (qs_width_ok)
        return with_qs_slabs(a.nslab, [&](auto n) { return launch_qs<qs_64(decltype(n)::value)>(grid, st, a); });
    if (a.nslab == 8) return launch_qs<QS_1024>(grid, st, a);
    switch (qs_variant()) {
    case 2: return launch_qs<QsCfg{.nslab = 6, .rb = 1, .sl = 6, .ns = 6, .xpf = true, .nbuf = 8}>(grid, st, a);
    case 3: return launch_qs<with(QS_768, &QsCfg::ping, 0)>(grid, st, a);
    default: return launch_qs<QS_768>(grid, st, a);
    }
}

// The threshold-only SAMPLE stage on the query-stationary tiling (scan_qs.h, SMP = 1): the sample rows as 64-row tiles, four per workgroup
// on a full chip (one 144-KB workgroup per CU), 4 keys per workgroup and query = 1024 keys per query.  LYNSE_HIP_QS_SAMPLE=0: the 256 x 256 sample tiles of k_scan_h16 (A/B; read per call).
static bool qs_sample_ok(const ScanArgs& a, bool fs, bool filt, bool f4, uint32_t plan_tile) {
    const int v = qs_variant();
    if (!env_on("LYNSE_HIP_QS_SAMPLE", true) || (v != 1 && v != 3)) return false;
    return !fs && !filt && !f4 && a.emit_all == 2 && plan_tile == 256 && a.nslab != 8 && qs_width_ok(a.ld16, a.nslab) && a.qpad == 256 && a.nq <= 256 && a.tile_stride >= 256 &&
           a.skip_stride == 0 && !a.mask && !a.row_ids && a.row1 > a.row0;
}
static int launch_scan_qs_sample(const ScanArgs& a, uint32_t grid, hipStream_t st) {
    return with_qs_slabs(a.nslab, [&](auto n) { return launch_qs<with(qs_64(decltype(n)::value), &QsCfg::ping, 0, &QsCfg::smp, 1)>(grid, st, a); });
}

// The query-stationary tiling of the f16 shadow at low dimension (scan_qh.h): threshold stages of an unfiltered FLAT batch of 33..256
// queries on the float path over rows of 1 or 2 whole 64-element slabs (64 / 128 columns: BASELINE config 3).  ON by default since the
// deferred emission of round 5 (LYNSE_HIP_QH=0: k_scan_h16's 256 x 256 tile, A/B; read per call): bit-identical results (tests), C3
// 0.190-0.194 against 0.213-0.219 ms per batch on the same box; DESIGN 4.3 has the phase table and what the first versions lost to
// (keys stored straight to global memory stalled the ring; a grouped slow path as long as the MFMAs of its step).
constexpr int QH_DEFAULT = 1;
static int qh_variant() { return env_int("LYNSE_HIP_QH", QH_DEFAULT); }   // 0 = k_scan_h16, 1 = k_scan_qh
// the batch SHAPE k_scan_qh takes (shared with i8c_eligible, which sends FLAT-IP batches of this shape to the float pass only because
// this kernel runs them: ADVICE r5): 33..256 queries — one 256-query chunk —, rows of one or two whole 64-element slabs
static bool qh_shape(uint32_t ld16, uint64_t nq) { return qh_variant() == 1 && nq > SCAN_BQ_SMALL && nq <= QCHUNK && (ld16 == 64u || ld16 == 128u); }
static bool qh_scan_ok(const ScanArgs& a, bool filt, uint32_t qchunks, int level) {
    if (level != 0) return false;   // (the plan ladder's later levels run k_scan_h16: k_scan_qh may hand a batch with massive ties to it)
    return qh_shape(a.ld16, a.nq) && !filt && a.emit_all == 0 && qchunks == 1 && a.qpad == 256 && a.tile_stride == 0 && a.skip_stride == 0 && !a.mask && !a.row_ids &&
           !a.tiles && a.row1 > a.row0 && (a.nslab == 1 || a.nslab == 2) && a.ld16 == a.nslab * 64u;
}
static uint32_t qh_grid(const ScanArgs& a, uint32_t num_cu, uint32_t* segs_per_wg) {
    *segs_per_wg = 1u;   // (one segment per workgroup and query: the deferred emission of scan_qh.h)
    return std::min<uint32_t>((a.row1 - a.row0 + 63u) / 64u, 2u * num_cu);
}
// 32 queries per wave, 64-row tiles, two workgroups per CU (<= 80 KB of LDS each; three ring stages: the LDS of the fourth is the staging regions')
constexpr QhCfg qh_64(int nslab, int met, int smp) { return {.nslab = nslab, .met = met, .ns = 3, .nbuf = 2, .qb = 1, .smp = smp}; }
template <int SMP>
static int launch_scan_qh_any(const ScanArgs& a, int metric, uint32_t grid, hipStream_t st) {
    auto by_metric = [&](auto n) {
        return with_metric(metric, [&](auto m) { return launch_qh<qh_64(decltype(n)::value, decltype(m)::value, SMP)>(grid, st, a); });
    };
    return a.nslab == 1 ? by_metric(std::integral_constant<int, 1>{}) : by_metric(std::integral_constant<int, 2>{});
}
static int launch_scan_qh(const ScanArgs& a, int metric, uint32_t grid, hipStream_t st) { return launch_scan_qh_any<0>(a, metric, grid, st); }

// The threshold-only SAMPLE stage of the same plans on k_scan_qh<.., SMP> (scan_qh.h): the sample rows as 64-row tiles, two workgroups per CU,
// 4 keys per workgroup and query.
static bool qh_sample_ok(const ScanArgs& a, bool filt, uint32_t qchunks, int level, uint32_t plan_tile) {
    if (qh_variant() != 1 || level != 0) return false;
    return !filt && a.emit_all == 2 && plan_tile == 256 && qchunks == 1 && a.qpad == 256 && a.nq <= 256 && a.tile_stride >= 256 && a.skip_stride == 0 && !a.mask && !a.row_ids &&
           !a.tiles && a.row1 > a.row0 && (a.nslab == 1 || a.nslab == 2) && a.ld16 == a.nslab * 64u;
}
// -> the grid of the sample launch (0: the sample stage stays on k_scan_h16): two workgroups per CU, enough keys for k_select's threshold-only
// rule (>= 8 k), inside the candidate buffer, <= 32 tiles per workgroup (the packed position of a sample key, scan_qh.h)
static uint32_t qh_sample_grid(const ScanArgs& a, uint32_t sample_tiles, bool filt, uint32_t qchunks, int level, uint32_t plan_tile, uint32_t k, uint32_t cap, uint32_t num_cu) {
    if (!sample_tiles || !qh_sample_ok(a, filt, qchunks, level, plan_tile)) return 0;
    const uint32_t nt64 = sample_tiles * 4u, sgrid = std::min<uint32_t>(nt64, 2u * num_cu);
    const bool ok = (uint64_t)sgrid * 4u >= 8ull * k && sgrid * 4u <= cap && (nt64 + sgrid - 1) / sgrid <= 32u;
    return ok ? sgrid : 0u;
}
static int launch_scan_qh_sample(const ScanArgs& a, int metric, uint32_t grid, hipStream_t st) { return launch_scan_qh_any<1>(a, metric, grid, st); }

// (round 5, measured and removed: 1024-bit Hamming on a 64-queries-per-wave form of k_scan_qh — k_scan_qh<4, M_IP, 4, 8, QB = 2, one row block
// per wave, FP4 MFMA>: every row fragment read feeds two MFMAs, half the LDS fragment returns per MFMA.  Bit-identical, and SLOWER: C5 share
// 1.900 / 1.916 / 1.928 against 1.705 / 1.708 / 1.725 ms per batch, same box, alternating (scripts/gpu_r5_c5.sh): with one 32-row block per
// wave a step is 32 MFMAs between two barriers, and a wave's epilogue / DMA issue is no longer covered by its SIMD partner's MFMAs.)
// The 256 x 256 tiling of the certified int8 pass (3 + 2-stage rings over whole 128-column slabs, threshold stages) and its one-wave-per-SIMD
// form (kernels.h, AG)
constexpr H16Cfg I8C_256 = with(F16_IP_256, &H16Cfg::rag, false, &H16Cfg::i8q, 2, &H16Cfg::emit, 0);
constexpr H16Cfg I8C_AG = with(I8C_256, &H16Cfg::wr, 2, &H16Cfg::tr, 4);
static int launch_scan_i8c(const ScanArgs& a, uint32_t grid, hipStream_t st, bool fs = false, bool filt = false, bool f4 = false, bool qs = false, bool m16 = false) {
    if (qs && f4) {   // batched Hamming on the query-stationary tiling (scan_qs.h, F4)
        if (a.nslab == 2) return launch_qs<with(qs_64(2), &QsCfg::f4, 1)>(grid, st, a);   // 512-bit rows
        if (a.nslab == 8) return launch_qs<with(QS_1024, &QsCfg::f4, 1)>(grid, st, a);   // 2048-bit rows: 32-row tiles
        return launch_qs<with(qs_64(4), &QsCfg::f4, 1)>(grid, st, a);
    }
    if (qs) return launch_scan_qs(a, grid, st, m16);
    if (f4) {   // batched Hamming: FP4 +-1 operands (kernels.h, I8Q = 3); whole 128-B slabs by construction, unfiltered
        if (a.ld16 % 128 != 0 || filt || fs) return set_error(LYNSE_ERR_INTERNAL, "the FP4 Hamming scan runs unfiltered over whole slabs");
        if (a.emit_all == 1) return launch_h16<with(I8C_256, &H16Cfg::i8q, 3, &H16Cfg::emit, 1)>(grid, st, a);
        if (a.emit_all == 2) return launch_h16<with(I8C_256, &H16Cfg::i8q, 3, &H16Cfg::emit, 2)>(grid, st, a);
        if (a.dense) return launch_h16<with(I8C_256, &H16Cfg::i8q, 3, &H16Cfg::dense, true)>(grid, st, a);
        return launch_h16<with(I8C_256, &H16Cfg::i8q, 3)>(grid, st, a);
    }
    if (filt) {  // masked scan (subset as a row bitmask): emit-all sample with sentinels, DENSE threshold stages (kernels.h, FILT && I8C)
        if (a.ld16 % 128 != 0 || a.row_ids) return set_error(LYNSE_ERR_INTERNAL, "the masked int8 scan needs whole 128-column slabs and a row bitmask");
        if (a.emit_all == 1) return launch_h16<with(I8C_256, &H16Cfg::filt, true, &H16Cfg::emit, 1)>(grid, st, a);
        if (a.emit_all != 0 || !a.dense) return set_error(LYNSE_ERR_INTERNAL, "the masked int8 scan runs emit-all and DENSE threshold stages");
        return launch_h16<with(I8C_256, &H16Cfg::filt, true, &H16Cfg::dense, true)>(grid, st, a);
    }
    // One wave per SIMD: 4 waves x (128 queries x 128 rows), accumulators in fixed AGPR tuples (kernels.h, AG) — the threshold
    // stages over whole 128-column slabs (LYNSE_HIP_AG=1; the sample stages keep the 8-wave kernels)
    if (ag_env() && a.ld16 % 128 == 0 && a.emit_all == 0 && !fs) {
        if (a.dense) return launch_h16<with(I8C_AG, &H16Cfg::dense, true)>(grid, st, a);
        return launch_h16<I8C_AG>(grid, st, a);
    }
    if (a.ld16 % 128 == 0) {
        if (fs) {  // fused sample stage: sample tile + in-launch thresholds + the first threshold stage (kernels.h, FS)
            if (a.emit_all != 0) return set_error(LYNSE_ERR_INTERNAL, "the fused sample stage is a threshold stage");
            if (!a.dense) return set_error(LYNSE_ERR_INTERNAL, "the fused sample stage is compiled with the DENSE epilogue");  // (the two-level body spills 12 B with it)
            return launch_h16<with(I8C_256, &H16Cfg::dense, true, &H16Cfg::fs, 1)>(grid, st, a);
        }
        if (a.emit_all == 0 && a.dense) return launch_h16<with(I8C_256, &H16Cfg::dense, true)>(grid, st, a);
        if (a.emit_all == 0) return launch_h16<I8C_256>(grid, st, a);
        if (a.emit_all == 1) return launch_h16<with(I8C_256, &H16Cfg::emit, 1)>(grid, st, a);
        return launch_h16<with(I8C_256, &H16Cfg::emit, 2)>(grid, st, a);
    }
    if (a.emit_all == 0) return launch_h16<with(I8C_256, &H16Cfg::rag, true)>(grid, st, a);
    if (a.emit_all == 1) return launch_h16<with(I8C_256, &H16Cfg::rag, true, &H16Cfg::emit, 1)>(grid, st, a);
    return launch_h16<with(I8C_256, &H16Cfg::rag, true, &H16Cfg::emit, 2)>(grid, st, a);
}

// f16 shadow rows [n16, n) (all rows again when the scale changed)
static int ensure_shadow_locked(lynse_hip_flat* h) {
    if (h->packed_only || h->n == 0) return LYNSE_OK;
    if (is_f16(h) && h->sv == 1.0f) {   // the f16 bits ARE the shadow (no scaling): one copy of the rows in HBM
        if (!h->shadow_alias && h->rows16) (void)hipFree(h->rows16);
        h->shadow_alias = true;
        h->rows16 = h->rows_h;
        h->cap16 = h->capacity;
        h->n16 = h->n;
        h->sv16 = h->sv;
        return LYNSE_OK;
    }
    if (h->shadow_alias) {              // the scale moved away from 1: the shadow becomes a buffer of its own
        h->shadow_alias = false;
        h->rows16 = nullptr;
        h->cap16 = 0;
        h->n16 = 0;
    }
    if (h->cap16 < h->n) {
        const uint64_t cap = std::max<uint64_t>(h->capacity, h->n);
        _Float16* nr = nullptr;
        LY_HIP(hipMalloc(&nr, (size_t)cap * h->ld16 * sizeof(_Float16) + 256));
        if (h->rows16 && h->n16 && h->sv16 == h->sv)
            LY_HIP(hipMemcpyAsync(nr, h->rows16, (size_t)h->n16 * h->ld16 * sizeof(_Float16), hipMemcpyDeviceToDevice, cur(h).stream));
        LY_HIP(hipStreamSynchronize(cur(h).stream));
        if (h->rows16) (void)hipFree(h->rows16);
        h->rows16 = nr;
        h->cap16 = cap;
    }
    if (h->sv16 != h->sv) h->n16 = 0;
    if (h->n16 < h->n) {
        const uint64_t chunks = (h->n - h->n16) * (h->ld16 / 8);
        const uint32_t blocks = (uint32_t)std::min<uint64_t>((chunks + 255) / 256, (uint64_t)h->num_cu * 32);
        if (is_f16(h))
            hipLaunchKernelGGL(k_rows_to_f16<_Float16>, dim3(std::max<uint32_t>(blocks, 1)), dim3(256), 0, cur(h).stream, h->rows_h, h->ld16, h->dim,
                               h->n16, h->n, h->sv, h->rows16, h->ld16);
        else
            hipLaunchKernelGGL(k_rows_to_f16<float>, dim3(std::max<uint32_t>(blocks, 1)), dim3(256), 0, cur(h).stream, h->rows, h->ld, h->dim,
                               h->n16, h->n, h->sv, h->rows16, h->ld16);
        LY_HIP(hipGetLastError());
        LY_HIP(hipStreamSynchronize(cur(h).stream));
    }
    h->n16 = h->n;
    h->sv16 = h->sv;
    return LYNSE_OK;
}

static int launch_scan_binary(const BinArgs& a, int metric, uint32_t grid, size_t lds, hipStream_t st) {
    // (the opt-in is to the most the kernel may be launched with: the launch size depends on the batch)
    constexpr size_t LDS_MAX = 160 * 1024 - 64;
    switch (metric) {
    case M_HAMMING: LY_TRY(ensure_lds<k_scan_binary<0>>(LDS_MAX)); hipLaunchKernelGGL(k_scan_binary<0>, dim3(grid), dim3(256), lds, st, a); break;
    case M_DICE: LY_TRY(ensure_lds<k_scan_binary<2>>(LDS_MAX)); hipLaunchKernelGGL(k_scan_binary<2>, dim3(grid), dim3(256), lds, st, a); break;
    default: LY_TRY(ensure_lds<k_scan_binary<1>>(LDS_MAX)); hipLaunchKernelGGL(k_scan_binary<1>, dim3(grid), dim3(256), lds, st, a); break;
    }
    LY_HIP(hipGetLastError());
    return LYNSE_OK;
}

// rows wider than 4096 bits (k_scan_binary_wide): no LDS, no register-resident words
static int launch_scan_binary_wide(const BinArgs& a, int metric, uint32_t grid, hipStream_t st) {
    switch (metric) {
    case M_HAMMING: hipLaunchKernelGGL(k_scan_binary_wide<0>, dim3(grid), dim3(256), 0, st, a); break;
    case M_DICE: hipLaunchKernelGGL(k_scan_binary_wide<2>, dim3(grid), dim3(256), 0, st, a); break;
    default: hipLaunchKernelGGL(k_scan_binary_wide<1>, dim3(grid), dim3(256), 0, st, a); break;
    }
    LY_HIP(hipGetLastError());
    return LYNSE_OK;
}

// lane-per-row batched kernel: WCAP = the power of two >= words
template <int KIND>
static int launch_scan_binary_rows_k(const BinArgs& a, uint32_t grid, hipStream_t st) {
    auto lds = [](int wcap) { return (size_t)4 * 64 * bin_rows_stride(wcap); };
    if (a.W & 1u) {
        if (a.W <= 1) return launch_lds<k_scan_binary_rows<KIND, 1, true>>(grid, 256, lds(1), st, a);
        if (a.W <= 4) return launch_lds<k_scan_binary_rows<KIND, 4, true>>(grid, 256, lds(4), st, a);
        if (a.W <= 8) return launch_lds<k_scan_binary_rows<KIND, 8, true>>(grid, 256, lds(8), st, a);
        if (a.W <= 16) return launch_lds<k_scan_binary_rows<KIND, 16, true>>(grid, 256, lds(16), st, a);
        if (a.W <= 32) return launch_lds<k_scan_binary_rows<KIND, 32, true>>(grid, 256, lds(32), st, a);
        return launch_lds<k_scan_binary_rows<KIND, 64, true>>(grid, 256, lds(64), st, a);
    }
    if (a.W <= 2) return launch_lds<k_scan_binary_rows<KIND, 2, false>>(grid, 256, lds(2), st, a);
    if (a.W <= 4) return launch_lds<k_scan_binary_rows<KIND, 4, false>>(grid, 256, lds(4), st, a);
    if (a.W <= 8) return launch_lds<k_scan_binary_rows<KIND, 8, false>>(grid, 256, lds(8), st, a);
    if (a.W <= 16) return launch_lds<k_scan_binary_rows<KIND, 16, false>>(grid, 256, lds(16), st, a);
    if (a.W <= 32) return launch_lds<k_scan_binary_rows<KIND, 32, false>>(grid, 256, lds(32), st, a);
    return launch_lds<k_scan_binary_rows<KIND, 64, false>>(grid, 256, lds(64), st, a);
}
static int launch_scan_binary_rows(const BinArgs& a, int metric, uint32_t grid, hipStream_t st) {
    switch (metric) {
    case M_HAMMING: return launch_scan_binary_rows_k<0>(a, grid, st);
    case M_DICE: return launch_scan_binary_rows_k<2>(a, grid, st);
    default: return launch_scan_binary_rows_k<1>(a, grid, st);
    }
}

// dynamic LDS of the select / final kernels: the cap key slots + scratch for the LDS-staged exact rescoring (rescore_keys): 48 KB hold
// the query and 15 rows of 768 floats per chunk; one workgroup per query either way
constexpr size_t SEL_LDS_MAX = 150 * 1024;
static inline uint32_t sel_lds_bytes(uint32_t cap, uint32_t nq = 0) {
    // (a widened pass — thousands of queries per launch, the k-means assignment — is bound by how many of its one-per-query workgroups
    // fit a CU: no scratch there, 4096 key slots stay 32 KB instead of 80 KB)
    if (nq > 512) return cap * 8u;
    return (uint32_t)std::min<size_t>((size_t)cap * 8 + 48 * 1024, SEL_LDS_MAX);
}

static int get_event(lynse_hip_flat* h, size_t idx, hipEvent_t* out) {
    while (cur(h).ev_pool.size() <= idx) {
        hipEvent_t e;
        LY_HIP(hipEventCreate(&e));
        cur(h).ev_pool.push_back(e);
    }
    *out = cur(h).ev_pool[idx];
    return LYNSE_OK;
}

// The knobs of run_chunk that more than one place reads.
// LYNSE_HIP_FUSED=0: no fused single-launch search (k_small_search), FLAT and IVF (A/B); read once per process
static int fused_env() { static const int v = env_int("LYNSE_HIP_FUSED", 1); return v; }

// Squared L2 has two int8 forms: unfiltered FLAT batches over whole 128-column slabs run on the PLAIN codes with the exact f32
// row norms in a float epilogue (k_scan_h16<.., I8Q = 4>, every tiling: 1 B per element, no second code set, IP-sized margins);
// everything else (ragged widths, masked scans, IVF) on the codes of the AUGMENTED rows through the IP kernels.  nqc = 0: "not a FLAT
// batch" (IVF): the augmented form.
static bool l2_plain(const lynse_hip_flat* h, uint64_t nqc, bool masked) {
    // (1M x 128, k = 100: 0.244 ms on the f16 shadow, 0.277 on the codes with the <4,2,2,4> tiling and 0.291 with the query-stationary
    // L2 tiling (k_scan_qs<1,4,1,6,.., MET = 1>, built and measured in round 4: at k = 100 the first threshold lets 0.8 % of all
    // (row, query) pairs through and the scan is bound by the emission of ~8000 keys per query, not by the tiling) — from 256
    // dimensions on)
    return !masked && nqc >= 1 && nqc <= QCHUNK && h->ld8 % 128 == 0 && h->dim >= 256;
}
// The form of the certified int8 pass a batch of nqc queries of `metric` takes — which code set it streams and how the prep kernel
// builds the query image (I8cPrepArgs::l2n / aug / cosine).  nqc = 0: not a FLAT batch (the IVF list scan).
enum I8cForm { I8C_IP, I8C_L2_PLAIN, I8C_L2_AUG, I8C_COS };
static I8cForm i8c_form(const lynse_hip_flat* h, int metric, uint64_t nqc, bool masked) {
    if (metric == M_L2) return l2_plain(h, nqc, masked) ? I8C_L2_PLAIN : I8C_L2_AUG;
    return metric == M_COS ? I8C_COS : I8C_IP;
}
static const CodeSet& i8c_code_set(const lynse_hip_flat* h, I8cForm form) {
    return form == I8C_L2_AUG ? h->sq8a : (form == I8C_COS ? h->sq8c : h->sq8);
}
// What the prep and scan stages read of the code set of a form; sq7: the non-negative 7-bit copy stands in for the plain codes (its
// own scales and maxima; minima, pitch and width are those of `sq8`).
struct I8cOperand {
    const int8_t* codes;
    uint32_t ld, cols, norm_cols;   // norm_cols: the trailing columns that carry |v|^2 (the augmented form)
    const float *mins, *scales;
    uint32_t a1, a2sq;
    float eps2;
    bool sq7;
};
static I8cOperand i8c_operand(const lynse_hip_flat* h, I8cForm form, bool sq7) {
    const CodeSet& s = i8c_code_set(h, form);
    I8cOperand v{s.codes, s.ld, s.cols, s.cols - h->dim, s.mins, s.scales, s.a1, s.a2sq, s.eps2, sq7};
    if (sq7) { v.codes = h->sq7.codes; v.scales = h->sq7.scales; v.a1 = h->sq7.a1; v.a2sq = h->sq7.a2sq; v.eps2 = h->sq7.eps2; }
    return v;
}
static void fill_i8c_prep(I8cPrepArgs& p, const I8cOperand& v, I8cForm form) {
    p.mins = v.mins; p.scales = v.scales; p.a1 = v.a1;
    p.a2sq = v.a2sq; p.eps2 = v.eps2;   // (the Cauchy-Schwarz terms, k_i8c_prep_queries)
    p.cosine = form == I8C_COS ? 1 : 0; p.aug = (int)v.norm_cols; p.l2n = form == I8C_L2_PLAIN ? 1 : 0; p.sq7 = v.sq7 ? 1 : 0;
}

static int fused_sample_env() { return env_int("LYNSE_HIP_FUSED_SAMPLE", 0); }   // (read per call: tests flip it)
static bool sq7_wanted(const lynse_hip_flat* h, int metric, uint64_t nqc, bool masked);
static bool sq7_ready(const lynse_hip_flat* h);
static bool predict_wanted(const lynse_hip_flat* h, int metric, uint64_t nqc, uint32_t k, bool masked);
static double predict_keys_per_query(uint32_t k);

// What run_chunk does with the chunk.  CHUNK_ASSIGN (flat_assign_top1_device): the lane-max scan of the k-means assignment over EVERY
// tile of the (small) centroid store, then stop — k_assign_pick reads the keys (kernels.h).  CHUNK_COARSE_DUMP
// (lynse_hip_flat_coarse_scores): one emit-all stage over the whole (small) shard, then stop — the candidate buffer then holds the
// coarse score of every (row, query) exactly as the scan kernels compute it.
enum ChunkMode { CHUNK_SEARCH, CHUNK_ASSIGN, CHUNK_COARSE_DUMP };
struct ChunkReq {
    uint32_t nq = 0, k = 0, out_k = 0;
    int metric = 0, level = 0;           // level selects the stage plan (make_plan)
    const uint32_t* mask = nullptr;      // row bitmask of a subset filter
    const uint32_t* row_ids = nullptr;   // the scanned rows are a gathered copy: their ids in the shard
    // the float queries of the chunk when they already live in device memory that stays valid for the whole search (no staging copy into
    // the workspace); nullptr = w.Qf
    const float* qsrc = nullptr;
    // the coarse pass streams the SQ8 codes (1 B / element) against the symmetric int8 query image with a certified error bound
    // (k_i8c_prep_queries) instead of the f16 shadow — FLAT-IP batches of 33..256 queries
    bool i8c = false;
    bool allow_sts = true;    // the self-tightening single-launch scan may answer this chunk (an overflow of it is retried on the staged plan of the same coarse pass, without a strike)
    bool allow_predict = false;   // the chunk may run the predicted plan: one threshold stage on a threshold k_select_final verifies afterwards (the blocking FLAT search; a miss or an overflow is re-answered on the sampled plan)
    bool allow_sq7 = false;   // the chunk may scan the non-negative 7-bit copy of the codes (the blocking FLAT search and the certificate diagnostics; an overflow is re-answered on the SQ8 codes, without a strike against the int8 pass)
    struct Out {
        // where k_final writes rows, distances (stride out_k) and a second copy of the counts — the caller's device arrays or the pinned
        // staging buffer; nullptr = the workspace (copied out by the caller)
        uint64_t* rows = nullptr;
        float* dists = nullptr;
        uint32_t* counts2 = nullptr;
        uint32_t* any_ovf = nullptr;   // device status word k_final ORs the overflow flags into (searches in flight), or nullptr
        bool hdr_direct = false;       // k_final writes counts + overflow flags straight into the pinned header of the context (no copy kernel behind the search)
    } out;
    ChunkMode mode = CHUNK_SEARCH;
};
struct ChunkResult { bool sampled = false, used_sts = false, used_sq7 = false, used_predict = false; };   // the plan began with a sample stage / ran the self-tightening scan / read the SQ7 copy / ran on a predicted threshold
// the events of a profiled search: events taken from the context's pool so far, and (first event, rows scanned) per scan launch
struct ScanProf { size_t ev_used = 0; std::vector<std::pair<size_t, uint64_t>> scan_events; };

// One chunk (<= QCHUNK queries) whose inputs are already in the workspace (Qf for float metrics,
// QW for binary).  Results land in ws.out_* or where rq.out says.
static int run_chunk(lynse_hip_flat* h, const ChunkReq& rq, hipStream_t st, ScanProf* prof, ChunkResult* res = nullptr) {
    ChunkResult unread;
    if (!res) res = &unread;
    const uint32_t nq = rq.nq, k = rq.k, out_k = rq.out_k;
    const int metric = rq.metric, level = rq.level;
    const uint32_t *mask = rq.mask, *row_ids = rq.row_ids;
    const bool assign = rq.mode == CHUNK_ASSIGN, coarse_dump = rq.mode == CHUNK_COARSE_DUMP;
    bool i8c = rq.i8c;
    Workspace& w = cur(h).ws;
    const float* Qf = rq.qsrc ? rq.qsrc : w.Qf;
    const bool binary = metric >= M_HAMMING;
    const bool asc = metric_ascending(metric);
    // batched Hamming on the int8 MFMA: the +-1 copy of the rows is there and the batch is large enough (search_impl builds it)
    const bool bin_mfma = bin_mfma_eligible(h, metric, mask != nullptr || row_ids != nullptr, nq) && h->bpm && h->n_bpm == h->n;
    if (bin_mfma) i8c = true;   // the scan side IS the certified-int8 IP scan (exact here: margin 0)
    // squared L2 on the certified int8 pass: an inner product of augmented vectors in the negated score space (kernels.h,
    // I8cPrepArgs::aug): scan, thresholds and selects run as a best-first IP search, exact scores are -|q - v|^2
    // squared L2 on the plain codes + exact row norms (l2_plain): the <4,2,2,4> L2 tiling with int8 operands and the float epilogue
    const bool i8q = i8c && !bin_mfma;   // the chunk streams a code set
    // (i8c_eligible never admits the gathered rows of a subset filter: the code sets cover the shard, not the copy)
    if (i8q && row_ids) return set_error(LYNSE_ERR_INTERNAL, "the int8 pass does not scan gathered rows");
    const I8cForm form = i8q ? i8c_form(h, metric, nq, mask != nullptr) : I8C_IP;
    const bool l2n = i8q && form == I8C_L2_PLAIN;
    const bool aug = i8q && form == I8C_L2_AUG;
    const bool cosq = i8q && form == I8C_COS;   // cosine distance: unit vectors, negated score space (I8cPrepArgs::cosine)
    // SQ7: same kernels, same plan — only the code rows every stage reads and the prep outputs (B_q, E) differ
    // (sq7_wanted is the whole predicate of the shape: IP, 129..256 queries — so no small / mid tiling —, no self-tightening or fused-sample plan)
    const bool sq7 = rq.allow_sq7 && i8q && !mask && sq7_wanted(h, metric, nq, false) && sq7_ready(h);
    res->used_sq7 = sq7;
    const I8cOperand opd = i8q ? i8c_operand(h, form, sq7) : I8cOperand{};
    const int key_metric = (bin_mfma || aug || cosq) ? (int)M_IP : metric;   // the order of the candidate keys
    const uint32_t nslab = bin_mfma ? h->ld_bpm / 128 : i8c ? (opd.cols + 127) / 128 : (h->dim + SCAN_BK - 1) / SCAN_BK;  // HK == SCAN_BK == 64
    const bool small = nq <= SCAN_BQ_SMALL;
    // mid-size batches on the int8 codes: 33..64 queries -> the 128 x 64 tiling, 65..128 -> the 256 x 128 tiling (LYNSE_HIP_MID_TILINGS=0: off)
    const int mid_env = env_int("LYNSE_HIP_MID_TILINGS", 1);   // (read per call: tests flip it)
    // ... unless the query-stationary tiling takes the batch (768-column codes of the IP / cosine / plain-L2 forms; a row bitmask only on
    // the IP / cosine form): waves without queries skip their MFMAs there, and it beats both mid tilings from 33 queries on (10M x 768, IP:
    // 40 / 64 / 100 / 128 queries 1.28 / 1.32 / 1.48 / 1.49 -> 1.22 / 1.25 / 1.29 / 1.31 ms; L2 1.39 / 1.43 / 1.81 / 1.89 -> 1.34 / 1.38 / 1.57 /
    // 1.62).  LYNSE_HIP_QS_MID=0: the mid tilings (A/B, tests; read per call)
    const bool qs_mid = env_on("LYNSE_HIP_QS_MID", true) && qs_variant() >= 1 && qs_variant() <= 3 && i8c && !bin_mfma &&
                        !small && !row_ids && !aug && qs_width_ok(h->ld8, (h->dim + 127) / 128, mask != nullptr) && !(l2n && (h->dim + 127) / 128 == 8) && nq <= 256 &&   // (plain-L2: not on the 32-row tiles of 1024 columns)
                        (h->ld8 == 768 || nq > 64) &&   // (narrower rows: the 128 x 64 tiling keeps 33..64 queries — 6M x 256, 40 queries: 0.34 ms against 0.37)
                        (!mask || (!l2n && qs_variant() != 2 && qs_masked_on()));
    const bool mid_ok = mid_env && !qs_mid && i8c && !bin_mfma && !small && !row_ids && (!mask || opd.ld % 128 == 0);
    const bool mid64 = mid_ok && nq <= 64, mid128 = mid_ok && !mid64 && nq <= 128;
    const bool narrow = small || mid64;   // 128-row tiles
    const uint32_t qpad = small ? SCAN_BQ_SMALL : mid64 ? 64u : mid128 ? 128u : round_up(nq, SCAN_BQ_LARGE);  // > 256 queries: a widened handle, qpad / 256 chunks per launch
    const uint32_t qchunks = (small || mid64 || mid128) ? 1u : qpad / SCAN_BQ_LARGE;
    if (qchunks > 1 && (binary || i8c || mask || row_ids || h->n > w.cap || nq > w.qcap))
        return set_error(LYNSE_ERR_INTERNAL, "more than 256 queries per pass need the widened float pipeline over <= cap rows");
    int ip_form = h->ip_form;
    if (ip_form == LYNSE_IPFORM_AUTO) ip_form = h->n < 4096 ? LYNSE_IPFORM_SINGLE : LYNSE_IPFORM_BATCH8;
    if (mask || row_ids) ip_form = LYNSE_IPFORM_SINGLE;
    if (h->dtype == LYNSE_DTYPE_F16) ip_form = LYNSE_IPFORM_F16SEQ;  // every f16 path of the reference uses the sequential kernels  // search_filtered scores every row with the single-row kernels (flat_mmap.rs:553-560)

    LY_TRY(ensure_lds<k_select<SEL_NT>>(SEL_LDS_MAX));
    LY_TRY(ensure_lds<k_final<SEL_NT>>(SEL_LDS_MAX));
    LY_TRY(ensure_lds<k_select_final<SEL_NT>>(SEL_LDS_MAX));

    const bool sts = rq.allow_sts && sts_env_on() && level == 0 && i8c && !bin_mfma && !aug && !l2n && !small && !mid64 && !mid128 && !mask && !row_ids &&
                     k >= 1 && k <= 32 && qs_variant() >= 1 && qs_variant() <= 3 && opd.ld == 768 && nslab == 6 && qpad == 256 && h->n >= 65536 &&
                     h->n < 0xffffff00ull && (metric == M_IP || cosq);
    res->used_sts = sts;
    // Predicted plan: prep -> ONE threshold stage over [0, n) on the threshold the prep kernel predicts from the column statistics
    // of the code set the stage reads -> k_select_final, which verifies it.  (predict_wanted is the predicate of the shape; the statistics
    // must be up to date: code_stats_locked)
    const bool fused_tail_on = env_int("LYNSE_HIP_FUSED_TAIL", 1) != 0;   // (the verification lives in k_select_final)
    const CodeSet* pred_set = !i8q ? nullptr : (sq7 ? &h->sq7 : &i8c_code_set(h, form));
    const bool predict = rq.allow_predict && rq.mode == CHUNK_SEARCH && !sts && level == 0 && i8q && !aug && !l2n && !small && !mid64 && !mid128 && !mask && !row_ids &&
                         fused_tail_on && qpad == 256 && predict_wanted(h, metric, nq, k, false) && pred_set->stats_ready() && h->n < 0xffffff00ull;
    res->used_predict = predict;
    if (bin_mfma) {
        // (the prep kernels write every byte of the image: the lines of their queries, pad columns included, and — blocks nq .. qpad - 1 of the
        // grid — zero lines for the pad queries of the tile; up to round 5 a hipMemsetAsync of the image ran in front: a launch of its own)
        BpmPrepArgs p{};
        p.QW = w.QW; p.W = h->words; p.D = h->dim; p.qpad = qpad; p.nslab = nslab; p.nq = nq; p.img = reinterpret_cast<uint8_t*>(w.Q16);
        p.sq = w.qinv; p.bq = w.qn2; p.marg2 = w.marg2; p.thr = w.thr; p.count = w.count; p.overflow = w.overflow;
        hipLaunchKernelGGL(k_bpm_prep_queries, dim3(qpad), dim3(256), 0, st, p);
        LY_HIP(hipGetLastError());
    } else if (binary) {
        std::vector<float> thr0(nq, INFINITY);
        LY_HIP(hipMemcpyAsync(w.thr, thr0.data(), nq * 4, hipMemcpyHostToDevice, st));
        LY_HIP(hipMemsetAsync(w.count, 0, nq * 4, st));
        LY_HIP(hipMemsetAsync(w.overflow, 0, nq * 4, st));
        LY_HIP(hipStreamSynchronize(st));  // thr0 is a stack/heap temporary
    } else if (i8c) {
        I8cPrepArgs p{};
        p.Q = Qf; p.D = h->dim; p.qpad = qpad; p.nslab = nslab; p.nq = nq; p.vmax = h->vmax; p.img = reinterpret_cast<int8_t*>(w.Q16);
        fill_i8c_prep(p, opd, form);
        p.sq = w.qinv; p.bq = w.qn2; p.marg2 = w.marg2; p.thr = w.thr; p.count = w.count; p.overflow = w.overflow;
        p.gsync = w.gsync;
        if (predict) {
            p.pred_mu = pred_set->mu; p.pred_var = pred_set->var; p.pred_chk = w.pred_chk; p.pred_dbg = w.pred_dbg;
            p.pred_z = predict_z(h->n, predict_keys_per_query(k));
        }
        if (sts) {   // seed the partition maxima of the self-tightening scan from a few sample rows (valid thresholds from the first tile on)
            p.codes = opd.codes; p.ld8 = opd.ld; p.n_rows = (uint32_t)h->n; p.tile_rows = 64; p.dyn_ks = k;
            p.seed_rows = std::min<uint32_t>(1024u, 32u * k);
            p.dyn_thr = w.dyn; p.dyn_marg = w.dyn + w.qcap; p.dyn_slot = w.dyn + 2 * (size_t)w.qcap;
        }
        hipLaunchKernelGGL(k_i8c_prep_queries, dim3(qpad), dim3(256), sts ? (size_t)nslab * 128 : 0, st, p);
        LY_HIP(hipGetLastError());
    } else {
        // queries with index >= nq inside the padded tile must be finite: blocks nq .. qpad - 1 of the grid write zero lines
        PrepArgs p{};
        p.Q = Qf; p.D = h->dim; p.nq = nq; p.qpad = qpad; p.nslab = nslab; p.metric = metric; p.layout = 2;
        p.sv = h->sv; p.vmax = h->vmax; p.vmin = h->vmin; p.cos_degenerate = h->cos_degenerate; p.rows_integer = h->rows_integer; p.rows_nonneg = h->rows_nonneg; p.amax_v = h->amax;
        p.Q16 = w.Q16; p.qinv = w.qinv; p.qn2 = w.qn2; p.qrinv = w.qrinv; p.marg2 = w.marg2; p.thr = w.thr;
        p.count = w.count; p.overflow = w.overflow;
        hipLaunchKernelGGL(k_prep_queries, dim3(qpad), dim3(256), 0, st, p);
        LY_HIP(hipGetLastError());
    }

    // the sampled plan needs the strided-tile support of k_scan_h16; the popcount kernels start at level 1
    const uint32_t plan_tile = binary ? 0u : (narrow ? 128u : 256u);
    // wave tiling of the 256 x 256 tile (measured on MI355X, 10M x 768, 256 queries): IP is fastest with <2,4,4,2> and the
    // 3+2-stage split rings, L2 / cosine (norm ring in LDS, more registers in the epilogue) with <4,2,2,4> and 2+2 stages
    // (each tiling is compiled only for the metrics it is the default of)
    const bool filt = mask != nullptr || row_ids != nullptr;
    // (the subset-filter variants of <2,4,4,2> spill 96 B into the MFMA loop: masked 10M x 768 scan 7.5 ms vs 4.9 ms with <4,2,2,4>)
    const int waves16 = l2n ? 0 : i8c ? 3 : ((metric == M_IP && !filt) ? 3 : 0);
    // the subset-filter kernel variants carry no lane-max code (registers)
    // (k <= 16: the best tile alone supplies k keys, so even a shard sorted by score gets a tight threshold from its best
    // sample tile; up to k = 128 the sample as a whole supplies >= 8 k keys — a clustered shard may then overflow the first
    // stage and fall back to the contiguous plan)
    const bool can_threshold_only = !binary && !filt && k <= 128;
    Stage assign_stage{0u, (uint32_t)h->n};   // (CHUNK_ASSIGN) every 256-row tile of the store as a "sample" tile: lane-max keys, no threshold
    assign_stage.sample_tiles = (uint32_t)((h->n + 255) / 256);
    assign_stage.sample_stride = 256;
    const std::vector<Stage> plan = assign ? std::vector<Stage>{assign_stage}
                                    : (sts || coarse_dump || predict) ? std::vector<Stage>{Stage{0u, (uint32_t)h->n}}
                                        : make_plan(h, k, (level == 0 && !plan_tile) ? 1 : level, plan_tile, can_threshold_only,
                                                    // large k on the float tilings: the epilogue's cost is the emissions (one sample threshold over 1M x 128,
                                                    // k = 100, admits 1400 rows per query: 87 of the stage's 163 us) — a second threshold stage a quarter of the
                                                    // way in halves them (same box, alternating: 0.241 -> 0.233 ms per batch)
                                                    (!i8c && !binary && k >= 64) ? 4u : 0u);
    const Stage sample = (!plan.empty() && plan[0].sample_tiles) ? plan[0] : Stage{0, 0};
    res->sampled = sample.sample_tiles != 0;
    // sampled plan: the sample stage only has to produce a threshold -> one key per lane (its best row) instead of every
    // score, as long as that leaves comfortably more than k keys per query (2 WR keys per tile and query)
    const uint32_t sample_keys_per_tile = (small || mid64 || mid128 || waves16 != 0) ? 16u : 8u;  // 2 WR lanes per query and tile x their best 2 rows (WR = 4: 16, <4,2,2,4>: 8)
    // k <= keys per tile: the best sample tile alone supplies k keys (a shard sorted by score still gets a tight threshold)
    const bool sample_threshold_only = !binary && !filt && sample.sample_tiles && sample_keys_per_tile &&
                                       (k <= sample_keys_per_tile || (uint64_t)sample.sample_tiles * sample_keys_per_tile >= 8ull * k);
    // Fused sample stage (k_scan_h16<.., FS>, LYNSE_HIP_FUSED_SAMPLE=1; OFF by default): the sample tiles are scored by the
    // workgroups of the FIRST threshold stage (one each) and the grid agrees on the thresholds inside that launch — no
    // sample launch, no k_select between.  Needs one sample tile per workgroup, every workgroup resident (grid = CUs) and
    // the register-resident query constants of the certified int8 pass.  Bit-identical results (tests), but MEASURED SLOWER
    // than the two launches it replaces (MI355X, 1.25M x 768 x 256: 366 us against 33 + 26 + 261 us; s_memtime stamps:
    // first tile 32 us, hand-over 1 27 us, select 15 us, hand-over 2 17 us, restart): a grid-wide
    // hand-over drains the LDS-DMA ring of every CU and idles the chip twice, which costs more than a kernel boundary.
    const int fs_env = fused_sample_env();
    const bool fs = fs_env != 0 && i8c && !aug && !cosq && !l2n && !bin_mfma && !mid64 && !mid128 && h->ld8 % 128 == 0 && sample_threshold_only && plan.size() >= 2 && k <= 32 &&
                    sample.sample_tiles == (uint32_t)h->num_cu && (plan[1].r1 - plan[1].r0 + 255) / 256 >= (uint32_t)h->num_cu &&
                    (uint64_t)k * 50000ull > (uint64_t)sample.sample_tiles * plan_tile;   // (the stage behind the sample runs the DENSE epilogue)
    bool plan_used_segments = false, plan_used_qs = false, plan_qs_sample = false, plan_used_qh = false, plan_qs_m16 = false;
    // the select behind the last stage + exact rescoring + final order in one launch (k_select_final); LYNSE_HIP_FUSED_TAIL=0:
    // the three separate kernels (A/B)
    const int fused_tail_env = env_int("LYNSE_HIP_FUSED_TAIL", 1);   // (read per call: tests flip it)
    const bool fused_tail = fused_tail_env != 0 && !plan.empty();
    SelectArgs sa_last{};
    for (size_t si = 0; si < plan.size(); ++si) {
        const Stage s = plan[si];
        const bool emit_all = si == 0 && !sts && !predict;   // (predict: the one stage is a threshold stage on the predicted a.thr; sts: the one stage is a threshold stage — its thresholds live in w.dyn and tighten while it runs)
        if (fs && si == 0) continue;   // scored inside the launch of stage 1
        const bool fs_stage = fs && si == 1;
        uint32_t qs_sample_keys = 0;   // != 0: the sample stage ran on the query-stationary tiling and left this many keys per query
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (tl_prof) {
            LY_TRY(get_event(h, prof->ev_used++, &e0));
            LY_TRY(get_event(h, prof->ev_used++, &e1));
            LY_HIP(hipEventRecord(e0, st));
        }
        uint32_t st_nseg = 0, st_seg = 0;  // segmented emission of this stage (k_select gathers)
        int a_emit_all_last = -1;
        if (binary && !bin_mfma) {
            BinArgs b{};
            b.P = h->packed; b.W = h->words; b.row0 = s.r0; b.row1 = s.r1; b.QW = w.QW; b.nq = nq;
            b.thr = w.thr; b.cand = w.cand; b.count = w.count; b.cap = w.cap; b.emit_all = emit_all ? 1 : 0;
            b.mask = mask;
            static const int rows_minq = env_int("LYNSE_HIP_BIN_ROWS_MINQ", 1);
            if (h->words > 16u * BIN_MAX_CHUNKS) {  // wider than 4096 bits: the generic strided kernel
                const uint32_t groups = (s.r1 - s.r0 + 31) / 32;
                const uint32_t grid = std::max<uint32_t>(1, std::min<uint32_t>(groups, (uint32_t)h->num_cu * 8));
                LY_TRY(launch_scan_binary_wide(b, metric, grid, st));
            } else if ((int)nq >= rows_minq || mask) {  // batched: lane-per-row, scalar query words
                uint32_t wcap = 1;
                while (wcap < h->words) wcap <<= 1;
                if (wcap != h->words) {
                    if (si == 0) {
                        hipLaunchKernelGGL(k_pad_words, dim3((nq * wcap + 255) / 256), dim3(256), 0, st, w.QW, h->words, w.QWp, wcap, nq);
                        LY_HIP(hipGetLastError());
                    }
                    b.QW = w.QWp;
                }
                const uint32_t groups = (s.r1 - s.r0 + 255) / 256;
                const uint32_t grid = std::max<uint32_t>(1, std::min<uint32_t>(groups, (uint32_t)h->num_cu * 8));
                LY_TRY(launch_scan_binary_rows(b, metric, grid, st));
            } else {
                const uint32_t groups = (s.r1 - s.r0 + 31) / 32;
                const uint32_t grid = std::max<uint32_t>(1, std::min<uint32_t>(groups, (uint32_t)h->num_cu * 8));
                const size_t lds = (size_t)nq * h->words * 8 + (size_t)nq * 4;
                LY_TRY(launch_scan_binary(b, metric, grid, lds, st));
            }
        } else {
            ScanArgs a{};
            a.V = score_rows(h); a.ld = score_ld(h); a.D = h->dim; a.row0 = s.r0; a.row1 = s.r1; a.Q16 = w.Q16;
            a.mask = mask;
            a.row_ids = row_ids;
            a.tile_stride = s.sample_stride;  // 0 = contiguous
            if (!s.sample_tiles && sample.sample_tiles && !sample_threshold_only) { a.skip_stride = sample.sample_stride; a.skip_tiles = sample.sample_tiles; }
            const uint32_t tile_rows = narrow ? 128u : 256u;
            a.V16 = h->rows16; a.ld16 = h->ld16;
            if (i8c) { a.V16 = reinterpret_cast<const _Float16*>(bin_mfma ? (const int8_t*)h->bpm : opd.codes); a.ld16 = bin_mfma ? h->ld_bpm : opd.ld; }
            a.qpad = qpad; a.nq = nq; a.nslab = nslab; a.ntiles = (s.r1 - s.r0 + tile_rows - 1) / tile_rows;
            if (s.sample_tiles) a.ntiles = s.sample_tiles;
            a.qinv = w.qinv; a.qn2 = w.qn2; a.qrinv = w.qrinv; a.thr = w.thr; a.vn2 = h->vn2; a.vrinv = h->vrinv;
            a.sv = h->sv; a.vmax2 = h->vmax * h->vmax; a.cand = w.cand; a.count = w.count; a.cap = w.cap; a.emit_all = emit_all ? 1 : 0;
            // sampled plan: the sample stage only has to produce a threshold -> one key per lane (its best row) instead of
            // every score, as long as that leaves at least k keys per query
            if (sample_threshold_only && s.sample_tiles) a.emit_all = 2;
            if (i8c && small) {
                a.candB = w.candB; a.segcnt = w.segcnt;
                const uint32_t grid = std::min<uint32_t>(a.ntiles, (uint32_t)h->num_cu * 2);
                if (!a.emit_all) seg_geometry(grid, 4, &a.nseg, &a.seg);
                LY_TRY(launch_scan_i8c_small(a, grid, st, l2n, filt));
            } else if (mid64 || mid128) {
                a.candB = w.candB; a.segcnt = w.segcnt;
                const uint32_t grid = std::min<uint32_t>(a.ntiles, (uint32_t)h->num_cu * (mid64 ? 2u : 1u));
                if (!a.emit_all) seg_geometry(grid, 4, &a.nseg, &a.seg);
                LY_TRY(launch_scan_i8c_mid(a, grid, st, mid128, l2n, filt));
            } else if (l2n) {
                a.candB = w.candB; a.segcnt = w.segcnt;
                uint32_t grid = std::min<uint32_t>(a.ntiles, (uint32_t)h->num_cu);
                const uint64_t seen_before = s.sample_tiles ? 0 : (sample.sample_tiles ? std::max<uint64_t>((uint64_t)sample.sample_tiles * plan_tile, s.r0) : s.r0);
                a.dense = (!a.emit_all && seen_before) ? 1 : 0;   // (the DENSE float epilogue, like every L2 threshold stage of the f16 shadow)
                const uint32_t qs_rt = qs_l2_rows(a);   // threshold stages on the query-stationary tiling (scan_qs.h, MET = 1)
                if (qs_rt) {
                    grid = std::min<uint32_t>((a.row1 - a.row0 + qs_rt - 1) / qs_rt, (uint32_t)h->num_cu);
                    seg_geometry(grid, 2, &a.nseg, &a.seg);
                    plan_used_qs = true;
                } else if (!a.emit_all) seg_geometry(grid, a.dense ? 4 : 2, &a.nseg, &a.seg);
                LY_TRY(launch_scan_i8l2(a, grid, st, qs_rt != 0));
            } else if (i8c) {
                a.candB = w.candB; a.segcnt = w.segcnt;
                const uint32_t grid = std::min<uint32_t>(a.ntiles, (uint32_t)h->num_cu);
                // DENSE epilogue while the threshold is loose (kernels.h): the int8 margin keeps ~5x the rows an exact threshold
                // would, so a 32-query x 64-row block holds a survivor with probability ~ 2048 * 5 k / rows-seen-before; above
                // ~0.2 one integer compare per accumulator beats level 1 + (mostly) level 2.  Segments are per wave half then.
                const uint64_t seen_before = s.sample_tiles ? 0 : (sample.sample_tiles ? std::max<uint64_t>((uint64_t)sample.sample_tiles * plan_tile, s.r0) : s.r0);
                a.dense = (!a.emit_all && a.ld16 % 128 == 0 && seen_before &&
                           (filt || (uint64_t)k * 50000ull > seen_before)) ? 1 : 0;   // (masked: DENSE is the one epilogue compiled with the mask)
                const bool ag = ag_env() && a.ld16 % 128 == 0 && !a.emit_all && !fs_stage && !filt && !bin_mfma;
                if (sts) {
                    a.dyn_thr = w.dyn; a.dyn_marg = w.dyn + w.qcap; a.dyn_slot = w.dyn + 2 * (size_t)w.qcap; a.dyn_ks = k;
                    a.dyn_warm = h->n >= 4000000ull ? 4u : 2u;   // tiles per workgroup that only feed the maxima first (scanned again at the end)
                }
                // the threshold-only sample stage on the query-stationary tiling (4 keys per workgroup and query; the same sample rows)
                if (s.sample_tiles && !sts && qs_sample_ok(a, fs_stage, filt, bin_mfma, plan_tile)) {
                    const uint32_t nt64 = s.sample_tiles * 4u;
                    const uint32_t sgrid = std::min<uint32_t>(nt64, (uint32_t)h->num_cu);   // one 144-KB workgroup per CU: a second round of workgroups pays the launch ramp and the query image again (40 us against 30)
                    if ((uint64_t)sgrid * 4u >= 8ull * k && sgrid * 4u <= w.cap && (nt64 + sgrid - 1) / sgrid <= 32u) {   // (<= 32 tiles per workgroup: the packed position of a sample key, scan_qs.h)
                        a.ntiles = nt64;
                        LY_TRY(launch_scan_qs_sample(a, sgrid, st));
                        qs_sample_keys = sgrid * 4u;
                        plan_qs_sample = true;
                    }
                }
                if (!qs_sample_keys) {
                const bool qs = sts || (!ag && qs_scan_ok(a, fs_stage, filt, bin_mfma));   // the query-stationary tiling (scan_qs.h): two segments per workgroup and query
                uint32_t launch_grid = qs ? qs_grid(a, (uint32_t)h->num_cu) : grid;
                if (sts) {   // contiguous chunks of dyn_pitch tiles per workgroup; the pitch coprime to the partition count (scan_qs.h)
                    const uint32_t nt = (a.row1 - a.row0 + 63) / 64;
                    uint32_t pitch = (nt + launch_grid - 1) / launch_grid;
                    auto gcd = [](uint32_t x, uint32_t y) { while (y) { const uint32_t t = x % y; x = y; y = t; } return x; };
                    while (gcd(pitch, k) != 1) ++pitch;
                    a.dyn_pitch = pitch;
                    launch_grid = (nt + pitch - 1) / pitch;
                }
                const bool m16 = qs && qs_m16_stage(a, sts, filt, bin_mfma);   // the 16x16x64 form: four lanes share a query, four segments per workgroup and query
                if (qs) { seg_geometry(launch_grid, m16 ? 4 : 2, &a.nseg, &a.seg); plan_used_qs = true; plan_qs_m16 = plan_qs_m16 || m16; }
                else
                if (!a.emit_all) seg_geometry(grid, (a.dense ? 8 : 4) / (ag ? 2 : 1), &a.nseg, &a.seg);   // (segments per workgroup: WR, or 2 WR wave halves with DENSE)
                if (fs_stage) {
                    a.fs_stride = sample.sample_stride; a.fs_rows = (uint32_t)h->n; a.gsync = w.gsync; a.Qf = Qf; a.marg2 = w.marg2;
                    a.thr_out = w.thr; a.k = k; a.ip_form = ip_form; a.metric = metric;
                }
                LY_TRY(launch_scan_i8c(a, launch_grid, st, fs_stage, filt, bin_mfma, qs, m16));
                }
            } else {
                a.candB = w.candB; a.segcnt = w.segcnt;
                if (small) {
                    const uint32_t grid = std::min<uint32_t>(a.ntiles, (uint32_t)h->num_cu * 2);
                    if (!a.emit_all) seg_geometry(grid, 4, &a.nseg, &a.seg);
                    LY_TRY((launch_scan_h16<F16_SMALL>(a, metric, grid, st)));
                } else if (const uint32_t sgrid = qh_sample_grid(a, s.sample_tiles, filt, qchunks, level, plan_tile, k, w.cap, (uint32_t)h->num_cu)) {
                    // the threshold-only sample stage on k_scan_qh<.., SMP>: 4 keys per workgroup and query
                    a.ntiles = s.sample_tiles * 4u;
                    LY_TRY(launch_scan_qh_sample(a, metric, sgrid, st));
                    qs_sample_keys = sgrid * 4u;
                    plan_used_qh = true;
                } else if (qh_scan_ok(a, filt, qchunks, level)) {   // the query-stationary tiling of the low-dimensional f16 shadow (scan_qh.h): one segment per workgroup and query
                    uint32_t segs = 0;
                    const uint32_t grid = qh_grid(a, (uint32_t)h->num_cu, &segs);
                    seg_geometry(grid, segs, &a.nseg, &a.seg);
                    plan_used_qh = true;
                    LY_TRY(launch_scan_qh(a, metric, grid, st));
                } else {
                    const uint32_t grid = std::min<uint32_t>(a.ntiles, (uint32_t)h->num_cu);
                    // DENSE epilogue (<4,2,2,4>, L2 / cosine, unfiltered; kernels.h).  Its segments are per wave half.
                    const uint64_t seen_before = s.sample_tiles ? 0 : (sample.sample_tiles ? std::max<uint64_t>((uint64_t)sample.sample_tiles * plan_tile, s.r0) : s.r0);
                    // (since the grouped branches + shared, prefetched norm loads of the DENSE epilogue it beats the two-level filter
                    // at every threshold tightness measured: 1M x 128 and 4M x 128 / 768, k = 10 and 100)
                    a.dense = (!a.emit_all && waves16 == 0 && metric != M_IP && !filt && seen_before) ? 1 : 0;
                    if (!a.emit_all) seg_geometry(grid, (a.dense || waves16 == 3) ? 4 : 2, &a.nseg, &a.seg);
                    if (qchunks > 1 && !(plan.size() == 1 && (a.emit_all == 1 || (assign && a.emit_all == 2))))
                        return set_error(LYNSE_ERR_INTERNAL, "the widened pipeline runs single-stage emit-all plans only");
                    if (waves16 == 3) { LY_TRY((launch_scan_h16<F16_IP_256>(a, metric, grid, st, qchunks))); }
                    else { LY_TRY((launch_scan_h16<F16_L2_256>(a, metric, grid, st, qchunks))); }
                }
            }
            a_emit_all_last = (int)a.emit_all;
            st_nseg = a.seg ? a.nseg : 0; st_seg = a.seg;
            plan_used_segments = plan_used_segments || a.seg != 0;
        }
        if (coarse_dump) return LYNSE_OK;   // (diagnostics: the emit-all stage has written one key per row and query; nothing else runs)
        if (assign) {
            if (a_emit_all_last != 2) return set_error(LYNSE_ERR_INTERNAL, "the assignment scan must run in lane-max mode");
            return LYNSE_OK;   // (k_assign_pick reads the lane-max keys)
        }
        if (tl_prof) {
            LY_HIP(hipEventRecord(e1, st));
            prof->scan_events.push_back({prof->ev_used - 2, s.sample_tiles ? (uint64_t)s.sample_tiles * plan_tile
                                                                  : (uint64_t)(s.r1 - s.r0) + (fs_stage ? (uint64_t)sample.sample_tiles * plan_tile : 0ull)});
        }
        SelectArgs sa{};
        sa.cand = w.cand; sa.count = w.count; sa.overflow = w.overflow; sa.thr = w.thr; sa.marg2 = w.marg2;
        sa.k = k; sa.cap = w.cap; sa.keep_max = w.cap / 2; sa.metric = key_metric; sa.ip_form = ip_form;   // (bin_mfma: best-first +-1 dot products; aug: negated squared L2)
        sa.neg_metric1 = (aug || cosq) ? metric + 1 : 0;
        sa.exact = binary ? 1 : 0;
        // (worth its ~k exact rescorings per query and stage where the margin is wide — the int8 pass — or k is small)
        sa.tighten = (!binary && (i8c || k <= 32)) ? 1 : 0;
        sa.drop_sentinels = (mask && emit_all) ? 1 : 0;
        sa.emit_all_n = emit_all ? (s.sample_tiles ? (int)(s.sample_tiles * plan_tile) : (int)(s.r1 - s.r0)) : -1;
        if (!binary && emit_all && sample_threshold_only) {
            sa.threshold_only = 1;
            sa.drop_sentinels = 1;  // a lane whose rows are all masked / out of range wrote the sentinel
            sa.emit_all_n = qs_sample_keys ? (int)qs_sample_keys : (int)(s.sample_tiles * sample_keys_per_tile);
        }
        sa.Qf = Qf; sa.V = score_rows(h); sa.ld = score_ld(h); sa.D = h->dim;
        sa.candB = w.candB; sa.segcnt = w.segcnt; sa.seg = st_seg; sa.nseg = st_nseg;
        sa.abort_word = fs_stage ? w.gsync + 2 : nullptr;
        if (fused_tail && si + 1 == plan.size()) { sa_last = sa; continue; }  // the last select runs inside k_select_final
        // (round 5, tried: the survivors of the last select handed to the final rescoring in LDS instead of through cand[q] — a store, its
        // acknowledgement and a load less in the tail's chain: 10M 1.8216 / 1.8213 / 1.8527 against 1.8206 / 1.8455 / 1.8381 ms, shard
        // 0.2835 / 0.2875 / 0.2824 against 0.2877 / 0.2884 / 0.2950: nothing, removed again, scripts/gpu_r5_tail1.sh)
        // (round 5, tried: the LAST select without the exact-rescored threshold, its coarse-rule survivors all rescored in the final pass —
        // 116 instead of 35 rows per query, two rounds of the final rescoring: 10M step +10 us, shard step +6 us; dropped)
        sa.lds_bytes = sel_lds_bytes(w.cap, nq);
        hipLaunchKernelGGL(k_select<SEL_NT>, dim3(nq), dim3(SEL_NT), sa.lds_bytes, st, sa);
        LY_HIP(hipGetLastError());
    }
    if (tl_prof && (!binary || bin_mfma)) {   // (batched Hamming on the matrix pipe runs the float pipeline's plans)
        const uint64_t tiling = plan_used_qs ? 0x81u : plan_used_qh ? 0x82u : (small || mid64) ? 0x14u : ((mid128 || waves16 == 3) ? 0x24u : 0x42u);   // (0x81: query-stationary threshold stages; 0x82: those of the low-dimensional f16 shadow, scan_qh.h)
        std::lock_guard<std::mutex> plk(h->prof_mu);
        h->prof.last_plan = (sample.sample_tiles ? 1u : 0u) | ((sample.sample_tiles && sample_threshold_only) ? 2u : 0u) | (i8c ? 4u : 0u) |
                            (plan_used_segments ? 8u : 0u) | (small ? 16u : 0u) | (fs ? 128u : 0u) | ((uint64_t)(plan.size() & 0xff) << 8) | (tiling << 16) |
                            (sts ? (1ull << 24) : 0ull) | (plan_qs_sample ? (1ull << 25) : 0ull) |   // bit 24: self-tightening single-launch scan; bit 25: sample stage on the query-stationary tiling
                            (sq7 ? (1ull << 26) : 0ull) |   // bit 26: the stages read the non-negative 7-bit copy of the codes (SQ7)
                            (predict ? (1ull << 28) : 0ull) |   // bit 28: one threshold stage on a predicted threshold, verified in k_select_final
                            (plan_qs_m16 ? (1ull << 27) : 0ull);   // bit 27: query-stationary threshold stages on v_mfma_i32_16x16x64_i8 (scan_qs.h, M16)
    }
    FinalArgs fa{};
    fa.cand = w.cand; fa.count = w.count; fa.k = k; fa.out_k = out_k; fa.cap = w.cap; fa.metric = key_metric; fa.ip_form = ip_form;
    fa.ham_dim = bin_mfma ? h->dim : 0u;
    fa.neg_metric1 = (aug || cosq) ? metric + 1 : 0;
    fa.exact = binary ? 1 : 0; fa.Qf = Qf; fa.V = score_rows(h); fa.ld = score_ld(h); fa.D = h->dim;
    fa.row_stride = h->row_stride; fa.row_offset = h->row_offset;
    fa.nan_rows = (!binary && !mask && !row_ids && h->n <= 0xffffffffull) ? (uint32_t)h->n : 0u;   // (FinalArgs::nan_rows: the all-NaN query of an unfiltered FLAT search)
    fa.out_rows = rq.out.rows ? rq.out.rows : w.out_rows; fa.out_dists = rq.out.dists ? rq.out.dists : w.out_dists; fa.out_counts = w.out_counts;
    fa.out_counts2 = rq.out.counts2;
    fa.pool_total = tl_prof ? w.pool_total : nullptr;
    fa.overflow = w.overflow; fa.any_overflow = rq.out.any_ovf;
    if (rq.out.hdr_direct) { fa.h_hdr = w.h_hdr; fa.hdr_q = w.qcap; }
    if (fused_tail) {
        TailArgs ta{sa_last, fa, predict ? w.pred_chk : nullptr};
        ta.s.hand_exact = env_int("LYNSE_HIP_HAND_EXACT", 1);   // (0: the final rescoring always reads its rows, A/B)
        ta.s.lds_bytes = ta.f.lds_bytes = sel_lds_bytes(w.cap, nq);
        hipLaunchKernelGGL(k_select_final<SEL_NT>, dim3(nq), dim3(SEL_NT), ta.s.lds_bytes, st, ta);
        LY_HIP(hipGetLastError());
        (void)asc;
        return LYNSE_OK;
    }
    if (i8c && !bin_mfma) {  // a few hundred survivors per query inside the int8 margin: spread their exact rescoring over the chip
        hipLaunchKernelGGL(k_rescore_pool<256>, dim3(nq, 4), dim3(256), 0, st, fa);
        LY_HIP(hipGetLastError());
        fa.exact = 1;
    }
    fa.lds_bytes = sel_lds_bytes(w.cap, nq);
    hipLaunchKernelGGL(k_final<SEL_NT>, dim3(nq), dim3(SEL_NT), fa.lds_bytes, st, fa);
    LY_HIP(hipGetLastError());
    (void)asc;
    return LYNSE_OK;
}

// kmeans::assign_metric (kmeans.rs:237-264) for the device k-means: the nearest centroid of every data row, WITHOUT the general
// top-1 search.  `h` is the centroid store (a widened handle: h->qchunk data rows per pass, <= cap centroids), d_q the data rows in
// device memory.  Per pass of <= qchunk data rows: query image + certified margin (k_prep_queries), ONE lane-max scan over all
// centroid tiles (run_chunk in CHUNK_ASSIGN mode), k_assign_pick.  d_ids[i] = the centroid of row i, or 0xffffffff for the rows whose two
// best coarse centroids lie within the certified margin: their indices come back in d_redo[0 .. *d_redo_count) and the caller answers
// them with the exact top-1 search (lynse_hip_flat_search_f32_device), whose first-strictly-smaller rule they need.
// Returns LYNSE_ERR_UNSUPPORTED when the shape is not the one this path is built for (the caller falls back to the search).
static int flat_assign_top1_device(lynse_hip_flat* h, const float* d_q, uint64_t nq, int metric, uint32_t* d_ids, uint32_t* d_redo,
                                   uint32_t* d_redo_count) {
    if (!h || !d_q || !d_ids || !d_redo || !d_redo_count) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    if (metric < M_IP || metric > M_COS) return set_error(LYNSE_ERR_UNSUPPORTED, "float metrics only");
    LY_WRITER(h, lk);
    LY_TRY(use_device(h));
    if (h->n == 0 || h->n > h->cap || h->qchunk <= QCHUNK || h->packed_only || h->dtype != LYNSE_DTYPE_F32)
        return set_error(LYNSE_ERR_UNSUPPORTED, "not the widened float shape of the assignment pass");
    struct Slot0 { int prev; Slot0() : prev(tl_ctx_slot) { tl_ctx_slot = 0; } ~Slot0() { tl_ctx_slot = prev; } } scope;
    LY_TRY(finalize_locked(h));
    if (metric == M_COS && h->cos_degenerate) return set_error(LYNSE_ERR_UNSUPPORTED, "degenerate norms: the exact search answers");
    LY_TRY(ensure_shadow_locked(h));
    LY_TRY(ensure_workspace(h, 1));
    Workspace& w = cur(h).ws;
    hipStream_t st = cur(h).stream;
    const uint32_t ntiles = (uint32_t)((h->n + 255) / 256);
    const uint32_t nkeys = ntiles * ((metric == M_IP) ? 16u : 8u);   // 2 WR lanes per tile and data row x their best two (<2,4,4,2> / <4,2,2,4>)
    if (nkeys > w.cap) return set_error(LYNSE_ERR_UNSUPPORTED, "lane-max keys exceed the candidate slots");
    LY_HIP(hipMemsetAsync(d_redo_count, 0, 4, st));
    ScanProf sprof;
    ChunkReq rq;
    rq.k = rq.out_k = 1; rq.metric = metric; rq.allow_sts = false; rq.mode = CHUNK_ASSIGN;
    const bool prof_prev = tl_prof;
    tl_prof = false;
    int rc = LYNSE_OK;
    for (uint64_t q0 = 0; q0 < nq && rc == LYNSE_OK; q0 += w.qcap) {
        const uint32_t nqc = (uint32_t)std::min<uint64_t>(w.qcap, nq - q0);
        rq.nq = nqc; rq.qsrc = d_q + q0 * h->dim;
        rc = run_chunk(h, rq, st, &sprof);
        if (rc != LYNSE_OK) break;
        int ip_form = h->ip_form;
        if (ip_form == LYNSE_IPFORM_AUTO) ip_form = h->n < 4096 ? LYNSE_IPFORM_SINGLE : LYNSE_IPFORM_BATCH8;   // (run_chunk's rule)
        hipLaunchKernelGGL(k_assign_pick, dim3((nqc + 3) / 4), dim3(256), 0, st, w.cand, w.cap, nkeys, w.marg2, metric_ascending(metric) ? 1 : 0,
                           nqc, (uint32_t)q0, d_ids, d_redo, d_redo_count, d_q, score_rows(h), score_ld(h), h->dim, metric, ip_form);
        if (hipGetLastError() != hipSuccess) rc = set_error(LYNSE_ERR_DEVICE, "k_assign_pick launch failed");
    }
    tl_prof = prof_prev;
    if (rc != LYNSE_OK) { (void)hipStreamSynchronize(st); return rc; }
    LY_HIP(hipStreamSynchronize(st));
    return LYNSE_OK;
}

// The fused single-launch search (k_small_search): a few queries over a shard small enough that the eight dependent
// launches of the staged pipeline, not the bytes, are the cost.  Exact scores straight from the f32 rows.
static bool small_path_ok(const lynse_hip_flat* h, uint64_t nq, uint32_t kk, int metric, bool filtered) {
    static const uint64_t max_bytes = (uint64_t)env_int("LYNSE_HIP_FUSED_MAX_MB", 64) << 20;
    return fused_env() && !h->no_fused && metric <= M_COS && !filtered && h->dtype == LYNSE_DTYPE_F32 && !h->packed_only && nq <= (uint64_t)SMALL_MAX_Q &&
           kk <= (uint32_t)SMALL_MAX_K && (uint64_t)h->n * h->ld * 4 * nq <= max_bytes &&
           (size_t)((h->dim + 3) / 4 * 4) * 4 + (size_t)128 * 1024 + 64 <= 150u * 1024u;
}

// SmallRows: the row matrix a fused search scans when it is not the handle's own (IVF: the centroid matrix, the slab with
// its row map); SmallIvf: the probed-lists mode of k_small_search.
struct SmallRows { const float* V; uint32_t ld; uint64_t n; int ip_form; uint64_t row_stride, row_offset; };
struct SmallIvf { const uint64_t* probes; uint32_t nprobe, nlist; const uint64_t* list_off; const uint32_t* orig; int flag_empty; };

static int run_small(lynse_hip_flat* h, uint32_t nq, uint32_t k, uint32_t out_k, int metric, hipStream_t st, ScanProf* prof, uint64_t* r_dst, float* d_dst, uint32_t* c_dst, uint32_t* o_dst,
                     const float* d_q, const SmallRows* rows = nullptr, const SmallIvf* ivf = nullptr) {
    // r_dst / d_dst / c_dst / o_dst: where the last workgroup writes rows, distances, counts and overflow flags — the
    // caller's device buffers, or pinned host memory (device-visible): no copy kernels behind the search
    Workspace& w = cur(h).ws;
    SmallArgs a{};
    a.V = h->rows; a.ld = h->ld; a.D = h->dim; a.n = (uint32_t)h->n; a.Qf = d_q; a.nq = nq; a.k = k; a.out_k = out_k; a.metric = metric;
    int ip_form = h->ip_form;
    if (ip_form == LYNSE_IPFORM_AUTO) ip_form = h->n < 4096 ? LYNSE_IPFORM_SINGLE : LYNSE_IPFORM_BATCH8;  // flat_mmap.rs:4852-4854
    a.ip_form = ip_form;
    a.row_stride = h->row_stride; a.row_offset = h->row_offset;
    uint64_t n_scan = h->n;  // rows one query scans (IVF mode: an upper bound, for the grid size only)
    if (rows) { a.V = rows->V; a.ld = rows->ld; a.n = (uint32_t)rows->n; a.ip_form = rows->ip_form; a.row_stride = rows->row_stride; a.row_offset = rows->row_offset; n_scan = rows->n; }
    if (ivf) { a.probes = ivf->probes; a.nprobe = ivf->nprobe; a.nlist = ivf->nlist; a.list_off = ivf->list_off; a.orig = ivf->orig; a.flag_empty = ivf->flag_empty; }
    a.part = w.small_part; a.ticket = w.small_ticket;
    a.out_rows = r_dst; a.out_dists = d_dst; a.out_counts = c_dst; a.overflow = o_dst;
    // two workgroups per CU (16 waves: the scan is a chain of dependent load batches per wave), one merge list per workgroup:
    // at most SMALL_NT lists (one per thread of the last workgroup) and 128 KB of them in the hand-over buffer
    uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>((uint64_t)std::min(2 * h->num_cu, SMALL_NT), 16384u / std::max<uint32_t>(k, 1)), (n_scan + 127) / 128));
    {   // whole passes for every workgroup (a pass = 128 rows per workgroup): 100k rows over 512 workgroups are 1.53 passes — half of the
        // workgroups idle through the second one and all 512 queue at the ticket; 391 workgroups x 2 passes: kernel 21.4 -> 19.7 us
        const uint64_t passes = (n_scan + (uint64_t)grid * 128 - 1) / ((uint64_t)grid * 128);
        if (passes > 1) grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(grid, (n_scan + 128 * passes - 1) / (128 * passes)));
    }
    auto pow2_at_least = [](uint32_t v) { uint32_t p = 2; while (p < v) p <<= 1; return p; };
    const size_t lds = (size_t)((h->dim + 3) / 4 * 4) * 4 + (size_t)SMALL_NT * 8 + (size_t)pow2_at_least(std::min<uint32_t>(k, grid) * k) * 8 + 64;  // the query, the wave lists (later the heads of the merge), the merge's candidate keys
    LY_TRY(ensure_lds<k_small_search>(160 * 1024 - 1024));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    const bool timed = tl_prof && prof;
    if (timed) {
        LY_TRY(get_event(h, prof->ev_used++, &e0));
        LY_TRY(get_event(h, prof->ev_used++, &e1));
        LY_HIP(hipEventRecord(e0, st));
    }
    hipLaunchKernelGGL(k_small_search, dim3(grid), dim3(SMALL_NT), lds, st, a);
    LY_HIP(hipGetLastError());
    if (timed) {
        LY_HIP(hipEventRecord(e1, st));
        prof->scan_events.push_back({prof->ev_used - 2, (uint64_t)h->n * nq});
        std::lock_guard<std::mutex> plk(h->prof_mu);
        h->prof.last_plan = 32u | (1u << 8);  // bit 5: fused single-launch search
    }
    return LYNSE_OK;
}

// ------------------------------------------------------------------------------ SQ8 two-pass ----
// ensure_sq8 (flat_mmap.rs:375-386) + SQ8Data::from_f32_parallel (:5685-5737): (re)built over ALL rows whenever rows were
// appended since the last build (min / max are collection-wide).
// Rows appended to a shard that already has its codes (Collection::flush hands over <= 10,000 rows at a time, src/engine.rs:93-94):
// the new rows' per-dimension min / max are MERGED into the stored table; when no entry moves, the collection-wide fit — and with
// it every existing code — is what a full rebuild would produce (SQ8Data::from_f32_parallel, flat_mmap.rs:5685-5737, fits min / max
// over all rows), so only the new rows are quantised (and the max row L1 norm / the non-finite count keep accumulating).  A moved
// entry means new scales: everything is coded again, from the already merged table.  Returns the first row that still needs codes
// (0 = all of them) and whether `mm` already covers every row.
static int sq8_merge_new_rows(lynse_hip_flat* h, uint32_t* mm, uint32_t D, uint64_t n_done, const float* row_scale, uint64_t* first_row, bool* mm_covers_all) {
    *first_row = 0;
    *mm_covers_all = false;
    if (n_done == 0 || n_done >= h->n) return LYNSE_OK;
    if (!h->sq8_mm_prev) LY_HIP(hipMalloc(&h->sq8_mm_prev, ((size_t)(h->dim + 64) * 2 + 1) * 4));
    hipStream_t st = cur(h).stream;
    uint32_t* flag = h->sq8_mm_prev + 2 * (size_t)D;
    LY_HIP(hipMemcpyAsync(h->sq8_mm_prev, mm, (size_t)D * 8, hipMemcpyDeviceToDevice, st));
    LY_HIP(hipMemsetAsync(flag, 0, 4, st));
    const uint64_t nn = h->n - n_done;
    const uint32_t gx = (D + 255) / 256;
    const uint32_t gy = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(nn / 256, 1), (uint64_t)h->num_cu * 8);
    if (is_f16(h)) hipLaunchKernelGGL(k_sq8_minmax<_Float16>, dim3(gx, gy), dim3(256), 0, st, (const _Float16*)h->rows_h + n_done * h->ld16, h->ld16, D, nn, mm, mm + D,
                                      row_scale ? row_scale + n_done : nullptr);
    else hipLaunchKernelGGL(k_sq8_minmax<float>, dim3(gx, gy), dim3(256), 0, st, h->rows + n_done * h->ld, h->ld, D, nn, mm, mm + D, row_scale ? row_scale + n_done : nullptr);
    hipLaunchKernelGGL(k_mm_changed, dim3((2 * D + 255) / 256), dim3(256), 0, st, mm, h->sq8_mm_prev, 2 * D, flag);
    LY_HIP(hipGetLastError());
    uint32_t moved = 1;
    LY_HIP(hipMemcpyAsync(&moved, flag, 4, hipMemcpyDeviceToHost, st));
    LY_HIP(hipStreamSynchronize(st));
    *mm_covers_all = true;
    if (!moved) *first_row = n_done;
    return LYNSE_OK;
}

// LYNSE_HIP_PREDICT: the predicted first threshold of the certified int8 pass (predict.h): 0 = never, 1 = wherever the shape is
// eligible, unset = auto (read per call: tests flip it)
static int predict_env() { return env_int("LYNSE_HIP_PREDICT", -1); }
// auto: from this many rows on.  Forced, the plan gains at every measured shard size (profiles/predict_size_sweep.json: 1.25M / 2.4M / 4M /
// 6M / 8M / 10M rows gain 36 / 61 / 58 / 38 / 37 / 56 us per step, each beyond three times the spread of its runs); the plans the tests pin
// without a knob go up to 2.4M rows, so auto starts at the next measured size.
static const uint64_t PREDICT_AUTO_MIN_ROWS = 4000000ull;
static bool predict_size_ok(const lynse_hip_flat* h) { const int e = predict_env(); return e == 1 || (e != 0 && h->n >= PREDICT_AUTO_MIN_ROWS); }

// Brings the column statistics of a code set up to date with its codes: the sums take in rows colsum_n .. n (all of them after a new
// fit, which resets colsum_n), then mu / sigma^2 are formed on the host and uploaded.  Synchronises the stream.
static int code_stats_locked(lynse_hip_flat* h, CodeSet& s) {
    if (!s.codes || s.n == 0 || s.ld % 4 != 0 || s.stats_ready()) return LYNSE_OK;
    hipStream_t st = cur(h).stream;
    const uint32_t DC = s.cols;
    if (!s.colsum) {
        LY_HIP(hipMalloc(&s.colsum, (size_t)DC * 16));
        LY_HIP(hipMalloc(&s.mu, (size_t)DC * 8));
        LY_HIP(hipMalloc(&s.var, (size_t)DC * 8));
        s.colsum_n = 0;
    }
    if (s.colsum_n > s.n) s.colsum_n = 0;
    if (s.colsum_n == 0) LY_HIP(hipMemsetAsync(s.colsum, 0, (size_t)DC * 16, st));
    const uint64_t nn = s.n - s.colsum_n;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((nn + 1023) / 1024, (uint64_t)h->num_cu * 8);
    hipLaunchKernelGGL(k_code_colsums, dim3(grid), dim3(256), 0, st, s.codes + s.colsum_n * s.ld, s.ld, DC, nn, s.colsum);
    LY_HIP(hipGetLastError());
    std::vector<long long> sums((size_t)DC * 2);
    LY_HIP(hipMemcpyAsync(sums.data(), s.colsum, (size_t)DC * 16, hipMemcpyDeviceToHost, st));
    LY_HIP(hipStreamSynchronize(st));
    s.h_mu.resize(DC); s.h_var.resize(DC);
    predict_col_stats(sums.data(), DC, s.n, s.h_mu.data(), s.h_var.data());
    LY_HIP(hipMemcpyAsync(s.mu, s.h_mu.data(), (size_t)DC * 8, hipMemcpyHostToDevice, st));
    LY_HIP(hipMemcpyAsync(s.var, s.h_var.data(), (size_t)DC * 8, hipMemcpyHostToDevice, st));
    LY_HIP(hipStreamSynchronize(st));
    s.colsum_n = s.n;
    return LYNSE_OK;
}

// The tail every code-set builder shares: rows r0 .. n of `s` are coded (k_sq8_quantize, minima `mins`, the set's own scales), the four
// stats words come back into a1 / a2sq / eps2 / finite and the set covers the shard; the column statistics of the predicted threshold
// follow where a shard of this size may use them (not for the augmented rows of the L2 form).  Synchronises the stream.
static int quantize_rows_locked(lynse_hip_flat* h, CodeSet& s, uint64_t r0, const float* mins, const float* extra_col, uint32_t n_extra,
                                const float* row_scale, int sq7) {
    hipStream_t st = cur(h).stream;
    const uint64_t nn = h->n - r0;
    const uint32_t qgrid = (uint32_t)std::min<uint64_t>((nn + 3) / 4, (uint64_t)h->num_cu * 16);
    int8_t* out = s.codes + r0 * s.ld;
    int *sum = s.sum ? s.sum + r0 : nullptr, *sum2 = s.sum2 ? s.sum2 + r0 : nullptr;
    if (extra_col) extra_col += r0;
    if (row_scale) row_scale += r0;
    if (is_f16(h)) hipLaunchKernelGGL(k_sq8_quantize<_Float16>, dim3(qgrid), dim3(256), 0, st, (const _Float16*)h->rows_h + r0 * h->ld16, h->ld16, h->dim, nn,
                                      mins, s.scales, out, s.ld, sum, sum2, s.stats, extra_col, n_extra, row_scale, sq7);
    else hipLaunchKernelGGL(k_sq8_quantize<float>, dim3(qgrid), dim3(256), 0, st, h->rows + r0 * h->ld, h->ld, h->dim, nn,
                            mins, s.scales, out, s.ld, sum, sum2, s.stats, extra_col, n_extra, row_scale, sq7);
    LY_HIP(hipGetLastError());
    uint32_t qst[4] = {0, 0, 0, 0};
    LY_HIP(hipMemcpyAsync(qst, s.stats, 16, hipMemcpyDeviceToHost, st));
    LY_HIP(hipStreamSynchronize(st));
    s.a1 = qst[0];
    s.a2sq = qst[2];
    memcpy(&s.eps2, &qst[3], 4);
    s.finite = qst[1] == 0;
    s.n = h->n;
    if (r0 == 0) { s.colsum_n = 0; if (!extra_col) h->predict_strikes.store(0); }   // a new fit: the sums start again, and so does the model's record
    if (!extra_col && s.finite && predict_size_ok(h)) LY_TRY(code_stats_locked(h, s));
    return LYNSE_OK;
}

// What tells the three fitted code sets apart (ensure_codes_locked).
struct CodeForm {
    bool norm_cols;     // columns dim .. cols - 1 of the coded row hold its squared norm (vn2): the augmented rows of the L2 form
    bool unit_rows;     // the coded row is v * vrinv[row]: the cosine form
    bool incremental;   // rows appended inside the fitted ranges are coded alone (sq8_merge_new_rows); otherwise every append refits
    bool keeps_sums;    // per-row sums of the codes (FLAT-*-SQ8)
    bool bumps_fit;     // a new fit counts in sq8_fit (the SQ7 copy follows it)
};
static constexpr CodeForm CODES_PLAIN{false, false, true, true, true};
static constexpr CodeForm CODES_AUG{true, false, false, false, false};
static constexpr CodeForm CODES_UNIT{false, true, true, false, false};

// Brings a fitted code set up to date with the rows: (re)allocation, per-column min / max over all rows — or merged from the appended
// rows alone —, minima + scales, codes.
static int ensure_codes_locked(lynse_hip_flat* h, CodeSet& s, const CodeForm& f) {
    if (s.ready(h->n)) return LYNSE_OK;
    hipStream_t st = cur(h).stream;
    const uint32_t D = h->dim, DC = s.cols;
    const float* row_scale = f.unit_rows ? h->vrinv : nullptr;
    const bool kept = f.incremental && s.codes != nullptr && s.mins != nullptr && s.cap >= h->n;   // the existing codes survive (no reallocation)
    if (s.cap < h->n) {
        s.release();
        const uint64_t cap = std::max<uint64_t>(h->capacity, h->n);
        LY_HIP(hipMalloc(&s.codes, (size_t)cap * s.ld + 256));
        if (f.keeps_sums) {
            LY_HIP(hipMalloc(&s.sum, ((size_t)cap + 256) * 4));
            LY_HIP(hipMalloc(&s.sum2, ((size_t)cap + 256) * 4));
            LY_HIP(hipMemsetAsync(s.sum, 0, ((size_t)cap + 256) * 4, st));
            LY_HIP(hipMemsetAsync(s.sum2, 0, ((size_t)cap + 256) * 4, st));
        }
        s.cap = cap;
    }
    if (!s.mins) {
        LY_HIP(hipMalloc(&s.mins, (size_t)DC * 4));
        LY_HIP(hipMalloc(&s.scales, (size_t)DC * 4));
        LY_HIP(hipMalloc(&s.mm, (size_t)DC * 8));
        LY_HIP(hipMalloc(&s.stats, 16));   // (four words: k_sq8_quantize)
    }
    uint64_t r0 = 0;
    bool mm_done = false;
    if (kept) LY_TRY(sq8_merge_new_rows(h, s.mm, DC, s.n, row_scale, &r0, &mm_done));   // (appended rows inside the fitted ranges: only they are coded)
    std::vector<uint32_t> init;
    if (!mm_done) {
        init.resize((size_t)DC * 2);
        for (uint32_t d = 0; d < DC; ++d) { init[d] = f32_to_ord(INFINITY); init[DC + d] = f32_to_ord(-INFINITY); }
        LY_HIP(hipMemcpyAsync(s.mm, init.data(), init.size() * 4, hipMemcpyHostToDevice, st));
        const uint32_t gx = (D + 255) / 256;
        const uint32_t gy = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(h->n / 256, 1), (uint64_t)h->num_cu * 8);
        if (is_f16(h)) hipLaunchKernelGGL(k_sq8_minmax<_Float16>, dim3(gx, gy), dim3(256), 0, st, (const _Float16*)h->rows_h, h->ld16, D, h->n, s.mm, s.mm + DC, row_scale);
        else hipLaunchKernelGGL(k_sq8_minmax<float>, dim3(gx, gy), dim3(256), 0, st, h->rows, h->ld, D, h->n, s.mm, s.mm + DC, row_scale);
        if (f.norm_cols)
            hipLaunchKernelGGL(k_vec_minmax, dim3((uint32_t)std::min<uint64_t>((h->n + 255) / 256, (uint64_t)h->num_cu * 8)), dim3(256), 0, st,
                               h->vn2, h->n, s.mm + D, s.mm + DC + D, DC - D);
    }
    if (r0 == 0) {   // a new fit: every row is coded (again)
        if (f.bumps_fit) ++h->sq8_fit;
        LY_HIP(hipMemsetAsync(s.stats, 0, 16, st));
        hipLaunchKernelGGL(k_sq8_scales, dim3((DC + 255) / 256), dim3(256), 0, st, s.mm, s.mm + DC, DC, s.mins, s.scales, 255.0f);
    }
    return quantize_rows_locked(h, s, r0, s.mins, f.norm_cols ? h->vn2 : nullptr, DC - D, row_scale, 0);   // (synchronises: `init` is a temporary)
}
static int ensure_sq8_locked(lynse_hip_flat* h) { return ensure_codes_locked(h, h->sq8, CODES_PLAIN); }

// LYNSE_HIP_SQ7: 0 = never, 1 = wherever the shape is eligible (any shard size, any sign), unset = auto (read per call: tests flip it)
static int sq7_env() { return env_int("LYNSE_HIP_SQ7", -1); }
// auto: from this many rows on — the smallest measured shard at which the gain of the whole step passes the three-spreads rule
// (profiles/sq7_bench_ab.json: LYNSE_HIP_SQ7=0 against 1 at 2.4M / 4M / 6M / 8M rows gains 5 / 19 / 43 / 52 us, each short of three times
// the spread of its runs (8M: 52.2 us); the 10M step gains 80 us against 58).  It loses nowhere from 2.4M rows on; LYNSE_HIP_SQ7=1 forces it.
static const uint64_t SQ7_AUTO_MIN_ROWS = 10000000ull;
// Does a FLAT-IP batch of nqc queries over this shard scan the SQ7 copy?  The query-stationary tiling with more than 128 queries, whole
// 128-column slabs; auto: only over non-negative rows (the host cannot see the sign of a device-resident batch: non-negative rows are
// the proxy for non-negative queries — a mixed-sign batch over them is still answered exactly, without the gain).
static bool sq7_wanted(const lynse_hip_flat* h, int metric, uint64_t nqc, bool masked) {
    const int e = sq7_env();
    if (e == 0 || metric != M_IP || masked || nqc <= 128 || nqc > QCHUNK || h->qchunk > QCHUNK) return false;
    if (qs_variant() < 1 || qs_variant() > 3 || !qs_width_ok(h->ld8, (h->dim + 127) / 128, false)) return false;
    if (sts_env_on() || fused_sample_env() != 0) return false;   // (those plans keep the SQ8 codes)
    if (h->sq7_strikes.load() >= 3) return false;
    return e == 1 || (h->rows_nonneg && h->n >= SQ7_AUTO_MIN_ROWS);
}
// The copy only changes speed: a shape that scans it gets it built here (writer lock), and a build that fails — no memory for one more byte
// per element — leaves the batch on the SQ8 codes and switches SQ7 off for the handle.  A copy the handle will not scan again (struck
// out, or rows that turned mixed-sign under auto) is freed.
static bool sq7_stale(const lynse_hip_flat* h) { return h->sq7.codes && (h->sq7_strikes.load() >= 3 || (!h->rows_nonneg && sq7_env() != 1)); }
static int ensure_sq7_locked(lynse_hip_flat* h);
static void sq7_sync_locked(lynse_hip_flat* h, int metric, uint64_t nqc, bool masked) {
    if (sq7_stale(h)) h->sq7.release();
    if (!sq7_wanted(h, metric, nqc, masked) || !h->sq8.ready(h->n) || !h->sq8.finite) return;
    if (ensure_sq7_locked(h) != LYNSE_OK) {
        (void)hipGetLastError();
        h->sq7.release();
        h->sq7_strikes.store(3);
    }
}
// The SQ7 copy, from the fit of the SQ8 codes (which must be up to date): rows appended under an unchanged fit are coded alone and
// raise the maxima; a new fit codes every row again.  (Callers: sq7_sync_locked.)
static int ensure_sq7_locked(lynse_hip_flat* h) {
    CodeSet& s = h->sq7;
    if (s.ready(h->n) && h->sq7_fit == h->sq8_fit) return LYNSE_OK;
    if (!h->sq8.ready(h->n)) return set_error(LYNSE_ERR_INTERNAL, "the SQ7 copy is built from the fit of up-to-date SQ8 codes");
    hipStream_t st = cur(h).stream;
    const bool kept = s.codes != nullptr && s.cap >= h->n && h->sq7_fit == h->sq8_fit && s.n < h->n;
    if (s.cap < h->n) {
        s.release();
        const uint64_t cap = std::max<uint64_t>(h->capacity, h->n);
        LY_HIP(hipMalloc(&s.codes, (size_t)cap * s.ld + 256));
        s.cap = cap;
    }
    if (!s.scales) {
        LY_HIP(hipMalloc(&s.scales, (size_t)s.cols * 4));
        LY_HIP(hipMalloc(&s.stats, 16));
    }
    const uint64_t r0 = kept ? s.n : 0;
    if (r0 == 0) {
        LY_HIP(hipMemsetAsync(s.stats, 0, 16, st));
        hipLaunchKernelGGL(k_sq8_scales, dim3((s.cols + 255) / 256), dim3(256), 0, st, h->sq8.mm, h->sq8.mm + s.cols, s.cols, (float*)nullptr, s.scales, 127.0f);
    }
    LY_TRY(quantize_rows_locked(h, s, r0, h->sq8.mins, nullptr, 0u, nullptr, 1));
    h->sq7_fit = h->sq8_fit;
    return LYNSE_OK;
}
static bool sq7_ready(const lynse_hip_flat* h) { return h->sq7.ready(h->n) && h->sq7_fit == h->sq8_fit && h->sq8.ready(h->n); }

// Does a batch of nqc queries over this shard run the predicted plan (run_chunk)?  The shapes the query-stationary tiling answers with
// more than 128 queries — IP and cosine, whole 128-column slabs, k <= 32 —, unmasked; a shard large enough that the C keys per query
// the threshold aims at are a far tail of its rows; not beside the self-tightening or fused-sample plans; not after three strikes.
// LYNSE_HIP_PREDICT_C: the target key count per query in units of k (A/B; default 40, the best of profiles/predict_c_sweep.json).
static double predict_keys_per_query(uint32_t k) { return (double)std::max(1, env_int("LYNSE_HIP_PREDICT_C", 40)) * (double)k; }
static bool predict_wanted(const lynse_hip_flat* h, int metric, uint64_t nqc, uint32_t k, bool masked) {
    if (predict_env() == 0 || (metric != M_IP && metric != M_COS) || masked || nqc <= 128 || nqc > QCHUNK || h->qchunk > QCHUNK) return false;
    if (k < 1 || k > 32 || h->n < 65536 || (double)h->n < 8.0 * predict_keys_per_query(k)) return false;
    if (qs_variant() < 1 || qs_variant() > 3 || !qs_width_ok(h->ld8, (h->dim + 127) / 128, false)) return false;
    if (sts_env_on() || fused_sample_env() != 0) return false;
    if (h->predict_strikes.load() >= 3) return false;
    return predict_size_ok(h);
}
// The code set a predicted chunk of this shape would read, as run_chunk picks it.
static CodeSet& predict_code_set(lynse_hip_flat* h, int metric, uint64_t nqc) {
    if (sq7_wanted(h, metric, nqc, false) && sq7_ready(h)) return h->sq7;
    return metric == M_COS ? h->sq8c : h->sq8;
}
// Statistics only change speed: a shape that wants them gets them built here (writer lock), after the code sets themselves.
static int predict_sync_locked(lynse_hip_flat* h, int metric, uint64_t nqc, uint32_t k, bool masked) {
    if (!predict_wanted(h, metric, nqc, k, masked)) return LYNSE_OK;
    CodeSet& s = predict_code_set(h, metric, nqc);
    if (!s.ready(h->n) || !s.finite) return LYNSE_OK;
    return code_stats_locked(h, s);
}

extern "C" int lynse_hip_flat_sq8_params(lynse_hip_flat* h, float* mins, float* scales) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    LY_WRITER(h, lk);
    LY_TRY(use_device(h));
    if (h->packed_only || h->n == 0) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "no f32 rows");
    LY_TRY(finalize_locked(h));
    LY_TRY(ensure_sq8_locked(h));
    if (mins) LY_HIP(hipMemcpy(mins, h->sq8.mins, (size_t)h->dim * 4, hipMemcpyDeviceToHost));
    if (scales) LY_HIP(hipMemcpy(scales, h->sq8.scales, (size_t)h->dim * 4, hipMemcpyDeviceToHost));
    return LYNSE_OK;
}

// sq8_two_pass_search (flat_mmap.rs:5868-5926) for one chunk of <= 256 queries (queries in ws.Qf): pass 1 = exact integer
// scores of the u8 codes on the i8 MFMA, exact top-n_cand in (score, row) order with the staged strict thresholds of the
// packed-binary path; pass 2 = exact f32 rescoring of the n_cand rows, (distance, row) order, top k.
static int run_chunk_sq8(lynse_hip_flat* h, uint32_t nq, uint32_t k, uint32_t out_k, uint32_t n_cand, int metric, int level, hipStream_t st,
                         bool pass1_only = false) {
    // pass1_only: stop after pass 1 — the outputs are the top-k rows by the integer score of the codes, in (score, row) order,
    // with that score as the distance (the large-n_cand path merges such lists over row ranges; tests look at the ranking)
    Workspace& w = cur(h).ws;
    const bool ip = metric == M_IP;
    const int m1 = ip ? M_IP : M_L2;  // cosine ranks the codes by squared L2 too (:5887-5890)
    const uint32_t nslab = (h->dim + 127) / 128, qpad = SCAN_BQ_LARGE;
    LY_TRY(ensure_lds<k_select<SEL_NT>>(SEL_LDS_MAX));
    LY_TRY(ensure_lds<k_final<SEL_NT>>(SEL_LDS_MAX));
    LY_HIP(hipMemsetAsync(w.Q16, 0, (size_t)nslab * qpad * 128, st));
    hipLaunchKernelGGL(k_sq8_prep_queries, dim3(nq), dim3(256), 0, st, w.Qf, h->dim, qpad, nslab, h->sq8.mins, h->sq8.scales,
                       reinterpret_cast<int8_t*>(w.Q16), w.qn2, w.thr, w.count, w.overflow, ip ? 1 : 0);
    LY_HIP(hipGetLastError());
    const std::vector<Stage> plan = make_plan(h, n_cand, level >= 2 ? 2 : 1, 0);  // contiguous stages: rows in ascending order
    for (size_t si = 0; si < plan.size(); ++si) {
        const Stage s = plan[si];
        ScanArgs a{};
        a.V16 = reinterpret_cast<const _Float16*>(h->sq8.codes); a.ld16 = h->sq8.ld; a.D = h->dim; a.row0 = s.r0; a.row1 = s.r1;
        a.Q16 = w.Q16; a.qpad = qpad; a.nq = nq; a.nslab = nslab; a.ntiles = (s.r1 - s.r0 + 255) / 256;
        a.qinv = w.qinv; a.qn2 = w.qn2; a.qrinv = w.qrinv; a.thr = w.thr;
        a.vn2 = reinterpret_cast<const float*>(ip ? h->sq8.sum : h->sq8.sum2); a.vrinv = a.vn2;
        a.sv = 1.0f; a.cand = w.cand; a.count = w.count; a.cap = w.cap; a.emit_all = si == 0 ? 1 : 0;
        const uint32_t grid = std::min<uint32_t>(a.ntiles, (uint32_t)h->num_cu);
        a.candB = w.candB; a.segcnt = w.segcnt;
        if (!a.emit_all) seg_geometry(grid, 2, &a.nseg, &a.seg);
        constexpr H16Cfg SQ8 = with(F16_L2_256, &H16Cfg::i8q, 1);   // integer scores of the u8 codes (kernels.h, I8Q = 1); may end in a ragged slab
        if (ip) LY_TRY((launch_h16<with(SQ8, &H16Cfg::metric, M_IP)>(grid, st, a)));
        else LY_TRY((launch_h16<SQ8>(grid, st, a)));
        SelectArgs sa{};
        sa.cand = w.cand; sa.count = w.count; sa.overflow = w.overflow; sa.thr = w.thr; sa.marg2 = w.marg2;
        sa.k = n_cand; sa.cap = w.cap; sa.keep_max = w.cap / 2; sa.metric = m1; sa.ip_form = LYNSE_IPFORM_SINGLE;
        sa.exact = 1; sa.emit_all_n = si == 0 ? (int)(s.r1 - s.r0) : -1;
        sa.Qf = w.Qf; sa.V = h->rows; sa.ld = h->ld; sa.D = h->dim;
        sa.candB = w.candB; sa.segcnt = w.segcnt; sa.seg = a.seg; sa.nseg = a.seg ? a.nseg : 0;
        sa.lds_bytes = sel_lds_bytes(w.cap, nq);
        hipLaunchKernelGGL(k_select<SEL_NT>, dim3(nq), dim3(SEL_NT), sa.lds_bytes, st, sa);
        LY_HIP(hipGetLastError());
    }
    FinalArgs fa{};
    fa.cand = w.cand; fa.count = w.count; fa.k = k; fa.out_k = out_k; fa.cap = w.cap; fa.metric = metric;
    fa.ip_form = LYNSE_IPFORM_SINGLE;  // pass 2 uses simd::inner_product_f32 & co (:5899-5906)
    fa.exact = 0; fa.Qf = w.Qf; fa.V = h->rows; fa.ld = h->ld; fa.D = h->dim;
    fa.row_stride = h->row_stride; fa.row_offset = h->row_offset;
    fa.out_rows = w.out_rows; fa.out_dists = w.out_dists; fa.out_counts = w.out_counts; fa.pool_total = nullptr;
    if (pass1_only || env_on("LYNSE_HIP_SQ8_PASS1", false)) {   // (tests: return the pass-1 ranking (integer scores) instead of rescoring; read per call)
        fa.metric = m1;
    } else {
        hipLaunchKernelGGL(k_rescore_pool<256>, dim3(nq, nq >= 64 ? 4 : 32), dim3(256), 0, st, fa);
        LY_HIP(hipGetLastError());
    }
    fa.exact = 1;
    fa.lds_bytes = sel_lds_bytes(w.cap, nq);
    hipLaunchKernelGGL(k_final<SEL_NT>, dim3(nq), dim3(SEL_NT), fa.lds_bytes, st, fa);
    LY_HIP(hipGetLastError());
    return LYNSE_OK;
}

static int search_sq8_large(lynse_hip_flat* h, std::unique_lock<std::shared_mutex>& lk, const float* queries, uint64_t nq, uint32_t k, uint32_t kk,
                            uint32_t n_cand, int metric, uint64_t* out_rows, float* out_dists, uint32_t* out_counts);

extern "C" int lynse_hip_flat_search_sq8_f32(lynse_hip_flat* h, const float* queries, uint64_t nq, uint32_t k, int metric,
                                             uint64_t* out_rows, float* out_dists, uint32_t* out_counts) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    LY_TRY(metric_check(metric));
    // use_sq8 only changes ip / l2 / cosine (flat_mmap.rs:891-896); every other metric takes the ordinary path
    if (metric > M_COS) return lynse_hip_flat_search_f32(h, queries, nq, k, metric, out_rows, out_dists, out_counts);
    if (nq == 0) return LYNSE_OK;
    if (!queries || !out_counts || (k && (!out_rows || !out_dists))) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    LY_WRITER(h, lk);
    LY_TRY(use_device(h));
    if (h->packed_only) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "store holds packed rows; float metrics unavailable");
    if (h->dtype != LYNSE_DTYPE_F32) return set_error(LYNSE_ERR_UNSUPPORTED, "SQ8 mode on an F16 shard is not supported");
    if (h->n == 0 || k == 0) { memset(out_counts, 0, nq * 4); return LYNSE_OK; }
    const uint32_t kk = (uint32_t)std::min<uint64_t>(k, h->n);
    uint64_t n_cand = metric == M_COS ? std::max<uint64_t>((uint64_t)kk * 100, 500) : std::max<uint64_t>((uint64_t)kk * 20, 200);  // :5883-5893
    n_cand = std::min<uint64_t>(n_cand, h->n);
    LY_TRY(finalize_locked(h));
    LY_TRY(ensure_workspace(h, k));
    LY_TRY(ensure_sq8_locked(h));
    if (h->n > h->cap && n_cand > h->cap / 4)  // more candidates than one pass holds: row ranges + host merge (search_sq8_large)
        return search_sq8_large(h, lk, queries, nq, k, kk, (uint32_t)n_cand, metric, out_rows, out_dists, out_counts);
    Workspace& w = cur(h).ws;
    hipStream_t st = cur(h).stream;
    for (uint64_t q0 = 0; q0 < nq; q0 += QCHUNK) {
        const uint32_t nqc = (uint32_t)std::min<uint64_t>(QCHUNK, nq - q0);
        LY_HIP(hipMemcpyAsync(w.Qf, queries + q0 * h->dim, (size_t)nqc * h->dim * 4, hipMemcpyHostToDevice, st));
        for (int level = 1; level < 3; ++level) {
            LY_TRY(run_chunk_sq8(h, nqc, kk, k, (uint32_t)n_cand, metric, level, st));
            LY_HIP(hipMemcpyAsync(out_rows + q0 * k, w.out_rows, (size_t)nqc * k * 8, hipMemcpyDeviceToHost, st));  // speculative, as in search_impl
            LY_HIP(hipMemcpyAsync(out_dists + q0 * k, w.out_dists, (size_t)nqc * k * 4, hipMemcpyDeviceToHost, st));
            LY_HIP(hipMemcpyAsync(w.h_hdr, w.out_counts, 2 * QCHUNK * 4, hipMemcpyDeviceToHost, st));  // counts + overflow flags
            LY_HIP(hipStreamSynchronize(st));
            uint32_t nov = 0;
            for (uint32_t i = 0; i < nqc; ++i) nov += w.h_hdr[QCHUNK + i] ? 1 : 0;
            if (nov == 0) break;
            if (level == 2) return set_error(LYNSE_ERR_INTERNAL, "candidate overflow on the exhaustive plan");
        }
        memcpy(out_counts + q0, w.h_hdr, nqc * 4);
    }
    return LYNSE_OK;
}

// certified int8 coarse pass: FLAT-IP batches of 33..256 queries over an f32 shard (auto: shards of >= 64K rows;
// LYNSE_HIP_COARSE=i8 / f16 forces / disables it); strikes: overflows so far (3 turn it off), -1 = data not finite
static int coarse_env() {
    static const int v = []() { const char* e = env_str("LYNSE_HIP_COARSE"); return !e ? 0 : (!strcmp(e, "i8") ? 2 : (!strcmp(e, "f16") ? 1 : 0)); }();
    return v;
}
// per-metric state of the certified int8 pass: IP reads the SQ8 codes of the rows, squared L2 the codes of the augmented rows
static std::atomic<int>& i8c_strike_counter(lynse_hip_flat* h, int metric) {
    return metric == M_L2 ? h->i8c_strikes_l2 : (metric == M_COS ? h->i8c_strikes_cos : h->i8c_strikes);
}
// (which code set a batch reads and in which form: i8c_form / i8c_code_set, with run_chunk)
static bool i8c_codes_ready(const lynse_hip_flat* h, int metric, uint64_t nqc = 0, bool masked = false) {
    return i8c_code_set(h, i8c_form(h, metric, nqc, masked)).ready(h->n);
}
static bool i8c_codes_finite(const lynse_hip_flat* h, int metric, uint64_t nqc = 0, bool masked = false) {
    return i8c_code_set(h, i8c_form(h, metric, nqc, masked)).finite;
}
static int ensure_i8c_codes_locked(lynse_hip_flat* h, int metric, uint64_t nqc = 0, bool masked = false) {
    switch (i8c_form(h, metric, nqc, masked)) {
    case I8C_L2_AUG: return ensure_codes_locked(h, h->sq8a, CODES_AUG);
    case I8C_COS: return ensure_codes_locked(h, h->sq8c, CODES_UNIT);
    default: return ensure_sq8_locked(h);
    }
}
static void i8c_add_strike(lynse_hip_flat* h, int metric) {
    std::atomic<int>& c = i8c_strike_counter(h, metric);
    if (c.load() >= 0) c.fetch_add(1);
}
static bool i8c_eligible(const lynse_hip_flat* h, int metric, bool filtered, uint64_t nqc, bool view = false, bool masked = false, bool ivf = false) {
    // filtered: a subset filter on the gathered-rows strategy (never int8); masked: a subset filter as a row bitmask — the
    // masked int8 scan (whole 128-column slabs only)
    // view: a row-range view of search_large_k (h->n is the range): the SQ8 codes belong to the whole shard
    const int strikes = (metric == M_L2 ? h->i8c_strikes_l2 : (metric == M_COS ? h->i8c_strikes_cos : h->i8c_strikes)).load();
    static const int l2_off = []() { const char* e = env_str("LYNSE_HIP_COARSE_L2"); return e && !strcmp(e, "f16") ? 1 : 0; }();
    // squared L2 streams round_up(dim + 1, 128) bytes of augmented codes per row against 2 round_up(dim, 8) of the f16 shadow and
    // rescoring pools ~10x wider: it pays from ~256 dimensions on (MI355X: 10M x 768 x 256 3.97 -> 2.81 ms; 1M x 128, k = 100
    // 0.24 -> 0.34 ms: stays on the f16 pass)
    const bool l2_ok = metric == M_L2 && !l2_off &&
                       (i8c_form(h, metric, nqc, masked) == I8C_L2_PLAIN || (h->dim >= 256 && (uint64_t)h->ld8a * 4 <= (uint64_t)h->ld16 * 2 * 3));
    // cosine streams the codes of the unit rows (1 B per element, like IP); tiny-norm rows make the f16 pass go exhaustive and
    // are left to it
    const bool cos_ok = metric == M_COS && !l2_off && h->dim >= 256 && !h->cos_degenerate;
    if (masked && metric != M_L2 && h->ld8 % 128 != 0) return false;
    // batches of <= 32 queries (the 128 x 32 tiling, HBM-bound: half the bytes = half the time) from 256K rows on — below, the scan
    // is a few tens of microseconds either way and the exact few-query kernel often answers alone (LYNSE_HIP_COARSE_SMALLQ=0: off)
    static const int smallq = env_int("LYNSE_HIP_COARSE_SMALLQ", 1);
    const bool nq_ok = nqc > SCAN_BQ_SMALL || (smallq && nqc >= 1 && (coarse_env() == 2 || h->n >= 262144));   // (masked small batches too)
    // (F16 shards too: the codes are built from the exactly decoded halves, the exact rescoring uses the f16 kernels' sequential
    // sums — any summation order is inside the bound's rounding term)
    // FLAT-IP over rows of one or two whole 64-element slabs (64 / 128 columns, and the padded 48..63 / 96..127): batches of 33..256
    // queries run the float pass on the f16 shadow — k_scan_qh (scan_qh.h) is faster there than the 256 x 256 int8 tile over 128-byte code
    // rows and its margin ~2.5x tighter (round 5, 1M rows, 256 queries: 64 columns k = 10 / 100 0.222 / 0.318 -> 0.137 / 0.166 ms, 100 columns
    // 0.234 / 0.344 -> 0.169 / 0.188, 128 columns 0.163 / 0.273 -> 0.175 / 0.193; 100 queries 0.157 -> 0.127).  LYNSE_HIP_IP_LOWD=i8: the int8 pass
    // (read per call: tests; ivf: the list scans of an IVF store run the work-list tilings of k_scan_h16 either way — they keep the codes)
    const char* lowd_env = env_str("LYNSE_HIP_IP_LOWD");
    const bool lowd_i8 = lowd_env && !strcmp(lowd_env, "i8");
    // (gated on the very shape predicate qh_scan_ok applies — a batch k_scan_qh would not take must not lose the int8 pass to the slower
    // 256 x 256 f16 tile; `view` = the gathered rows of a subset filter, a widened handle never comes here with <= 256 queries)
    if (metric == M_IP && !lowd_i8 && !ivf && !masked && !filtered && !view && coarse_env() != 2 && h->qchunk <= QCHUNK && qh_shape(h->ld16, nqc))
        return false;
    return (metric == M_IP || l2_ok || cos_ok) && !filtered && !view && nq_ok &&
           coarse_env() != 1 && strikes >= 0 && strikes < 3 && (coarse_env() == 2 || h->n >= 65536);
}

// Shared driver: q_src is nq x dim f32 (float metrics / f32 binary queries) or nq x words u64
// (pre-packed).  Sources and destinations are host or device pointers according to `on_device`.
static int search_large_k(lynse_hip_flat* h, const void* q_src, bool packed_queries, uint64_t nq, uint32_t k, int metric,
                          uint64_t* out_rows, float* out_dists, uint32_t* out_counts, bool on_device, hipStream_t user_stream,
                          const uint64_t* subset = nullptr, uint64_t n_subset = 0, bool filtered = false,
                          const uint64_t* bitset_words = nullptr, uint64_t n_words = 0);

// Adds one finished search to the handle's profile: the pipeline time between its two events and the HIP-event duration of
// every scan launch (events of the search context `cx`).
static int prof_accumulate(lynse_hip_flat* h, lynse_hip_flat::Ctx& cx, hipEvent_t ev_begin, hipEvent_t ev_end,
                           const std::vector<std::pair<size_t, uint64_t>>& scan_events, bool binary, uint64_t fallback_queries) {
    LY_HIP(hipEventSynchronize(ev_end));
    float ms = 0.f;
    LY_HIP(hipEventElapsedTime(&ms, ev_begin, ev_end));
    std::lock_guard<std::mutex> plk(h->prof_mu);
    h->prof.total_us += (double)ms * 1000.0;
    const uint64_t row_bytes = binary ? (uint64_t)h->words * 8 : (uint64_t)h->dim * 4;
    for (auto& se : scan_events) {
        float sms = 0.f;
        LY_HIP(hipEventElapsedTime(&sms, cx.ev_pool[se.first], cx.ev_pool[se.first + 1]));
        h->prof.scan_us += (double)sms * 1000.0;
        h->prof.scan_launches += 1;
        h->prof.scan_rows += se.second;
        h->prof.scan_bytes += se.second * row_bytes;
    }
    h->prof.searches += 1;
    h->prof.fallback_queries += fallback_queries;
    return LYNSE_OK;
}

static int search_impl_once(lynse_hip_flat* h, const void* q_src, bool packed_queries, uint64_t nq, uint32_t k,
                            int metric, uint64_t* out_rows, float* out_dists, uint32_t* out_counts,
                            bool on_device, hipStream_t user_stream, const uint64_t* subset, uint64_t n_subset,
                            bool filtered, const uint64_t* bitset_words, uint64_t n_words, bool caller_holds_exclusive, bool force_shadow,
                            bool words_on_device);
static int search_impl(lynse_hip_flat* h, const void* q_src, bool packed_queries, uint64_t nq, uint32_t k,
                       int metric, uint64_t* out_rows, float* out_dists, uint32_t* out_counts,
                       bool on_device, hipStream_t user_stream, const uint64_t* subset = nullptr, uint64_t n_subset = 0,
                       bool filtered = false, const uint64_t* bitset_words = nullptr, uint64_t n_words = 0,
                       bool caller_holds_exclusive = false, bool words_on_device = false) {
    int rc = search_impl_once(h, q_src, packed_queries, nq, k, metric, out_rows, out_dists, out_counts, on_device, user_stream, subset, n_subset,
                              filtered, bitset_words, n_words, caller_holds_exclusive, false, words_on_device);
    // (a batch that started on the int8 pass under the shared lock and now needs the f16 shadow — an overflow, or a last chunk of a
    // different shape: once more from the top, under the writer lock, with the shadow built first)
    if (rc == LY_RESTART_EXCLUSIVE)
        rc = search_impl_once(h, q_src, packed_queries, nq, k, metric, out_rows, out_dists, out_counts, on_device, user_stream, subset, n_subset,
                              filtered, bitset_words, n_words, caller_holds_exclusive, true, words_on_device);
    return rc;
}
static int search_impl_once(lynse_hip_flat* h, const void* q_src, bool packed_queries, uint64_t nq, uint32_t k,
                            int metric, uint64_t* out_rows, float* out_dists, uint32_t* out_counts,
                            bool on_device, hipStream_t user_stream, const uint64_t* subset, uint64_t n_subset,
                            bool filtered, const uint64_t* bitset_words, uint64_t n_words, bool caller_holds_exclusive, bool force_shadow,
                            bool words_on_device) {
    // filtered: the subset is either a list of row ids (`subset`, n_subset) or BitSet words (`bitset_words`; n_subset =
    // number of set bits below len, counted by the caller).  words_on_device: the words are in this device's memory already
    // (lynse_hip_flat_search_filtered_bitset_device_f32): they reach the mask by a device copy
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    LY_TRY(metric_check(metric));
    if (nq == 0) return LYNSE_OK;
    if (!q_src || !out_counts || (k && (!out_rows || !out_dists))) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    LY_TRY(use_device(h));
    profile_begin_search(h);
    const bool binary = metric >= M_HAMMING;
    // Locking: an unfiltered search over a shard whose derived data (row statistics, f16 shadow, packed words, SQ8 codes of
    // the int8 coarse pass) is up to date runs under the SHARED lock on a search context of its own — subset-filtered searches on
    // the masked-scan strategy included; anything that has to build or borrows per-handle state (lazy builds, the gathered-rows
    // strategy of a subset filter) runs EXCLUSIVE on context 0.
    std::shared_lock<std::shared_mutex> rlk(h->rw, std::defer_lock);
    std::unique_lock<std::shared_mutex> xlk(h->rw, std::defer_lock);
    CtxLease lease;
    auto derived_ready = [&]() {
        if (binary) {
            if (!(h->packed_only || (h->packed != nullptr && h->n_packed == h->n))) return false;
            return !bin_mfma_eligible(h, metric, filtered, std::min<uint64_t>(nq, QCHUNK)) || (h->bpm && h->n_bpm == h->n);   // (the +-1 copy is a lazy build too)
        }
        if (h->packed_only) return true;  // (rejected below)
        if (h->n_stats != h->n) return false;
        if (force_shadow && !shadow_ready(h)) return false;
        // (filtered: what matters is the MASKED int8 scan — a gathered-rows search goes exclusive anyway)
        // a batch that takes the certified int8 pass needs its codes; every other float batch the f16 shadow (a lazy copy too).  The
        // chunks of a large batch can differ (the last one may be small): the chunk loop checks again and restarts under the writer lock
        if (i8c_eligible(h, metric, false, std::min<uint64_t>(nq, QCHUNK), caller_holds_exclusive, filtered)) {
            // (the blocking search alone scans the SQ7 copy: a wanted copy that is missing, or a stale one, is dealt with under the writer lock)
            if (sq7_stale(h) || (sq7_wanted(h, metric, std::min<uint64_t>(nq, QCHUNK), filtered) && h->sq8.finite && !sq7_ready(h))) return false;
            // (so does the predicted plan: column statistics that are wanted and missing are built under the writer lock)
            if (predict_wanted(h, metric, std::min<uint64_t>(nq, QCHUNK), (uint32_t)std::min<uint64_t>(k, h->n), filtered) &&
                i8c_codes_ready(h, metric, std::min<uint64_t>(nq, QCHUNK), filtered) && i8c_codes_finite(h, metric, std::min<uint64_t>(nq, QCHUNK), filtered) &&
                !predict_code_set(h, metric, std::min<uint64_t>(nq, QCHUNK)).stats_ready()) return false;
            return i8c_codes_ready(h, metric, std::min<uint64_t>(nq, QCHUNK), filtered);
        }
        return shadow_ready(h) || small_path_ok(h, std::min<uint64_t>(nq, QCHUNK), (uint32_t)std::min<uint64_t>(k, h->n), metric, filtered);
    };
    // k beyond the candidate capacity of one pass (k > cap / 4 over more than cap rows; the reference accepts any k, and its
    // server caps at MAX_TOP_K = 10,000, src/server/mod.rs:46): row ranges of `cap` rows, each answered exactly, merged.
    // (n and cap are read under the lock the search then runs under: an append between the decision and the search
    // cannot turn an ordinary search into an unsupported one.)
    auto needs_large_k = [&]() {
        if (h->n <= h->cap) return false;
        const uint64_t kk0 = std::min<uint64_t>(k, h->n);
        return (filtered ? std::min<uint64_t>(kk0, n_subset) : kk0) > h->cap / 4;
    };
    auto go_large_k = [&]() {
        if (filtered && words_on_device) {   // (the row-range views take their subset from host words: read them back)
            std::vector<uint64_t> host_words(std::max<uint64_t>(1, n_words), 0ull);
            if (n_words && hipMemcpy(host_words.data(), bitset_words, (size_t)n_words * 8, hipMemcpyDeviceToHost) != hipSuccess)
                return set_error(LYNSE_ERR_DEVICE, "hipMemcpy of the device BitSet words failed");
            return search_large_k(h, q_src, packed_queries, nq, k, metric, out_rows, out_dists, out_counts, on_device, user_stream,
                                  subset, n_subset, true, host_words.data(), n_words);
        }
        return filtered ? search_large_k(h, q_src, packed_queries, nq, k, metric, out_rows, out_dists, out_counts, on_device, user_stream,
                                         subset, n_subset, true, bitset_words, n_words)
                        : search_large_k(h, q_src, packed_queries, nq, k, metric, out_rows, out_dists, out_counts, on_device, user_stream);
    };
    // filtered search, strategy (flat_mmap.rs:549-556 switches at a fixed 50,000 ids): gather the listed shadow rows and scan
    // only those when that is cheaper than a masked scan of the whole shard — bytes over measured rates on MI355X
    bool strategy_direct = false, strategy_known = false;
    auto choose_direct = [&]() -> bool {
        if (!filtered || binary) return false;
        const double rate = nq <= SCAN_BQ_SMALL ? 6.0e12 : 3.4e12;
        const double chunks = (double)((nq + QCHUNK - 1) / QCHUNK);
        const double row_b = (double)h->dim * 2.0;
        const double c_direct = (double)n_subset * row_b * 2.0 / 2.5e12 + (double)n_subset * row_b / rate * chunks + 120e-6;
        // (the masked scan of 33..256 queries streams the SQ8 codes when the certified int8 pass is available: 1 B per element
        // at ~3.6 TB/s, measured 10M x 768 x 256 with a 50 % subset: 2.2 ms)
        const bool mask_i8 = i8c_eligible(h, metric, false, std::min<uint64_t>(nq, QCHUNK), caller_holds_exclusive, true);
        const double c_scan = (mask_i8 ? (double)h->n * (double)h->dim / (nq <= SCAN_BQ_SMALL ? 6.5e12 : 3.6e12) : (double)h->n * row_b / rate) * chunks + 80e-6;
        const int force = env_int("LYNSE_HIP_FILTER_STRATEGY", 0);  // tests: 1 = gathered rows, 2 = masked scan (read per call)
        return (double)n_subset * row_b <= 8e9 && (force == 1 || (force == 0 && c_direct < c_scan));
    };
    if (!caller_holds_exclusive) {
        rlk.lock();
        if (needs_large_k()) { rlk.unlock(); return go_large_k(); }
        // (a MASKED filtered search only needs scratch of its own context: shared lock; the gathered-rows strategy points the
        // handle's scan-side fields at the compact copy for the duration of the call: exclusive)
        // (the strategy is decided ONCE, here: its inputs — the strike counters concurrent searches bump, an environment variable —
        // can change between two evaluations, and "masked" under the shared lock followed by "gathered" at the use site would run
        // the gathered-rows path, which repoints handle-wide scan fields, beside concurrent readers)
        strategy_direct = filtered && n_subset != 0 && choose_direct();
        strategy_known = true;
        if (!user_stream && derived_ready() && !(filtered && (n_subset == 0 || strategy_direct))) {
            LY_TRY(lease.acquire(h));
        } else {
            rlk.unlock();
            LY_TRY(writer_lock(h, xlk));  // (builds, subset filters, a caller's stream: exclusive, and no tickets outstanding)
            if (needs_large_k()) { xlk.unlock(); return go_large_k(); }
        }
    }
    hipStream_t st = user_stream ? user_stream : cur(h).stream;
    const hipMemcpyKind in_kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const hipMemcpyKind out_kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;

    if (packed_queries && !binary) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "packed queries need a binary metric");
    if (!binary && h->packed_only) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "store holds packed rows; float metrics unavailable");

    if (filtered && n_subset && !subset && !bitset_words) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "subset is NULL");
    // empty store, k == 0 or an empty subset -> empty results, not an error (flat_mmap.rs:832-835, :498-500)
    if (h->n == 0 || k == 0 || (filtered && n_subset == 0)) {
        if (on_device) LY_HIP(hipMemsetAsync(out_counts, 0, nq * 4, st));
        else memset(out_counts, 0, nq * 4);
        if (on_device) LY_HIP(hipStreamSynchronize(st));
        return LYNSE_OK;
    }
    uint32_t kk = (uint32_t)std::min<uint64_t>(k, h->n);  // k.min(n), flat_mmap.rs:836
    if (filtered) kk = (uint32_t)std::min<uint64_t>(kk, n_subset);  // k.min(subset.len()), flat_mmap.rs:501
    if (h->n > h->cap && kk > h->cap / 4)
        return set_error(LYNSE_ERR_UNSUPPORTED, "k > cap/4 over more than cap rows is not supported together with a subset filter");
    // (rows wider than 4096 bits run on k_scan_binary_wide: no LDS tile, no register-resident words)

    if (binary) {
        LY_TRY(ensure_packed_locked(h));
        if (xlk.owns_lock() && bin_mfma_eligible(h, metric, filtered, std::min<uint64_t>(nq, QCHUNK))) LY_TRY(ensure_bpm_locked(h));
    } else {
        LY_TRY(finalize_locked(h));
        if (force_shadow && (xlk.owns_lock() || caller_holds_exclusive)) LY_TRY(ensure_shadow_locked(h));
    }
    LY_TRY(ensure_workspace(h, k));
    Workspace& w = cur(h).ws;
    hipStream_t st0 = user_stream ? user_stream : cur(h).stream;
    // the f16 shadow, for whoever is about to scan it: built here under the writer lock, or the whole search starts over under it
    auto need_shadow = [&]() -> int {
        if (binary || shadow_ready(h)) return LYNSE_OK;
        if (xlk.owns_lock() || caller_holds_exclusive) return ensure_shadow_locked(h);
        return LY_RESTART_EXCLUSIVE;
    };
    bool direct = false;
    std::vector<uint64_t> sorted_subset;
    auto& fc = cur(h);   // (this search's context: 0 under the exclusive lock, the leased one under the shared lock)
    if (filtered) {
        direct = strategy_known ? strategy_direct : choose_direct();   // (caller_holds_exclusive: evaluated here, under that lock)
        if (direct && !xlk.owns_lock() && !caller_holds_exclusive) return set_error(LYNSE_ERR_INTERNAL, "gathered-rows filter strategy without the exclusive lock");
        if (n_subset > fc.subset_cap && (direct || !bitset_words)) {
            if (fc.d_subset) (void)hipFree(fc.d_subset);
            fc.d_subset = nullptr;
            LY_HIP(hipMalloc(&fc.d_subset, n_subset * 8));
            fc.subset_cap = n_subset;
        }
        bool ids_on_device = false;
        if (bitset_words && direct) {  // BitSet::to_vec on the device: upload the words (they double as scratch in d_mask), expand
            const uint64_t nw = std::min<uint64_t>(n_words, (h->n + 63) / 64);
            const uint64_t words32 = (std::max<uint64_t>(h->n, h->capacity) + 511) / 32 + 8;
            const uint32_t nblocks = (uint32_t)((nw + 255) / 256);
            if (words32 + nblocks + 16 > fc.mask_words) {
                if (fc.d_mask) (void)hipFree(fc.d_mask);
                fc.d_mask = nullptr;
                LY_HIP(hipMalloc(&fc.d_mask, (words32 + nblocks + 16) * 4));
                fc.mask_words = words32 + nblocks + 16;
            }
            if (n_subset > fc.subset_cap) {
                if (fc.d_subset) (void)hipFree(fc.d_subset);
                fc.d_subset = nullptr;
                LY_HIP(hipMalloc(&fc.d_subset, n_subset * 8));
                fc.subset_cap = n_subset;
            }
            uint32_t* d_counts = fc.d_mask + words32;
            LY_HIP(hipMemcpyAsync(fc.d_mask, bitset_words, nw * 8, words_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st0));
            const uint64_t* d_words = reinterpret_cast<const uint64_t*>(fc.d_mask);
            hipLaunchKernelGGL(k_bits_count, dim3(nblocks), dim3(256), 0, st0, d_words, nw, h->n, d_counts);
            hipLaunchKernelGGL(k_bits_offsets, dim3(1), dim3(1024), 0, st0, d_counts, nblocks);
            hipLaunchKernelGGL(k_bits_expand, dim3(nblocks), dim3(256), 0, st0, d_words, nw, h->n, d_counts, fc.d_subset);
            LY_HIP(hipGetLastError());
            ids_on_device = true;
        }
        const uint64_t* src = subset;
        if (direct && n_subset && !ids_on_device) {  // the direct path needs a set: sort + unique unless already strictly ascending (a BitSet's to_vec is)
            bool ascending = subset[n_subset - 1] < h->n;  // and every id valid
            for (uint64_t i = 1; i < n_subset && ascending; ++i) ascending = subset[i - 1] < subset[i];
            if (!ascending) {
                sorted_subset.assign(subset, subset + n_subset);
                std::sort(sorted_subset.begin(), sorted_subset.end());
                sorted_subset.erase(std::unique(sorted_subset.begin(), sorted_subset.end()), sorted_subset.end());
                while (!sorted_subset.empty() && sorted_subset.back() >= h->n) sorted_subset.pop_back();  // rows >= n are skipped (:5243)
                src = sorted_subset.data();
                n_subset = sorted_subset.size();
            }
        }
        if (src && n_subset && !ids_on_device) LY_HIP(hipMemcpyAsync(fc.d_subset, src, n_subset * 8, hipMemcpyHostToDevice, st0));
        if (!direct) {  // subset ids -> row bitmask on the device (the reference's bitset, flat_mmap.rs:672-679)
            const uint64_t words = (std::max<uint64_t>(h->n, h->capacity) + 511) / 32 + 8;
            if (words > fc.mask_words) {
                if (fc.d_mask) (void)hipFree(fc.d_mask);
                fc.d_mask = nullptr;
                LY_HIP(hipMalloc(&fc.d_mask, words * 4));
                fc.mask_words = words;
            }
            LY_HIP(hipMemsetAsync(fc.d_mask, 0, fc.mask_words * 4, st0));
            if (bitset_words) {  // the caller's BitSet words ARE the mask (u64 LE = two u32 words); bits >= len never match a row
                const uint64_t bytes = std::min<uint64_t>(n_words * 8, (h->n + 63) / 64 * 8);
                LY_HIP(hipMemcpyAsync(fc.d_mask, bitset_words, bytes, words_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st0));
            } else {
                const uint32_t blocks = (uint32_t)std::min<uint64_t>((n_subset + 255) / 256, (uint64_t)h->num_cu * 8);
                hipLaunchKernelGGL(k_mask_build, dim3(std::max<uint32_t>(blocks, 1)), dim3(256), 0, st0, fc.d_subset, n_subset, h->n, fc.d_mask);
                LY_HIP(hipGetLastError());
            }
        }
        if (direct && n_subset) {  // compact copy of the listed shadow rows + norms + 32-bit ids
            if (n_subset > h->g_cap) {
                for (void* p : {(void*)h->g_rows16, (void*)h->g_vn2, (void*)h->g_vrinv, (void*)h->g_ids32})
                    if (p) (void)hipFree(p);
                h->g_rows16 = nullptr; h->g_vn2 = h->g_vrinv = nullptr; h->g_ids32 = nullptr; h->g_cap = 0;
                LY_HIP(hipMalloc(&h->g_rows16, (size_t)n_subset * h->ld16 * 2 + 256));
                LY_HIP(hipMalloc(&h->g_vn2, ((size_t)n_subset + 256) * 4));
                LY_HIP(hipMalloc(&h->g_vrinv, ((size_t)n_subset + 256) * 4));
                LY_HIP(hipMalloc(&h->g_ids32, ((size_t)n_subset + 256) * 4));
                LY_HIP(hipMemsetAsync(h->g_vn2, 0, ((size_t)n_subset + 256) * 4, st0));
                LY_HIP(hipMemsetAsync(h->g_vrinv, 0, ((size_t)n_subset + 256) * 4, st0));
                h->g_cap = n_subset;
            }
            const uint64_t pieces = n_subset * (h->ld16 / 8);
            LY_TRY(need_shadow());   // (the gathered-rows strategy runs under the writer lock)
            hipLaunchKernelGGL(k_gather_rows16, dim3((uint32_t)std::min<uint64_t>((pieces + 255) / 256, (uint64_t)h->num_cu * 32)), dim3(256), 0,
                               st0, h->rows16, h->ld16, fc.d_subset, n_subset, h->g_rows16);
            LY_HIP(hipGetLastError());
            hipLaunchKernelGGL(k_gather_norms, dim3((uint32_t)std::min<uint64_t>((n_subset + 255) / 256, (uint64_t)h->num_cu * 8)), dim3(256), 0,
                               st0, h->vn2, h->vrinv, fc.d_subset, n_subset, h->g_vn2, h->g_vrinv, h->g_ids32);
            LY_HIP(hipGetLastError());
        }
        LY_HIP(hipStreamSynchronize(st0));  // `subset` / sorted_subset are caller / stack memory
        if (direct && n_subset == 0) {  // every listed row was out of range
            if (on_device) LY_HIP(hipMemsetAsync(out_counts, 0, nq * 4, st0));
            else memset(out_counts, 0, nq * 4);
            if (on_device) LY_HIP(hipStreamSynchronize(st0));
            return LYNSE_OK;
        }
    }
    const uint32_t* mask = (filtered && !direct) ? fc.d_mask : nullptr;
    // the gathered path scans the compact store through the ordinary pipeline: point the scan-side fields of the handle
    // at it for the duration of this call (the mutex is held); rescoring keeps using the f32 source rows by original id
    struct ViewGuard {
        lynse_hip_flat* h; bool on; _Float16* r16; uint64_t n; float *vn2, *vrinv;
        ~ViewGuard() { if (on) { h->rows16 = r16; h->n = n; h->vn2 = vn2; h->vrinv = vrinv; } }
    } view{h, direct, h->rows16, h->n, h->vn2, h->vrinv};
    if (direct) { h->rows16 = h->g_rows16; h->n = n_subset; h->vn2 = h->g_vn2; h->vrinv = h->g_vrinv; }

    hipEvent_t ev_begin = nullptr, ev_end = nullptr;
    ScanProf sprof;
    if (tl_prof) {
        LY_TRY(get_event(h, sprof.ev_used++, &ev_begin));
        LY_TRY(get_event(h, sprof.ev_used++, &ev_end));
        LY_HIP(hipEventRecord(ev_begin, st));
    }
    uint64_t fallback_queries = 0, predicted_queries = 0, predict_miss_queries = 0;
    bool i8c_attempted = false;

    // queries per pipeline pass: QCHUNK; a widened handle (the k-means assignment's centroid store: unfiltered float search of
    // a shard of <= cap rows) takes h->qchunk queries per pass, one k_scan_h16 launch scoring qchunk / 256 chunks (blockIdx.y)
    const bool wide = h->qchunk > QCHUNK && !binary && !filtered && h->n <= h->cap;
    const uint32_t QC = wide ? w.qcap : QCHUNK;
    for (uint64_t q0 = 0; q0 < nq; q0 += QC) {
        const uint32_t nqc = (uint32_t)std::min<uint64_t>(QC, nq - q0);
        // stage the chunk's queries in the workspace
        if (binary) {
            if (packed_queries) {
                LY_HIP(hipMemcpyAsync(w.QW, (const uint64_t*)q_src + q0 * h->words, (size_t)nqc * h->words * 8, in_kind, st));
            } else {  // pack_binary_query (flat_mmap.rs:1292-1296)
                LY_HIP(hipMemcpyAsync(w.Qf, (const float*)q_src + q0 * h->dim, (size_t)nqc * h->dim * 4, in_kind, st));
                hipLaunchKernelGGL(k_pack_bits<float>, dim3((nqc + 3) / 4), dim3(256), 0, st, w.Qf, h->dim, h->dim, nqc, w.QW, h->words);
                LY_HIP(hipGetLastError());
            }
        } else if (!on_device) {  // (device queries are read in place: they stay valid for the whole call)
            LY_HIP(hipMemcpyAsync(w.Qf, (const float*)q_src + q0 * h->dim, (size_t)nqc * h->dim * 4, in_kind, st));
        }
        const float* qsrc = (on_device && !binary) ? (const float*)q_src + q0 * h->dim : nullptr;
        // certified int8 coarse pass: FLAT-IP batches of 33..256 queries over an f32 shard with finite values (auto: shards
        // of >= 64K rows; LYNSE_HIP_COARSE=i8 / f16 forces / disables it).  An overflow first retries the f16 coarse pass;
        // three such strikes turn the int8 pass off for this handle (margins too wide for this data).
        bool i8c = i8c_eligible(h, metric, filtered && direct, nqc, caller_holds_exclusive, filtered && !direct);
        if (i8c) {
            const bool msk = filtered && !direct;
            if (xlk.owns_lock()) { LY_TRY(ensure_i8c_codes_locked(h, metric, nqc, msk)); sq7_sync_locked(h, metric, nqc, msk); LY_TRY(predict_sync_locked(h, metric, nqc, kk, msk)); }   // lazy builds: exclusive path only (a chunk without the SQ7 copy scans the SQ8 codes, one without column statistics runs the sampled plan)
            else if (!i8c_codes_ready(h, metric, nqc, msk)) i8c = false;                    // (shared path: derived_ready() saw them built)
            if (i8c && !i8c_codes_finite(h, metric, nqc, msk)) { i8c_strike_counter(h, metric).store(-1); i8c = false; }
        }
        i8c_attempted = i8c_attempted || i8c;
        // this chunk scans the f16 shadow.  (Not on the gathered-rows strategy: the compact copy was gathered from the complete shadow
        // above and the handle now VIEWS it — n is the subset size, so shadow_ready() would report a stale shadow and
        // ensure_shadow_locked() would point an F16 shard's aliased rows16 back at the whole shard: the scan then scored rows
        // 0 .. n_subset - 1 of the shard under the subset's row ids)
        if (!binary && !i8c && !direct && !small_path_ok(h, nqc, kk, metric, filtered)) LY_TRY(need_shadow());
        if (small_path_ok(h, nqc, kk, metric, filtered)) {
            // fused single-launch search: the last workgroup writes straight into the caller's device buffers, or into
            // pinned host memory (no copy kernels, one synchronisation); it cannot overflow
            const size_t rows_b = (size_t)nqc * k * 8, dists_b = (size_t)nqc * k * 4;
            uint64_t* r_dst = on_device ? out_rows + q0 * k : reinterpret_cast<uint64_t*>(w.h_out);
            float* d_dst = on_device ? out_dists + q0 * k : reinterpret_cast<float*>(w.h_out + rows_b);
            uint32_t* c_dst = on_device ? out_counts + q0 : w.h_hdr;
            LY_TRY(run_small(h, nqc, kk, k, metric, st, &sprof, r_dst, d_dst, c_dst, w.h_hdr + w.qcap,
                             on_device ? (const float*)q_src + q0 * h->dim : w.Qf));  // device queries are read in place
            LY_HIP(hipStreamSynchronize(st));
            if (!on_device) {
                memcpy(out_rows + q0 * k, w.h_out, rows_b);
                memcpy(out_dists + q0 * k, w.h_out + rows_b, dists_b);
                memcpy(out_counts + q0, w.h_hdr, nqc * 4);
            }
            continue;
        }
        bool allow_sts = true, allow_sq7 = true, allow_predict = true;
        for (int level = 0; level < 3; ++level) {  // sampled plan -> contiguous plan -> exhaustive plan (make_plan)
            ChunkResult res;
            // k_final writes the results where they belong — the caller's device arrays, or the pinned (device-visible)
            // staging buffer for small host-API results: no copy kernels behind the search; only large host results go
            // through the workspace + two device-to-host copies.  One synchronisation per chunk (counts + overflow flags in
            // one small pinned readback); a retry on the next plan level overwrites the outputs in stream order.
            const size_t rows_b = (size_t)nqc * k * 8, dists_b = (size_t)nqc * k * 4;
            const bool staged = !on_device && rows_b + dists_b <= H_OUT_BYTES;
            ChunkReq rq;
            rq.nq = nqc; rq.k = kk; rq.out_k = k; rq.metric = metric; rq.level = level;
            rq.mask = mask; rq.row_ids = direct ? h->g_ids32 : nullptr; rq.qsrc = qsrc;
            rq.i8c = i8c; rq.allow_sts = allow_sts; rq.allow_sq7 = allow_sq7; rq.allow_predict = allow_predict;
            rq.out.rows = on_device ? out_rows + q0 * k : (staged ? reinterpret_cast<uint64_t*>(w.h_out) : nullptr);
            rq.out.dists = on_device ? out_dists + q0 * k : (staged ? reinterpret_cast<float*>(w.h_out + rows_b) : nullptr);
            rq.out.counts2 = on_device ? out_counts + q0 : nullptr;
            rq.out.hdr_direct = true;
            LY_TRY(run_chunk(h, rq, st, &sprof, &res));
            if (!on_device && !staged) {
                LY_HIP(hipMemcpyAsync(out_rows + q0 * k, w.out_rows, rows_b, out_kind, st));
                LY_HIP(hipMemcpyAsync(out_dists + q0 * k, w.out_dists, dists_b, out_kind, st));
            }
            LY_TRY(stream_wait(st));  // (counts + overflow flags: written into the pinned header by k_final)
            uint32_t nov = 0, nmiss = 0, nover = 0;
            for (uint32_t i = 0; i < nqc; ++i) {
                const uint32_t f = w.h_hdr[w.qcap + i];
                nov += f ? 1 : 0; nover += (f & 1u) ? 1 : 0; nmiss += (f & PRED_MISS) ? 1 : 0;
            }
            if (res.used_predict) { predicted_queries += nqc; predict_miss_queries += nmiss; }
            if (nov == 0) {
                if (staged) { memcpy(out_rows + q0 * k, w.h_out, rows_b); memcpy(out_dists + q0 * k, w.h_out + rows_b, dists_b); }
                break;
            }
            if (level == 2) return set_error(LYNSE_ERR_INTERNAL, "candidate overflow on the exhaustive plan");
            fallback_queries += nov;
            if (res.used_predict) {  // the predicted threshold was too high for some query (a miss), too low (an overflow), or the model had nothing to say: the sampled plan of the same coarse pass.  A strike against prediction alone — none against int8 or SQ7
                allow_predict = false;
                if (nmiss || nover) h->predict_strikes.fetch_add(1);
                --level;
                continue;
            }
            if (res.used_sts) {  // the self-tightening scan overflowed (scores rising along every workgroup's chunk): the staged plan of the same coarse pass
                allow_sts = false;
                --level;
                continue;
            }
            if (res.used_sq7) {  // the wider SQ7 margin overflowed: the same plan level on the SQ8 codes — a strike against SQ7, none against int8
                allow_sq7 = false;
                h->sq7_strikes.fetch_add(1);
                --level;
                continue;
            }
            if (i8c) {  // same plan level again with the f16 coarse pass
                i8c = false;
                i8c_add_strike(h, metric);
                LY_TRY(need_shadow());
                --level;
                continue;
            }
            if (level == 0 && !res.sampled) level = 1;  // level 1 would repeat the same contiguous plan
        }
        if (!on_device) memcpy(out_counts + q0, w.h_hdr, nqc * 4);
    }

    if (tl_prof) {
        LY_HIP(hipEventRecord(ev_end, st));
        LY_TRY(prof_accumulate(h, cur(h), ev_begin, ev_end, sprof.scan_events, binary, fallback_queries));
        if (i8c_attempted) {  // bit 6: the search STARTED on the certified int8 pass (an overflow may have sent it to the f16 pass)
            std::lock_guard<std::mutex> plk(h->prof_mu);
            h->prof.last_plan |= 64u;
        }
        if (predicted_queries) {
            std::lock_guard<std::mutex> plk(h->prof_mu);
            h->prof.predicted_queries += predicted_queries;
            h->prof.predict_miss_queries += predict_miss_queries;
        }
    }
    return LYNSE_OK;
}

// Diagnostics of the CERTIFICATE (tests/test_gpu_certificate.py): the coarse score of every row of a small shard (n <= cap) for up
// to 256 queries, exactly as the scan kernels compute it (one emit-all stage of the real pipeline: MFMA dot products, the kernels'
// float expressions), in the metric's own space (IP: score, L2 / cosine: distance), and the per-query bound E the prep kernel
// certified (the margin the pipeline keeps is 2E).  coarse = 0: the f16 shadow, 1: the certified int8 pass in the form a batch of
// this shape would take; *out_form: bit 0 int8, bit 1 augmented-L2 codes, bit 2 plain-code L2, bit 3 unit-row cosine codes.
static int coarse_scores_impl(lynse_hip_flat* h, const float* queries, uint64_t nq, int metric, int coarse,
                              float* out_scores, float* out_bound, int* out_form, bool want_sq7) {
    if (!h || !queries || !out_scores || !out_bound) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    if (metric_additive(metric)) return metric_check(metric);
    if (metric < M_IP || metric > M_COS) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "float metrics only");
    if (nq == 0 || nq > QCHUNK) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "1..256 queries");
    LY_TRY(use_device(h));
    std::unique_lock<std::shared_mutex> xlk;
    LY_TRY(writer_lock(h, xlk));
    if (h->packed_only || h->n == 0 || h->n > h->cap) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "a float shard of 1..cap rows");
    LY_TRY(finalize_locked(h));
    LY_TRY(ensure_workspace(h, 1));
    const bool i8c = coarse != 0;
    if (!i8c) LY_TRY(ensure_shadow_locked(h));
    if (i8c) {
        LY_TRY(ensure_i8c_codes_locked(h, metric, nq));
        if (!i8c_codes_finite(h, metric, nq)) return set_error(LYNSE_ERR_UNSUPPORTED, "the shard holds non-finite values: no int8 pass");
        if (want_sq7) sq7_sync_locked(h, metric, nq, false);
        if (want_sq7 && !(sq7_wanted(h, metric, nq, false) && sq7_ready(h)))
            return set_error(LYNSE_ERR_UNSUPPORTED, "no SQ7 scan for this shape (FLAT-IP, 129..256 queries, LYNSE_HIP_SQ7 not 0)");
    }
    Workspace& w = cur(h).ws;
    hipStream_t st = cur(h).stream;
    LY_HIP(hipMemcpyAsync(w.Qf, queries, (size_t)nq * h->dim * 4, hipMemcpyHostToDevice, st));
    ScanProf sprof;
    ChunkReq rq;
    rq.nq = (uint32_t)nq; rq.k = rq.out_k = 1; rq.metric = metric; rq.level = 1; rq.i8c = i8c; rq.allow_sq7 = want_sq7; rq.mode = CHUNK_COARSE_DUMP;
    ChunkResult res;
    LY_TRY(run_chunk(h, rq, st, &sprof, &res));
    if (want_sq7 && !res.used_sq7) return set_error(LYNSE_ERR_INTERNAL, "the diagnostics chunk did not scan the SQ7 copy");
    LY_HIP(hipStreamSynchronize(st));
    const I8cForm form = i8c_form(h, metric, nq, false);
    const bool l2n = i8c && form == I8C_L2_PLAIN, aug = i8c && form == I8C_L2_AUG, cosq = i8c && form == I8C_COS;
    if (out_form) *out_form = (i8c ? 1 : 0) | (aug ? 2 : 0) | (l2n ? 4 : 0) | (cosq ? 8 : 0) | (res.used_sq7 ? 16 : 0);
    const bool key_asc = metric_ascending((aug || cosq) ? (int)M_IP : metric);
    std::vector<uint64_t> keys(h->n);
    std::vector<float> m2(nq);
    LY_HIP(hipMemcpy(m2.data(), w.marg2, nq * 4, hipMemcpyDeviceToHost));
    for (uint64_t q = 0; q < nq; ++q) {
        LY_HIP(hipMemcpy(keys.data(), w.cand + (size_t)q * w.cap, (size_t)h->n * 8, hipMemcpyDeviceToHost));
        for (uint64_t r = 0; r < h->n; ++r) {
            if (key_row(keys[r]) != (uint32_t)r) return set_error(LYNSE_ERR_INTERNAL, "the emit-all stage did not leave row r in slot r");
            const float sc = key_score(keys[r], key_asc);
            out_scores[q * h->n + r] = (aug || cosq) ? -sc : sc;   // (those forms scan the NEGATED distance as an inner product)
        }
        out_bound[q] = 0.5f * m2[q];
    }
    return LYNSE_OK;
}

extern "C" int lynse_hip_flat_coarse_scores(lynse_hip_flat* h, const float* queries, uint64_t nq, int metric, int coarse,
                                            float* out_scores, float* out_bound, int* out_form) {
    return coarse_scores_impl(h, queries, nq, metric, coarse, out_scores, out_bound, out_form, false);
}
// The same diagnostics for the SQ7 form of the FLAT-IP int8 pass (129..256 queries, LYNSE_HIP_SQ7 not 0; forced with 1 on any shard):
// coarse scores of the non-negative 7-bit copy and the bound E its prep certified; *out_form gains bit 4.
extern "C" int lynse_hip_flat_coarse_scores_sq7(lynse_hip_flat* h, const float* queries, uint64_t nq, float* out_scores, float* out_bound, int* out_form) {
    return coarse_scores_impl(h, queries, nq, M_IP, 1, out_scores, out_bound, out_form, true);
}
// SQ7 state of a shard (tests, diagnostics): rows the copy covers (0: not built) and its overflow strikes (3 switch it off).
extern "C" int lynse_hip_flat_sq7_state(lynse_hip_flat* h, uint64_t* out_rows, int* out_strikes) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    std::shared_lock<std::shared_mutex> lk(h->rw);
    if (out_rows) *out_rows = h->sq7.codes ? h->sq7.n : 0;
    if (out_strikes) *out_strikes = h->sq7_strikes.load();
    return LYNSE_OK;
}

// The model of the predicted threshold on the host (predict.h; no device involved): tests restate it in numpy.
extern "C" int lynse_hip_predict_z(uint64_t n, double keys_per_query, double* out_z) {
    if (!out_z) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    *out_z = predict_z(n, keys_per_query);
    return LYNSE_OK;
}
extern "C" int lynse_hip_predict_col_stats(const int64_t* sums, uint32_t cols, uint64_t n, double* out_mu, double* out_var) {
    if (!sums || !out_mu || !out_var) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    static_assert(sizeof(long long) == sizeof(int64_t), "64-bit sums");
    predict_col_stats(reinterpret_cast<const long long*>(sums), cols, n, out_mu, out_var);
    return LYNSE_OK;
}
extern "C" int lynse_hip_predict_threshold(const int8_t* u, const double* mu, const double* var, uint32_t cols, double z, float bq, float sq,
                                           double* out_m, double* out_v, float* out_thr) {
    if (!u || !mu || !var || !out_thr) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    *out_thr = predict_threshold(u, mu, var, cols, z, bq, sq, out_m, out_v);
    return LYNSE_OK;
}

// Diagnostics of the predicted threshold (tests/test_gpu_predict.py): what k_i8c_prep_queries computes for a batch of the predicted shape
// — the int8 image u, B_q, s_q, m_q, v_q and the threshold, with z as the search forms it for k — and the column statistics it read.
// Builds codes and statistics like a search of the shape would; LYNSE_ERR_UNSUPPORTED where that search would not predict.
extern "C" int lynse_hip_flat_predict_debug(lynse_hip_flat* h, const float* queries, uint64_t nq, uint32_t k, int metric, int8_t* out_u, double* out_mu,
                                            double* out_var, float* out_bq, float* out_sq, double* out_m, double* out_v, float* out_thr, double* out_z,
                                            uint32_t* out_cols) {
    if (!h || !queries) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    if (nq == 0 || nq > QCHUNK) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "1..256 queries");
    LY_TRY(use_device(h));
    LY_WRITER(h, xlk);
    if (h->packed_only || h->n == 0) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "no float rows");
    LY_TRY(finalize_locked(h));
    LY_TRY(ensure_workspace(h, 1));
    const uint32_t kk = (uint32_t)std::min<uint64_t>(k, h->n);
    if (!predict_wanted(h, metric, nq, kk, false) || !i8c_eligible(h, metric, false, nq))
        return set_error(LYNSE_ERR_UNSUPPORTED, "no predicted plan for this shape (FLAT-IP / cosine, 129..256 queries, k <= 32, LYNSE_HIP_PREDICT not 0)");
    LY_TRY(ensure_i8c_codes_locked(h, metric, nq));
    if (!i8c_codes_finite(h, metric, nq)) return set_error(LYNSE_ERR_UNSUPPORTED, "the shard holds non-finite values: no int8 pass");
    sq7_sync_locked(h, metric, nq, false);
    LY_TRY(predict_sync_locked(h, metric, nq, kk, false));
    const bool sq7 = sq7_wanted(h, metric, nq, false) && sq7_ready(h);
    const CodeSet& s = predict_code_set(h, metric, nq);
    if (!s.stats_ready()) return set_error(LYNSE_ERR_UNSUPPORTED, "no column statistics for this code set");
    const I8cForm form = i8c_form(h, metric, nq, false);
    const I8cOperand opd = i8c_operand(h, form, sq7);
    Workspace& w = cur(h).ws;
    hipStream_t st = cur(h).stream;
    const uint32_t qpad = 256, nslab = (opd.cols + 127) / 128;
    LY_HIP(hipMemcpyAsync(w.Qf, queries, (size_t)nq * h->dim * 4, hipMemcpyHostToDevice, st));
    I8cPrepArgs p{};
    p.Q = w.Qf; p.D = h->dim; p.qpad = qpad; p.nslab = nslab; p.nq = (uint32_t)nq; p.vmax = h->vmax; p.img = reinterpret_cast<int8_t*>(w.Q16);
    fill_i8c_prep(p, opd, form);
    p.sq = w.qinv; p.bq = w.qn2; p.marg2 = w.marg2; p.thr = w.thr; p.count = w.count; p.overflow = w.overflow; p.gsync = w.gsync;
    p.pred_mu = s.mu; p.pred_var = s.var; p.pred_chk = w.pred_chk; p.pred_dbg = w.pred_dbg;
    const double z = predict_z(h->n, predict_keys_per_query(kk));
    p.pred_z = z;
    hipLaunchKernelGGL(k_i8c_prep_queries, dim3(qpad), dim3(256), 0, st, p);
    LY_HIP(hipGetLastError());
    std::vector<int8_t> img((size_t)nslab * qpad * 128);
    std::vector<double> dbg((size_t)nq * 2);
    LY_HIP(hipMemcpyAsync(img.data(), w.Q16, img.size(), hipMemcpyDeviceToHost, st));
    LY_HIP(hipMemcpyAsync(dbg.data(), w.pred_dbg, dbg.size() * 8, hipMemcpyDeviceToHost, st));
    if (out_bq) LY_HIP(hipMemcpyAsync(out_bq, w.qn2, nq * 4, hipMemcpyDeviceToHost, st));
    if (out_sq) LY_HIP(hipMemcpyAsync(out_sq, w.qinv, nq * 4, hipMemcpyDeviceToHost, st));
    if (out_thr) LY_HIP(hipMemcpyAsync(out_thr, w.thr, nq * 4, hipMemcpyDeviceToHost, st));
    LY_HIP(hipStreamSynchronize(st));
    for (uint64_t q = 0; q < nq; ++q) {
        if (out_m) out_m[q] = dbg[2 * q];
        if (out_v) out_v[q] = dbg[2 * q + 1];
        if (out_u)
            for (uint32_t i = 0; i < s.cols; ++i) {   // (the image layout of k_i8c_prep_queries)
                const uint32_t sl = i / 128, kc = i % 128, l = kc >> 4, e = kc & 15, pp = l ^ (((uint32_t)q >> 1) & 7);
                out_u[q * s.cols + i] = img[(((size_t)sl * qpad + q) * 8 + pp) * 16 + e];
            }
    }
    if (out_mu) memcpy(out_mu, s.h_mu.data(), (size_t)s.cols * 8);
    if (out_var) memcpy(out_var, s.h_var.data(), (size_t)s.cols * 8);
    if (out_z) *out_z = z;
    if (out_cols) *out_cols = s.cols;
    return LYNSE_OK;
}
// State of the predicted plan of a shard (tests, diagnostics): strikes so far (3 switch it off until the codes are fitted again) and the
// rows the column statistics of the plain / unit-row / SQ7 code sets cover (0: not collected).
extern "C" int lynse_hip_flat_predict_state(lynse_hip_flat* h, int* out_strikes, uint64_t* out_rows_sq8, uint64_t* out_rows_cos, uint64_t* out_rows_sq7) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    std::shared_lock<std::shared_mutex> lk(h->rw);
    if (out_strikes) *out_strikes = h->predict_strikes.load();
    if (out_rows_sq8) *out_rows_sq8 = h->sq8.mu ? h->sq8.colsum_n : 0;
    if (out_rows_cos) *out_rows_cos = h->sq8c.mu ? h->sq8c.colsum_n : 0;
    if (out_rows_sq7) *out_rows_sq7 = h->sq7.mu ? h->sq7.colsum_n : 0;
    return LYNSE_OK;
}

// State of the coarse-pass selection of a shard (tests, diagnostics): strikes = overflows of the certified int8 pass so
// far (3 switch it off for the handle, -1 = switched off because the data is not finite), sq8_rows = rows covered by the
// SQ8 codes currently built.
extern "C" int lynse_hip_flat_coarse_state(lynse_hip_flat* h, int* out_strikes, uint64_t* out_sq8_rows) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    std::shared_lock<std::shared_mutex> lk(h->rw);
    if (out_strikes) *out_strikes = h->i8c_strikes.load();
    if (out_sq8_rows) *out_sq8_rows = h->sq8.codes ? h->sq8.n : 0;
    return LYNSE_OK;
}

extern "C" uint64_t lynse_hip_flat_bpm_rows(const lynse_hip_flat* h) {
    if (!h) return 0;
    std::shared_lock<std::shared_mutex> lk(const_cast<lynse_hip_flat*>(h)->rw);   // (writers reallocate these fields)
    return h->bpm ? h->n_bpm : 0;
}

// Builds — now, not inside the first search that needs it — every derived copy a batch of `nq` queries of `metric` will read:
// row statistics + f16 shadow (float metrics), the SQ8 codes of the certified int8 pass (IP batches of 33..256 queries over
// >= 64K rows), the packed words (binary metrics from f32 rows) and the +-1 byte copy of batched Hamming (>= 96 queries).
// The reference builds its own derived data lazily too (ensure_binary / ensure_sq8, flat_mmap.rs:375-401); a server calls
// this after a bulk load so that the first query does not pay for it under the writer lock.
extern "C" int lynse_hip_flat_prepare(lynse_hip_flat* h, int metric, uint64_t nq) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    LY_TRY(metric_check(metric));
    LY_WRITER(h, lk);
    LY_TRY(use_device(h));
    if (h->n == 0) return LYNSE_OK;
    const uint64_t nqc = std::min<uint64_t>(std::max<uint64_t>(nq, 1), QCHUNK);
    if (metric >= M_HAMMING) {
        LY_TRY(ensure_packed_locked(h));
        if (bin_mfma_eligible(h, metric, false, nqc)) LY_TRY(ensure_bpm_locked(h));
        return LYNSE_OK;
    }
    if (h->packed_only) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "store holds packed rows; float metrics unavailable");
    LY_TRY(finalize_locked(h));
    if (i8c_eligible(h, metric, false, nqc)) {
        LY_TRY(ensure_i8c_codes_locked(h, metric, nqc));
        if (!i8c_codes_finite(h, metric, nqc)) i8c_strike_counter(h, metric).store(-1);
        else sq7_sync_locked(h, metric, nqc, false);
    }
    // a batch that does not take the int8 pass scans the f16 shadow (unless the exact few-query kernel answers it)
    if (!i8c_eligible(h, metric, false, nqc) && !small_path_ok(h, nqc, 10, metric, false)) LY_TRY(ensure_shadow_locked(h));
    return LYNSE_OK;
}

// Bytes of HBM the shard holds: source rows + every derived copy built so far (search workspaces not included).
extern "C" uint64_t lynse_hip_flat_hbm_bytes(const lynse_hip_flat* h) {
    if (!h) return 0;
    std::shared_lock<std::shared_mutex> lk(const_cast<lynse_hip_flat*>(h)->rw);   // (writers reallocate these fields)
    uint64_t b = 0;
    if (h->rows) b += h->capacity * h->ld * 4ull;
    if (h->rows_h) b += h->capacity * h->ld16 * 2ull;
    if (h->rows16 && !h->shadow_alias) b += h->cap16 * h->ld16 * 2ull;
    if (h->vn2) b += 2ull * (h->stats_capacity + 256) * 4;
    if (h->packed) b += h->packed_capacity * h->words * 8ull;
    for (const CodeSet* s : {&h->sq8, &h->sq7, &h->sq8a, &h->sq8c}) b += s->hbm_bytes();
    if (h->bpm) b += h->bpm_cap * h->ld_bpm;
    return b;
}

// Large k: the shard is cut into row ranges of `cap` rows (any k <= range size is exact there: emit-all + select), every
// range is searched through a temporary VIEW of the handle (pointers advanced to the range, row map offset), and the sorted
// per-range lists are merged on the host in the canonical (distance, row) order (VectorStore::merge_results semantics,
// vector_store.rs:953-970 — the reference's own segments are merged the same way).  Exclusive: the view borrows the handle.
// With a subset filter (search_filtered, flat_mmap.rs:498-560: k.min(subset.len())) every range is searched with the ids of
// the subset that fall into it.
static int search_large_k(lynse_hip_flat* h, const void* q_src, bool packed_queries, uint64_t nq, uint32_t k, int metric,
                          uint64_t* out_rows, float* out_dists, uint32_t* out_counts, bool on_device, hipStream_t user_stream,
                          const uint64_t* subset, uint64_t n_subset, bool filtered, const uint64_t* bitset_words, uint64_t n_words) {
    LY_WRITER(h, xlk);
    LY_TRY(use_device(h));
    const bool binary = metric >= M_HAMMING;
    if (packed_queries && !binary) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "packed queries need a binary metric");
    if (!binary && h->packed_only) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "store holds packed rows; float metrics unavailable");
    if (binary) LY_TRY(ensure_packed_locked(h));
    else { LY_TRY(finalize_locked(h)); LY_TRY(ensure_shadow_locked(h)); }   // (the row-range views below scan the f16 shadow: built for the WHOLE shard first)
    const uint64_t n = h->n, R = h->cap;
    // the subset as a sorted set of valid row ids (a BitSet's to_vec; ids >= n are skipped, duplicates count once)
    std::vector<uint64_t> ids;
    if (filtered) {
        if (bitset_words) {
            const uint64_t nw = std::min<uint64_t>(n_words, (n + 63) / 64);
            for (uint64_t w = 0; w < nw; ++w)
                for (uint64_t bits = bitset_words[w]; bits; bits &= bits - 1) {
                    const uint64_t r = w * 64 + (uint64_t)__builtin_ctzll(bits);
                    if (r < n) ids.push_back(r);
                }
        } else {
            ids.assign(subset, subset + n_subset);
            std::sort(ids.begin(), ids.end());
            ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
            while (!ids.empty() && ids.back() >= n) ids.pop_back();
        }
    }
    const uint32_t kk = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(k, n), filtered ? ids.size() : n);
    const uint64_t n_ranges = (n + R - 1) / R;
    const size_t q_elems = packed_queries ? h->words : h->dim, q_bytes = q_elems * (packed_queries ? 8 : 4);
    if (kk == 0) {  // an empty subset: empty results
        if (on_device) LY_TRY(memset_done(out_counts, 0, nq * 4));
        else memset(out_counts, 0, nq * 4);
        return LYNSE_OK;
    }
    // queries on the host (the per-range searches go through the host-array path)
    std::vector<uint8_t> q_host;
    const uint8_t* qh = reinterpret_cast<const uint8_t*>(q_src);
    if (on_device) {
        q_host.resize((size_t)nq * q_bytes);
        LY_HIP(hipMemcpy(q_host.data(), q_src, q_host.size(), hipMemcpyDeviceToHost));
        qh = q_host.data();
    }
    struct View {  // the scan-side fields of the handle, advanced to one row range for the duration of a call
        lynse_hip_flat* h;
        float* rows; _Float16 *rows16, *rows_h; float *vn2, *vrinv; uint64_t* packed;
        uint64_t n, n_stats, n16, n_packed, row_offset;
        explicit View(lynse_hip_flat* hh) : h(hh), rows(hh->rows), rows16(hh->rows16), rows_h(hh->rows_h), vn2(hh->vn2), vrinv(hh->vrinv), packed(hh->packed),
                                            n(hh->n), n_stats(hh->n_stats), n16(hh->n16), n_packed(hh->n_packed), row_offset(hh->row_offset) {}
        void set(uint64_t r0, uint64_t r1) {
            h->rows = rows ? rows + r0 * h->ld : nullptr;
            h->rows_h = rows_h ? rows_h + r0 * h->ld16 : nullptr;
            h->rows16 = rows16 ? rows16 + r0 * h->ld16 : nullptr;
            h->vn2 = vn2 ? vn2 + r0 : nullptr;
            h->vrinv = vrinv ? vrinv + r0 : nullptr;
            h->packed = packed ? packed + r0 * h->words : nullptr;
            h->n = r1 - r0;
            h->n_stats = h->n; h->n16 = rows16 ? h->n : 0; h->n_packed = packed ? h->n : 0;
            h->row_offset = row_offset + r0 * h->row_stride;
        }
        ~View() {
            h->rows = rows; h->rows_h = rows_h; h->rows16 = rows16; h->vn2 = vn2; h->vrinv = vrinv; h->packed = packed;
            h->n = n; h->n_stats = n_stats; h->n16 = n16; h->n_packed = n_packed; h->row_offset = row_offset;
        }
    } view(h);
    // the IP accumulation form follows the size of the WHOLE shard (flat_mmap.rs:4852-4854), not of a range
    struct FormGuard { lynse_hip_flat* h; int f; ~FormGuard() { h->ip_form = f; } } form_guard{h, h->ip_form};
    if (h->ip_form == LYNSE_IPFORM_AUTO) h->ip_form = n < 4096 ? LYNSE_IPFORM_SINGLE : LYNSE_IPFORM_BATCH8;
    const uint64_t qb = std::max<uint64_t>(1, std::min<uint64_t>(QCHUNK, (64ull << 20) / std::max<uint64_t>(1, n_ranges * kk * 12)));  // queries per pass (<= 64 MB of lists)
    std::vector<uint64_t> l_rows((size_t)qb * n_ranges * kk), m_rows(kk);
    std::vector<float> l_dists((size_t)qb * n_ranges * kk), m_dists(kk);
    std::vector<uint32_t> l_counts((size_t)qb * n_ranges), r_counts(qb);
    std::vector<uint64_t> t_rows((size_t)qb * kk);
    std::vector<float> t_dists((size_t)qb * kk);
    std::vector<uint64_t> o_rows(on_device ? (size_t)nq * k : 0);
    std::vector<float> o_dists(on_device ? (size_t)nq * k : 0);
    std::vector<uint32_t> o_counts(on_device ? nq : 0);
    uint64_t* res_rows = on_device ? o_rows.data() : out_rows;
    float* res_dists = on_device ? o_dists.data() : out_dists;
    uint32_t* res_counts = on_device ? o_counts.data() : out_counts;
    for (uint64_t q0 = 0; q0 < nq; q0 += qb) {
        const uint64_t nb = std::min<uint64_t>(qb, nq - q0);
        for (uint64_t ri = 0; ri < n_ranges; ++ri) {
            const uint64_t r0 = ri * R, r1 = std::min<uint64_t>(n, r0 + R);
            uint32_t kr = (uint32_t)std::min<uint64_t>(kk, r1 - r0);
            std::vector<uint64_t> local;   // the subset ids of this range, range-local
            if (filtered) {
                const auto lo = std::lower_bound(ids.begin(), ids.end(), r0), hi = std::lower_bound(ids.begin(), ids.end(), r1);
                local.assign(lo, hi);
                for (uint64_t& v : local) v -= r0;
                kr = (uint32_t)std::min<uint64_t>(kr, local.size());
                if (local.empty()) {
                    for (uint64_t q = 0; q < nb; ++q) l_counts[q * n_ranges + ri] = 0;
                    continue;
                }
            }
            view.set(r0, r1);
            const int rc = search_impl(h, qh + q0 * q_bytes, packed_queries, nb, kr, metric, t_rows.data(), t_dists.data(), r_counts.data(),
                                       false, user_stream, filtered ? local.data() : nullptr, local.size(), filtered, nullptr, 0, true);
            if (rc != LYNSE_OK) return rc;
            for (uint64_t q = 0; q < nb; ++q) {  // [query][range][kk] lists for the merge
                const uint32_t c = r_counts[q];
                l_counts[q * n_ranges + ri] = c;
                memcpy(&l_rows[(q * n_ranges + ri) * kk], &t_rows[q * kr], (size_t)c * 8);
                memcpy(&l_dists[(q * n_ranges + ri) * kk], &t_dists[q * kr], (size_t)c * 4);
            }
        }
        for (uint64_t q = 0; q < nb; ++q) {
            uint32_t cnt = 0;
            LY_TRY(lynse_hip_merge_topk(&l_rows[q * n_ranges * kk], &l_dists[q * n_ranges * kk], &l_counts[q * n_ranges], (uint32_t)n_ranges, kk, kk,
                                        metric, m_rows.data(), m_dists.data(), &cnt));
            memcpy(res_rows + (q0 + q) * k, m_rows.data(), (size_t)cnt * 8);
            memcpy(res_dists + (q0 + q) * k, m_dists.data(), (size_t)cnt * 4);
            res_counts[q0 + q] = cnt;
        }
    }
    if (on_device) {
        LY_TRY(h2d_done(out_rows, o_rows.data(), o_rows.size() * 8));
        LY_TRY(h2d_done(out_dists, o_dists.data(), o_dists.size() * 4));
        LY_TRY(h2d_done(out_counts, o_counts.data(), o_counts.size() * 4));
    }
    return LYNSE_OK;
}

// FLAT-*-SQ8 with more pass-1 candidates than one pass holds (n_cand = 20 k, cosine 100 k, flat_mmap.rs:5883-5893; above
// cap / 4 over more than cap rows): pass 1 runs per row range of `cap` rows (exact top-n_cand of the integer code scores
// there), the per-range lists are merged on the host in the (score, row) order, and pass 2 — the exact f32 scores of the
// n_cand rows, (distance, row) order, top k — is the subset-filtered exact search over those rows (single-row kernels, as
// flat_mmap.rs:5899-5906).  One query at a time: a rare shape, not a tuned one.  Called with the writer lock held.
static int search_sq8_large(lynse_hip_flat* h, std::unique_lock<std::shared_mutex>& lk, const float* queries, uint64_t nq, uint32_t k, uint32_t kk,
                            uint32_t n_cand, int metric, uint64_t* out_rows, float* out_dists, uint32_t* out_counts) {
    const uint64_t n = h->n, R = h->cap, n_ranges = (n + R - 1) / R;
    const int m1 = metric == M_IP ? M_IP : M_L2;
    LY_TRY(ensure_workspace(h, (uint32_t)std::min<uint64_t>(n_cand, R)));
    Workspace& w = cur(h).ws;
    hipStream_t st = cur(h).stream;
    struct Sq8View {  // the pass-1 side of the handle advanced to one row range; rows come back as RAW shard rows
        lynse_hip_flat* h;
        float* rows; CodeSet sq8; uint64_t n, stride, offset;
        explicit Sq8View(lynse_hip_flat* hh) : h(hh), rows(hh->rows), sq8(hh->sq8), n(hh->n),
                                               stride(hh->row_stride), offset(hh->row_offset) {}
        void set(uint64_t r0, uint64_t r1) {
            h->rows = rows + r0 * h->ld; h->sq8.codes = sq8.codes + r0 * sq8.ld; h->sq8.sum = sq8.sum + r0; h->sq8.sum2 = sq8.sum2 + r0;
            h->n = r1 - r0; h->sq8.n = h->n; h->row_stride = 1; h->row_offset = r0;
        }
        void restore() { h->rows = rows; h->sq8 = sq8; h->n = n; h->row_stride = stride; h->row_offset = offset; }
        ~Sq8View() { restore(); }
    };
    std::vector<std::vector<uint64_t>> cand(nq);   // per query: the top-n_cand rows of pass 1
    {
        Sq8View view(h);
        const uint64_t qb = std::max<uint64_t>(1, std::min<uint64_t>(QCHUNK, (64ull << 20) / std::max<uint64_t>(1, n_ranges * n_cand * 12)));
        std::vector<uint64_t> l_rows((size_t)qb * n_ranges * n_cand), m_rows(n_cand), t_rows;
        std::vector<float> l_dists((size_t)qb * n_ranges * n_cand), m_dists(n_cand), t_dists;
        std::vector<uint32_t> l_counts((size_t)qb * n_ranges);
        for (uint64_t q0 = 0; q0 < nq; q0 += qb) {
            const uint32_t nb = (uint32_t)std::min<uint64_t>(qb, nq - q0);
            LY_HIP(hipMemcpyAsync(w.Qf, queries + q0 * h->dim, (size_t)nb * h->dim * 4, hipMemcpyHostToDevice, st));
            for (uint64_t ri = 0; ri < n_ranges; ++ri) {
                const uint64_t r0 = ri * R, r1 = std::min<uint64_t>(n, r0 + R);
                const uint32_t kr = (uint32_t)std::min<uint64_t>(n_cand, r1 - r0);
                view.set(r0, r1);
                for (int level = 1; level < 3; ++level) {
                    LY_TRY(run_chunk_sq8(h, nb, kr, kr, kr, metric, level, st, true));
                    LY_HIP(hipMemcpyAsync(w.h_hdr, w.out_counts, (size_t)2 * w.qcap * 4, hipMemcpyDeviceToHost, st));
                    LY_HIP(hipStreamSynchronize(st));
                    uint32_t nov = 0;
                    for (uint32_t i = 0; i < nb; ++i) nov += w.h_hdr[w.qcap + i] ? 1 : 0;
                    if (nov == 0) break;
                    if (level == 2) return set_error(LYNSE_ERR_INTERNAL, "candidate overflow on the exhaustive plan");
                }
                t_rows.resize((size_t)nb * kr);
                t_dists.resize((size_t)nb * kr);
                LY_HIP(hipMemcpy(t_rows.data(), w.out_rows, t_rows.size() * 8, hipMemcpyDeviceToHost));
                LY_HIP(hipMemcpy(t_dists.data(), w.out_dists, t_dists.size() * 4, hipMemcpyDeviceToHost));
                for (uint32_t q = 0; q < nb; ++q) {
                    const uint32_t c = w.h_hdr[q];
                    l_counts[q * n_ranges + ri] = c;
                    memcpy(&l_rows[(q * n_ranges + ri) * n_cand], &t_rows[(size_t)q * kr], (size_t)c * 8);
                    memcpy(&l_dists[(q * n_ranges + ri) * n_cand], &t_dists[(size_t)q * kr], (size_t)c * 4);
                }
            }
            for (uint32_t q = 0; q < nb; ++q) {
                uint32_t cnt = 0;
                LY_TRY(lynse_hip_merge_topk(&l_rows[(size_t)q * n_ranges * n_cand], &l_dists[(size_t)q * n_ranges * n_cand], &l_counts[(size_t)q * n_ranges],
                                            (uint32_t)n_ranges, n_cand, n_cand, m1, m_rows.data(), m_dists.data(), &cnt));
                cand[q0 + q].assign(m_rows.begin(), m_rows.begin() + cnt);
            }
        }
    }
    // pass 2 through the public filtered path (it takes the locks itself; large k there goes through the row-range views)
    lk.unlock();
    for (uint64_t q = 0; q < nq; ++q) {
        LY_TRY(search_impl(h, queries + q * h->dim, false, 1, k, metric, out_rows + q * k, out_dists + q * k, out_counts + q, false, nullptr,
                           cand[q].data(), cand[q].size(), true));
        (void)kk;
    }
    return LYNSE_OK;
}

// ids 7-10 leave before the staged pipeline (additive_host.inc)
static int additive_search(lynse_hip_flat* h, const float* queries, uint64_t nq, uint32_t k, int metric, bool filtered,
                           const uint64_t* subset, uint64_t n_subset, const uint64_t* bitset_words, uint64_t n_words,
                           uint64_t* out_rows, float* out_dists, uint32_t* out_counts);

extern "C" int lynse_hip_flat_search_f32(lynse_hip_flat* h, const float* queries, uint64_t nq, uint32_t k, int metric,
                                         uint64_t* out_rows, float* out_dists, uint32_t* out_counts) {
    if (metric_additive(metric)) return additive_search(h, queries, nq, k, metric, false, nullptr, 0, nullptr, 0, out_rows, out_dists, out_counts);
    return search_impl(h, queries, false, nq, k, metric, out_rows, out_dists, out_counts, false, nullptr);
}

extern "C" int lynse_hip_flat_search_filtered_f32(lynse_hip_flat* h, const float* queries, uint64_t nq, uint32_t k, int metric,
                                                  const uint64_t* subset_rows, uint64_t n_subset, uint64_t* out_rows,
                                                  float* out_dists, uint32_t* out_counts) {
    if (metric_additive(metric)) return additive_search(h, queries, nq, k, metric, true, subset_rows, n_subset, nullptr, 0, out_rows, out_dists, out_counts);
    return search_impl(h, queries, false, nq, k, metric, out_rows, out_dists, out_counts, false, nullptr, subset_rows, n_subset, true);
}

extern "C" int lynse_hip_flat_search_filtered_bitset_f32(lynse_hip_flat* h, const float* queries, uint64_t nq, uint32_t k, int metric,
                                                         const uint64_t* bitset_words, uint64_t n_words, uint64_t* out_rows,
                                                         float* out_dists, uint32_t* out_counts) {
    if (!h) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "handle is NULL");
    if (n_words && !bitset_words) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "bitset is NULL");
    if (metric_additive(metric)) {   // (an empty BitSet is still a filter: no rows)
        static const uint64_t none = 0;
        return additive_search(h, queries, nq, k, metric, true, nullptr, 0, bitset_words ? bitset_words : &none, n_words, out_rows, out_dists, out_counts);
    }
    const uint64_t n = lynse_hip_flat_len(h);
    uint64_t count = 0;  // BitSet::count() restricted to rows below len
    const uint64_t full = std::min<uint64_t>(n_words, n / 64);
    for (uint64_t w = 0; w < full; ++w) count += (uint64_t)__builtin_popcountll(bitset_words[w]);
    if (full < n_words && (n % 64)) count += (uint64_t)__builtin_popcountll(bitset_words[full] & ((1ull << (n % 64)) - 1ull));
    return search_impl(h, queries, false, nq, k, metric, out_rows, out_dists, out_counts, false, nullptr, nullptr, count, true,
                       bitset_words, n_words);
}

extern "C" int lynse_hip_flat_search_f32_device(lynse_hip_flat* h, const float* d_queries, uint64_t nq, uint32_t k,
                                                int metric, uint64_t* d_out_rows, float* d_out_dists,
                                                uint32_t* d_out_counts, void* stream) {
    return search_impl(h, d_queries, false, nq, k, metric, d_out_rows, d_out_dists, d_out_counts, true, (hipStream_t)stream);
}

extern "C" int lynse_hip_flat_search_packed_u64(lynse_hip_flat* h, const uint64_t* qw, uint64_t nq, uint32_t k, int metric,
                                                uint64_t* out_rows, float* out_dists, uint32_t* out_counts) {
    return search_impl(h, qw, true, nq, k, metric, out_rows, out_dists, out_counts, false, nullptr);
}

extern "C" int lynse_hip_flat_search_packed_u64_device(lynse_hip_flat* h, const uint64_t* d_qw, uint64_t nq, uint32_t k,
                                                       int metric, uint64_t* d_out_rows, float* d_out_dists,
                                                       uint32_t* d_out_counts, void* stream) {
    return search_impl(h, d_qw, true, nq, k, metric, d_out_rows, d_out_dists, d_out_counts, true, (hipStream_t)stream);
}

// --------------------------------------------------------------------------- stand-alone calls ----
extern "C" int lynse_hip_top_k_search(const float* query, const float* candidates, uint64_t n, uint32_t dim, uint32_t k,
                                      int metric, int device, uint32_t* out_idx, float* out_dist, uint32_t* out_count) {
    // distance::top_k_search (distance/mod.rs:373-422): single-row kernels for every candidate.
    if (!out_count) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "out_count is NULL");
    *out_count = 0;
    if (!metric_valid(metric)) return set_error(LYNSE_ERR_UNKNOWN_METRIC, "Unknown metric id");
    if (dim == 0) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "dimension must be greater than zero");
    if (n == 0 || k == 0) return LYNSE_OK;
    if (!query || !candidates || !out_idx || !out_dist) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    // A scratch shard per calling thread and (device, dim), emptied and refilled per call: py_top_k_search / py_compute_distance /
    // Collection::pending_search call this in loops, and a handle (stream, stats buffers, workspace) is not free to create.
    struct Scratch {
        lynse_hip_flat* h = nullptr; int device = -1; uint32_t dim = 0;
        ~Scratch() { if (h) lynse_hip_flat_destroy(h); }
    };
    static thread_local Scratch sc;
    if (!sc.h || sc.device != device || sc.dim != dim) {
        if (sc.h) { lynse_hip_flat_destroy(sc.h); sc.h = nullptr; }
        LY_TRY(lynse_hip_flat_create(dim, device, &sc.h));
        sc.device = device; sc.dim = dim;
        LY_TRY(lynse_hip_flat_set_ip_form(sc.h, LYNSE_IPFORM_SINGLE));
    }
    lynse_hip_flat* h = sc.h;
    {   // empty the shard (capacity and buffers stay)
        std::unique_lock<std::shared_mutex> lk(h->rw);
        h->n = 0; h->n_stats = 0; h->n16 = 0; h->n_packed = 0; h->sq8.n = 0; h->sq7.n = 0; h->sq7_strikes.store(0); h->sq8a.n = 0; h->sq8c.n = 0; h->n_bpm = 0; h->i8c_strikes.store(0); h->i8c_strikes_l2.store(0); h->i8c_strikes_cos.store(0);
        h->amax = h->vmax = h->vmin = 0.f; h->sv = 1.f; h->cos_degenerate = 0; h->rows_integer = 0; h->rows_nonneg = 0;
        const uint32_t init[5] = {0u, 0u, 0x7f800000u, 0u, 0u};
        LY_TRY(use_device(h));
        approx_release(h);
        LY_TRY(h2d_done(h->d_stats, init, sizeof init));
    }
    int rc = lynse_hip_flat_append_f32(h, candidates, n);
    const uint32_t kk = (uint32_t)std::min<uint64_t>(k, n);
    std::vector<uint64_t> rows(kk);
    uint32_t cnt = 0;
    if (rc == LYNSE_OK) rc = lynse_hip_flat_search_f32(h, query, 1, kk, metric, rows.data(), out_dist, &cnt);
    if (rc != LYNSE_OK) return rc;
    for (uint32_t i = 0; i < cnt; ++i) out_idx[i] = (uint32_t)rows[i];
    *out_count = cnt;
    return LYNSE_OK;
}

extern "C" int lynse_hip_compute_distance(const float* a, const float* b, uint32_t dim, int metric, int device, float* out) {
    // distance::compute_distance_f32(a, b) (distance/mod.rs:193-213): a plays the query.
    if (!a || !b || !out) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    uint32_t idx = 0, cnt = 0;
    float d = 0.f;
    LY_TRY(lynse_hip_top_k_search(a, b, 1, dim, 1, metric, device, &idx, &d, &cnt));
    if (cnt != 1) return set_error(LYNSE_ERR_INTERNAL, "distance kernel returned no result");
    *out = d;
    return LYNSE_OK;
}

extern "C" int lynse_hip_pack_binary_f32(const float* rows, uint64_t n, uint32_t dim, int device, uint64_t* out_words) {
    if (n == 0) return LYNSE_OK;
    if (!rows || !out_words) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    lynse_hip_flat* h = nullptr;
    LY_TRY(lynse_hip_flat_create(dim, device, &h));
    int rc = lynse_hip_flat_append_f32(h, rows, n);
    if (rc == LYNSE_OK) rc = lynse_hip_flat_read_packed(h, 0, n, out_words);
    lynse_hip_flat_destroy(h);
    return rc;
}

extern "C" int lynse_hip_merge_topk(const uint64_t* ids, const float* dists, const uint32_t* counts, uint32_t n_lists,
                                    uint32_t stride, uint32_t k, int metric, uint64_t* out_ids, float* out_dists,
                                    uint32_t* out_count) {
    // VectorStore::merge_results (vector_store.rs:953-970): (distance in metric order, id ascending).
    if (!out_count) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "out_count is NULL");
    *out_count = 0;
    if (!metric_valid(metric)) return set_error(LYNSE_ERR_UNKNOWN_METRIC, "Unknown metric id");
    if (n_lists == 0 || k == 0) return LYNSE_OK;
    if (!ids || !dists || !counts || !out_ids || !out_dists) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    const bool asc = metric_ascending(metric);
    struct E { float d; uint64_t id; };
    std::vector<E> all;
    for (uint32_t l = 0; l < n_lists; ++l) {
        if (counts[l] > stride) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "count exceeds stride");
        for (uint32_t i = 0; i < counts[l]; ++i) all.push_back({dists[(size_t)l * stride + i], ids[(size_t)l * stride + i]});
    }
    auto before = [asc](const E& x, const E& y) {
        if (x.d < y.d) return asc;
        if (x.d > y.d) return !asc;
        return x.id < y.id;  // NaN compares Equal like partial_cmp().unwrap_or(Equal)
    };
    const size_t kk = std::min<size_t>(k, all.size());
    std::partial_sort(all.begin(), all.begin() + kk, all.end(), before);
    for (size_t i = 0; i < kk; ++i) { out_ids[i] = all[i].id; out_dists[i] = all[i].d; }
    *out_count = (uint32_t)kk;
    return LYNSE_OK;
}

static int merge_topk_device_impl(const void* d_blocks, uint64_t block_bytes, uint64_t rows_off,
                                  uint64_t dists_off, uint64_t counts_off, uint32_t n_lists, uint64_t nq,
                                  uint32_t k, int metric, uint64_t* d_out_rows, float* d_out_dists,
                                  uint32_t* d_out_counts, void* stream, uint64_t status_off, uint32_t* out_status) {
    LY_TRY(metric_check(metric));
    if (nq == 0) return LYNSE_OK;
    if (!d_blocks || !d_out_counts || (k && (!d_out_rows || !d_out_dists))) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_lists == 0) return set_error(LYNSE_ERR_INVALID_ARGUMENT, "n_lists is zero");
    if (k == 0) {
        LY_HIP(hipMemsetAsync(d_out_counts, 0, nq * 4, (hipStream_t)stream));
        return LYNSE_OK;
    }
    const uint64_t total = (uint64_t)n_lists * k;
    if (total > 8192) return set_error(LYNSE_ERR_UNSUPPORTED, "n_lists * k exceeds the merge kernel capacity (8192)");
    uint32_t np2 = 2;
    while (np2 < total) np2 <<= 1;
    LY_TRY(ensure_lds<k_merge<256>>(8192 * 12));
    MergeArgs a{};
    a.blocks = (const char*)d_blocks; a.block_bytes = block_bytes; a.rows_off = rows_off; a.dists_off = dists_off;
    a.counts_off = counts_off; a.n_lists = n_lists; a.k = k; a.metric = metric;
    a.out_rows = d_out_rows; a.out_dists = d_out_dists; a.out_counts = d_out_counts;
    a.status_off = status_off; a.out_status = out_status;
    hipLaunchKernelGGL(k_merge<256>, dim3((uint32_t)nq), dim3(256), (size_t)np2 * 12, (hipStream_t)stream, a);
    LY_HIP(hipGetLastError());
    return LYNSE_OK;
}

extern "C" int lynse_hip_merge_topk_device(const void* d_blocks, uint64_t block_bytes, uint64_t rows_off,
                                           uint64_t dists_off, uint64_t counts_off, uint32_t n_lists, uint64_t nq,
                                           uint32_t k, int metric, uint64_t* d_out_rows, float* d_out_dists,
                                           uint32_t* d_out_counts, void* stream) {
    return merge_topk_device_impl(d_blocks, block_bytes, rows_off, dists_off, counts_off, n_lists, nq, k, metric, d_out_rows,
                                  d_out_dists, d_out_counts, stream, 0, nullptr);
}

// ---------------------------------------------------------------------------------------------- bounded waits ----
// Every host wait that ends in a COLLECTIVE (the all-gather of a sharded batch, the all-reduce of a Lloyd iteration) is bounded: a rank
// that died or returned early must not strand its peers inside hipStreamSynchronize for good.  The reference's coordinator retries a
// shard once and errors (src/cluster.rs:243-261).  lynse_hip_set_wait_timeout_ms / LYNSE_HIP_WAIT_TIMEOUT_MS; 0 = 30 s for waits behind a
// collective, unbounded for one shard alone.
static std::atomic<uint32_t> g_wait_timeout_ms{[]() { const char* e = env_str("LYNSE_HIP_WAIT_TIMEOUT_MS"); return e ? (uint32_t)atoll(e) : 0u; }()};
extern "C" int lynse_hip_set_wait_timeout_ms(uint32_t ms) { g_wait_timeout_ms.store(ms); return LYNSE_OK; }
static uint32_t collective_timeout_ms() { const uint32_t to = g_wait_timeout_ms.load(); return to ? to : 30000u; }

// hipEventSynchronize with an upper bound: polls the event (spinning first: a batch is a millisecond or two), sleeps in between
static int event_wait_bounded(hipEvent_t ev, uint32_t timeout_ms) {
    if (timeout_ms == 0) { LY_HIP(hipEventSynchronize(ev)); return LYNSE_OK; }
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t q = hipEventQuery(ev);
        if (q == hipSuccess) return LYNSE_OK;
        if (q != hipErrorNotReady) return set_error(LYNSE_ERR_DEVICE, std::string("hipEventQuery: ") + hipGetErrorString(q));
        const auto el = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
        if (el > (int64_t)timeout_ms * 1000) return set_error(LYNSE_ERR_TIMEOUT, "the batch did not finish within the wait timeout (a rank of the collective is gone?)");
        if (el > 2000) std::this_thread::sleep_for(std::chrono::microseconds(el > 100000 ? 1000 : 50));
    }
}
// ... of everything enqueued on `st` so far, through an event of the caller (created on first use)
static int stream_wait_bounded(hipStream_t st, hipEvent_t* ev, uint32_t timeout_ms) {
    if (!*ev) LY_HIP(hipEventCreateWithFlags(ev, hipEventDisableTiming));
    LY_HIP(hipEventRecord(*ev, st));
    return event_wait_bounded(*ev, timeout_ms);
}
// Status word of a result block (comm_block_layout), OR-ed over the ranks by the merge.  The low byte asks for the batch to be
// answered again, on every rank: bit 0 = a query of that shard overflowed its candidate buffers (next plan level), bit 1 = an IVF query
// whose probed lists are all empty (k_or_word: the scan-every-list fallback of ivf.rs:258-265).  Any bit ABOVE the low byte = that rank
// FAILED while it built its block (the failing rank fills the word's bytes with 2: hipMemsetAsync) — it still takes part in the
// exchange (with an empty block), so that its peers learn of it from the merged word instead of from a timeout.
constexpr uint32_t STATUS_OVERFLOW = 1u, STATUS_EMPTY_LISTS = 2u, STATUS_REDO = STATUS_OVERFLOW | STATUS_EMPTY_LISTS;
static inline bool status_failed(uint32_t st) { return (st & 0xffffff00u) != 0u; }

#include "rerank_host.inc"
#include "ivf_host.inc"
#include "spann_host.inc"
#include "shard_host.inc"
#include "comm_host.inc"
#include "async_host.inc"
#include "ivf_async.inc"
#include "coded_host.inc"
#include "pq_host.inc"
#include "rabitq_host.inc"
#include "polarvec_host.inc"
#include "graph_host.inc"
#include "hnsw_host.inc"
#include "diskann_host.inc"
#include "range_host.inc"
#include "additive_host.inc"
#include "approx_host.inc"
#include "sparse_host.inc"
#include "text_host.inc"
#include "fields_host.inc"
#include "mutate_host.inc"
