/*
 * lynse_hip.h — C ABI of liblynse_hip.so: the MI355X (gfx950) implementation of LynseDB's
 * FLAT / IVF-Flat search hot path (src/distance + the FLAT/IVF search in src/index, src/storage).
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types.  Each entry point
 * names the reference interface it replaces (file:line relative to BirchKwok/lynsedb).  The
 * reference-side binding a maintainer would add (Rust `extern "C"` + the PyO3 glue that already
 * exists) is shown in INTEGRATION.md.
 *
 * Conventions (mirroring the reference boundary):
 *  - inputs are borrowed for the duration of the call; outputs are CALLER-allocated, fixed size
 *    (nq*k), short results are padded (row ~0, distance +inf / -inf: the worst of the metric) and the true length is
 *    written to out_counts[q];
 *  - empty store or k == 0 -> counts 0, not an error (flat_mmap.rs:832-835); k > N clamps (:836);
 *  - rows returned are ROW INDICES (u32 per segment in the reference, u64 here after the row map),
 *    best-first; ties are ordered by row ascending — the order VectorStore::merge_results imposes
 *    (vector_store.rs:953-970);
 *  - distances: IP raw dot (descending), L2 squared, cosine distance, Hamming/Jaccard/Dice as f32;
 *  - every function returns a status code (LynseError variants, src/error.rs:5-52); the message is
 *    available per thread from lynse_hip_last_error(); nothing throws or aborts across the ABI;
 *  - NON-FINITE VALUES.  The reference compares distances with partial_cmp(..).unwrap_or(Equal) (flat_mmap.rs:2141-2149,
 *    :2170-2176): a NaN distance is "equal" to everything, is never admitted once a top-k array is full and stays wherever the first
 *    fill put it — the result depends on the row order and the thread count.  This boundary pins ONE order instead: a NaN score is
 *    reported as the WORST value of the metric (+inf for the distances, -inf for IP) and ranks behind every better score, ties by
 *    ascending row like any other tie; +inf / -inf scores are ordinary values of the order.  A query with a NaN element (cosine: or
 *    an infinite one) scores NaN against every row: an unfiltered FLAT search answers it with rows 0 .. min(k, N) - 1 at the worst
 *    value — the rows the reference's first fill keeps.  Rows may hold NaN / +-inf elements (the certified int8 pass switches itself
 *    off for such a shard).  Pinned by tests/test_gpu_flat_parity.py::test_nan_and_infinite_rows_and_queries.
 *  - a handle may be searched from several threads: unfiltered searches run under a SHARED lock, each on one of the handle's
 *    search contexts (stream + workspace, up to LYNSE_HIP_CONTEXTS = 8 at a time, further callers wait for a free one) — the
 *    Arc<RwLock<Collection>>::read of the reference (src/python/mod.rs:950, :1187); append / finalize / lazy builds of derived copies
 *    and the gathered-rows strategy of a subset filter take the lock EXCLUSIVE, like `&mut self` in FlatMmap::write, and are
 *    refused while tickets of lynse_hip_flat_search_submit_* are outstanding.
 *  - there is NO CPU fallback: without a usable HIP device every compute entry returns
 *    LYNSE_ERR_DEVICE.
 */
#ifndef LYNSE_HIP_H
#define LYNSE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LYNSE_HIP_ABI_VERSION 1

/* Status codes — src/error.rs:5-52 (DimensionMismatch / InvalidArgument / IndexNotBuilt / Io ...). */
enum {
    LYNSE_OK = 0,
    LYNSE_ERR_INVALID_ARGUMENT = 1,
    LYNSE_ERR_DIMENSION_MISMATCH = 2,
    LYNSE_ERR_UNKNOWN_METRIC = 3,
    LYNSE_ERR_NOT_FINALIZED = 4,
    LYNSE_ERR_OUT_OF_MEMORY = 5,
    LYNSE_ERR_DEVICE = 6,
    LYNSE_ERR_INTERNAL = 7,
    LYNSE_ERR_INDEX_NOT_BUILT = 8,
    LYNSE_ERR_UNSUPPORTED = 9,
    LYNSE_ERR_TIMEOUT = 10 /* lynse_hip_flat_search_wait: the batch did not finish within the wait timeout (a peer rank is gone) */
};

/* Metric ids — DistanceMetric (src/distance/mod.rs:19-36), in-scope subset. */
enum {
    LYNSE_METRIC_IP = 0,
    LYNSE_METRIC_L2 = 1,
    LYNSE_METRIC_COSINE = 2,
    LYNSE_METRIC_HAMMING = 3,
    LYNSE_METRIC_JACCARD = 4,
    LYNSE_METRIC_DICE = 5,
    LYNSE_METRIC_TANIMOTO = 6,
    LYNSE_METRIC_L1 = 7,          /* the additive metrics: see the contract below */
    LYNSE_METRIC_CHEBYSHEV = 8,
    LYNSE_METRIC_CANBERRA = 9,
    LYNSE_METRIC_BRAY_CURTIS = 10
};
/* THE ADDITIVE METRICS (ids 7-10; the reference's `supports_flat_approx` group, src/distance/mod.rs:177-188, FLAT-L1 / -MANHATTAN /
 * -CITYBLOCK / -CHEBYSHEV / -CHEBYCHEV / -LINF / -CANBERRA / -BRAY-CURTIS / -BRAYCURTIS, src/index/mod.rs:426-495).  All four are
 * ascending.  The distance of a query a and a row b of D floats is the reference's AVX2 form bit for bit, all in f32, nothing fused:
 *   shape  chunks = D / 8; lane g of an 8-lane accumulator takes the elements 8 i + g, i = 0 .. chunks - 1, in order; the lanes are
 *          then reduced SEQUENTIALLY from lane 0 to lane 7 (not the pairwise tree of ip / l2 / cosine); the D % 8 tail elements
 *          are folded in one by one after that.
 *   L1           lane: acc += |a - b|; reduce: 0.0 + l0 + ... + l7; tail: sum += |a - b|.
 *   Chebyshev    lane: acc = (acc > d) ? acc : d with d = |a - b| (_mm256_max_ps: d whenever either operand is NaN, so a NaN step
 *                erases what the lane held and the next non-NaN step replaces the NaN); reduce and tail: f32::max from 0.0, which
 *                returns the non-NaN operand — a NaN left in a lane by its last step is dropped, the result is never NaN.
 *   Canberra     lane: den = |a| + |b|, q = |a - b| / den (IEEE), acc += (den != 0, ordered) ? q : +0 — a NaN den adds +0 in the
 *                body; reduce as L1; tail: if (den != 0.0) sum += |a - b| / den — plain !=, so a NaN den DOES add NaN there.
 *   Bray-Curtis  num += |a - b| and den += |a + b|, both reduced and tailed as L1; den == 0 ? (num == 0 ? 0 : +inf) : num / den.
 * Searches follow the NON-FINITE VALUES rule and the canonical order above: a NaN distance is reported as +inf, the order is
 * (distance, row ascending), min(k, live rows) entries come back.
 * Accepted by lynse_hip_flat_search_f32 / _filtered_f32 / _filtered_bitset_f32 (an exact scan of every row into a score matrix, the
 * cut and order of the range search; the call holds the handle's lock exclusively, runs on context 0, is refused while tickets are
 * outstanding and goes in query chunks like the range search), lynse_hip_flat_search_range_f32, lynse_hip_top_k_search,
 * lynse_hip_compute_distance, and as ascending metrics by lynse_hip_merge_topk / lynse_hip_merge_row_results /
 * lynse_hip_metric_is_ascending (1) / lynse_hip_metric_is_binary (0).
 * Refused with LYNSE_ERR_UNSUPPORTED: top-k on an F16 shard (the f16 sequential forms are not built; the range search scores the
 * decoded rows), a packed-only handle, a row-mapped handle, a row too wide for a query and a row to share the LDS — and every other
 * entry that takes a metric id (IVF / SPANN, SQ8, PQ, RaBitQ, packed queries, the _device, submit and sharded forms, prepare,
 * coarse_scores, merge_topk_device).  Ids outside 0-10 stay LYNSE_ERR_UNKNOWN_METRIC. */
/* THE APPROXIMATE FLAT SEARCH (Collection::search(approx = true, eps); FlatMmap::search's approx branch, src/storage/flat_mmap.rs:847-889,
 * src/storage/approx_search.rs).  Nothing is quantised: a coarse pass reads fewer bytes of the f32 rows — some of each row's dimensions,
 * or a cached order of the rows by their sums — and a pool of the best coarse rows is scored exactly.  One query per call, for ip, l2,
 * cosine and ids 7-10.  The shard is ONE segment (the reference applies the size tests per <= 256 MiB segment).  eps is normalised by
 * lynse_hip_normalize_eps first; it sizes the pool and the sample and rounds nothing here: the distances that come back are RAW, the
 * caller merges on them and rounds last (lynse_hip_round_distances_to_eps: v / eps, roundf — half away from zero —, times eps, in f32;
 * a non-finite value, quotient or product passes through).  big = dim > 16 and n > 65,536.  The paths, in the order they are tested:
 *   3  ip and big.  pool = lynse_hip_approx_ip_order_pool(k, n, eps) (<= 20,000).
 *        every query element >= 0: the pool is the `pool` rows with the LARGEST row sums, (sum descending, row ascending); every element
 *        <= 0 (and not the case before): the SMALLEST sums, (sum ascending, row ascending).  A row with a non-finite sum is left out.
 *        row sum: four 8-lane accumulators over chunks of 32 elements (accumulator j, lane g: element 32 c + 8 j + g), (acc0 + acc1) +
 *        (acc2 + acc3) per lane, the lanes added 0 -> 7 from 0.0, then the dim % 32 tail elements one by one.
 *        mixed signs (or a NaN): sample = lynse_hip_approx_hybrid_ip_sample_dims(dim, eps), pool = lynse_hip_approx_hybrid_ip_pool(k, n,
 *        eps); sample >= dim or pool >= n FALLS BACK to the exact search.  Else the coarse score of a row is acc = 0.0; acc += ip(q[block],
 *        row[block]) over the blocks of lynse_hip_approx_sampled_dim_blocks(dim, sample) in order, ip in the shard's IP form (below) on the
 *        block slice; the pool is the `pool` highest coarse scores.
 *        In all three cases the pool is scored with the single-row IP form; best k by (distance descending, row ascending).
 *   1  l2 and cosine, any size.  norm2[row] = the single-row IP form of the row with itself, inv[row] = norm2 > 1e-30 ? 1 / sqrt(norm2) : 0;
 *        q_norm2 / q_inv the same for the query.  dot = ip(q, row) in the shard's IP form.  l2: d = (q_norm2 + norm2[row]) - 2.0 * dot, three f32
 *        operations, then f32::max(d, 0.0) (a NaN becomes 0.0).  cosine: q_inv <= 0 answers rows 0 .. min(k, n) - 1 at 1.0; else d =
 *        inv[row] <= 0 ? 1.0 : 1.0 - (dot * q_inv) * inv[row].  Every row is scored; best k by (distance, row).
 *   4  ids 7-10 and big.  sample = lynse_hip_approx_hybrid_sample_dims(dim, eps), pool = lynse_hip_approx_hybrid_pool(k, n, eps); sample >= dim or
 *        pool >= n FALLS BACK to the exact search.  Coarse score over the blocks, each block slice in the metric's form above (THE ADDITIVE
 *        METRICS): l1 and canberra: (0.0 + s_0 + s_1 + s_2) * scale, scale = (f32)dim / (f32)sample; chebyshev: f32::max over the blocks from
 *        0.0; bray-curtis: ONE sequential chain over the blocks' elements in order (num += |a - b|, den += |a + b|, no lanes), then as above.
 *        The pool is the `pool` lowest coarse scores, scored exactly in the metric's form; best k by (distance, row).
 *   2  everything else (n <= 65,536 or dim <= 16; ip and ids 7-10).  Every row is scored exactly — ip ALWAYS in the single-row form, whatever n
 *        and lynse_hip_flat_set_ip_form say (the exact search uses the batch-of-8 form from 4,096 rows on), ids 7-10 as the exact search
 *        does —; best k by (distance, row).
 * The shard's IP form: what lynse_hip_flat_set_ip_form set, LYNSE_IPFORM_AUTO = single below 4,096 rows, batch-of-8 from there on.
 * Ties: wherever the reference leaves the order open (a selection on the score alone at the pool boundary, per-thread merges), the pool
 * is the best `pool` rows by the canonical key (coarse score in metric order, row ascending); a NaN coarse score orders last, with the
 * worst infinity, and -0.0 is +0.0.  Results follow the NON-FINITE VALUES rule like every search: min(k, n) entries.
 * out_info (may be NULL) tells what ran.  Derived copies (row sums, norms, the two sum orders per (n, pool)) are built by the first search
 * that needs them and dropped by append, update, compact and destroy.  Locking follows the additive search: the handle's lock held
 * exclusively, context 0, refused while tickets are outstanding; a path that is the exact search's (path 2 under ids 7-10, a fall-back)
 * runs lynse_hip_flat_search_f32 after the lock is released.  LYNSE_ERR_UNSUPPORTED: the binary metrics, an F16 shard, a packed-only
 * handle, a row-mapped handle, a row too wide for the LDS. */
typedef struct lynse_hip_approx_info {
    uint32_t path;        /* 1-4 as above; 0: nothing ran (n == 0 or k == 0) */
    uint32_t ip_case;     /* path 3: 1 = sum descending, 2 = sum ascending, 3 = hybrid; else 0 */
    uint32_t pool;        /* rows scored exactly after the coarse pass (paths 3 and 4; else 0) */
    uint32_t sample_dims; /* dimensions the coarse pass read per row (path 3 hybrid, path 4; else 0) */
    uint32_t fell_back;   /* 1: the size policy sent paths 3 / 4 to the exact search */
} lynse_hip_approx_info;

/* IP accumulation form of the exact rescoring pass. */
enum { LYNSE_IPFORM_AUTO = 0, LYNSE_IPFORM_SINGLE = 1, LYNSE_IPFORM_BATCH8 = 2,
       LYNSE_IPFORM_F16SEQ = 3 /* f16 storage: sequential sums of simd.rs:805-846 (set by the dtype, not by set_ip_form) */ };

/* Storage dtype of a float shard (src/storage/dtype.rs:6-29). */
enum { LYNSE_DTYPE_F32 = 0, LYNSE_DTYPE_F16 = 1 };

typedef struct lynse_hip_flat lynse_hip_flat; /* one HBM-resident FLAT shard: replaces FlatMmap */
typedef struct lynse_hip_ivf lynse_hip_ivf;   /* IVF-Flat over cluster slabs: replaces IVFIndex / IvfFlatMmap */

/* Per-search profile (the reference's QueryProfile, src/engine.rs:6906-6919, plus kernel timings
 * measured with HIP events on the launch stream).  Times in microseconds. */
typedef struct lynse_hip_profile {
    uint64_t searches;        /* profiled search calls accumulated */
    uint64_t scan_launches;   /* launches of the dominant scan kernel */
    double scan_us;           /* summed duration of those launches */
    uint64_t scan_rows;       /* rows scanned by those launches */
    uint64_t scan_bytes;      /* algorithmic bytes of those launches (rows * row bytes) */
    double total_us;          /* whole pipeline, first launch -> last launch */
    uint64_t fallback_queries;/* queries re-run on the exhaustive safe plan */
    uint64_t pool_entries;    /* candidates rescored exactly (sum over queries) */
    uint64_t last_plan;       /* plan of the last profiled float chunk: bit 0 sampled stage plan, bit 1 threshold-only
                                 (lane-max) sample stage, bit 2 certified int8 coarse pass, bit 3 segmented emission,
                                 bit 4 <= 32-query kernel, bit 5 fused single-launch search (k_small_search), bit 6 the search STARTED
                                 on the certified int8 pass (bit 2 tells what the LAST run used: an overflow retries on the f16
                                 pass), bit 7 the sample stage ran INSIDE the launch of the first threshold stage (one scan launch less than
                                 stages), bits 8..15 number of scan stages, bits 16..23 wave tiling
                                 (0x24 = <2,4,4,2>, 0x42 = <4,2,2,4>, 0x14 = <1,4,1,1>, 0x81 = the query-stationary k_scan_qs), bit 24 the self-tightening
                                 single-launch scan, bit 25 the sample stage ran on the query-stationary tiling, bit 26 the stages read the
                                 non-negative 7-bit copy of the codes (SQ7: FLAT-IP, 129..256 queries, LYNSE_HIP_SQ7), bit 27 the query-stationary
                                 threshold stages ran on v_mfma_i32_16x16x64_i8 (same tile, four segments per workgroup and query;
                                 LYNSE_HIP_QS_M16=0: the 32x32x32 form; results never change), bit 28 the PREDICTED plan: one threshold
                                 stage over all rows on a threshold predicted from the column statistics of the codes and verified
                                 afterwards (FLAT-IP / cosine, 129..256 queries, k <= 32, LYNSE_HIP_PREDICT; with it bits 0 / 1 read 0 and the
                                 stage count reads 1; a chunk it missed on is answered again on the sampled plan, which then is the last
                                 plan) — lets a test pin the kernel instantiation a benchmark configuration runs */
    uint64_t predicted_queries;    /* queries of chunks that ran the predicted plan */
    uint64_t predict_miss_queries; /* of those, queries whose predicted threshold failed its verification (their chunks were re-answered) */
} lynse_hip_profile;

/* ---- library ---- */
int lynse_hip_abi_version(void);
/* Copies the calling thread's last error message (NUL-terminated) and returns its length. */
size_t lynse_hip_last_error(char *buf, size_t cap);
int lynse_hip_device_count(int *out_count);
/* DistanceMetric::from_str (distance/mod.rs:39-63) / from_index_mode (:67-107). */
int lynse_hip_metric_from_str(const char *name, int *out_metric);
int lynse_hip_metric_from_index_mode(const char *mode, int *out_metric);
int lynse_hip_metric_is_ascending(int metric); /* distance/mod.rs:111-116 */
int lynse_hip_metric_is_binary(int metric);    /* distance/mod.rs:161-166 */

/* ---- FLAT shard: FlatMmap (src/storage/flat_mmap.rs:89-109, :187-221) ---- */

/* FlatMmap::open(path, dim, F32) -> an empty row-major f32 store on `device`. */
int lynse_hip_flat_create(uint32_t dim, int device, lynse_hip_flat **out);
int lynse_hip_flat_destroy(lynse_hip_flat *h);
int lynse_hip_flat_reserve(lynse_hip_flat *h, uint64_t rows);
/* FlatMmap::write / append (flat_mmap.rs:223-330): rows are n*dim little-endian f32, row-major —
 * exactly a reference segment file's bytes. */
int lynse_hip_flat_append_f32(lynse_hip_flat *h, const float *rows, uint64_t n);
int lynse_hip_flat_append_f32_device(lynse_hip_flat *h, const float *d_rows, uint64_t n);
/* Pre-packed one-bit rows, ceil(dim/64) u64 words per row, bit i of word i/64 LSB-first — the
 * BinaryData layout (flat_mmap.rs:145-160, simd.rs:750-757).  A store holds f32 rows or packed
 * rows, not both appended. */
int lynse_hip_flat_append_packed_u64(lynse_hip_flat *h, const uint64_t *words, uint64_t n);
int lynse_hip_flat_append_packed_u64_device(lynse_hip_flat *h, const uint64_t *d_words, uint64_t n);
/* Row statistics for newly appended rows (norms, scale).  Idempotent. */
/* VectorDtype::F16 storage (FlatMmap with dtype F16, flat_mmap.rs:187-221, search :905-908): appended f32 rows are
 * rounded through f16 (RNE) like `encode_f32_slice_as_le_bytes`, `append_f16_bits` takes the file's u16 words as they
 * are, and every distance follows the reference's f16 kernels (sequential f32 sums, simd.rs:805-846).  Must be called
 * on an empty shard.  ip / l2 / cosine (+ the packed-binary metrics, which only see value > 0.5). */
int lynse_hip_flat_set_dtype(lynse_hip_flat *h, int dtype);
int lynse_hip_flat_append_f16_bits(lynse_hip_flat *h, const uint16_t *rows, uint64_t n);
int lynse_hip_flat_finalize(lynse_hip_flat *h);
/* Returned row = local_row * stride + offset (multi-GPU shards; default 1, 0). */
int lynse_hip_flat_set_row_map(lynse_hip_flat *h, uint64_t stride, uint64_t offset);
int lynse_hip_flat_set_ip_form(lynse_hip_flat *h, int ip_form);
uint64_t lynse_hip_flat_len(const lynse_hip_flat *h); /* FlatMmap::len */
uint32_t lynse_hip_flat_dim(const lynse_hip_flat *h); /* FlatMmap::dim */
int lynse_hip_flat_device(const lynse_hip_flat *h);
/* Copy rows [first, first+n) back to host f32 (FlatMmap::as_slice). */
int lynse_hip_flat_read_rows(const lynse_hip_flat *h, uint64_t first, uint64_t n, float *out);
/* Same, into a device buffer of this handle's GPU (n*dim f32, dense). */
int lynse_hip_flat_copy_rows_device(const lynse_hip_flat *h, uint64_t first, uint64_t n, float *d_out);
/* ensure_binary (flat_mmap.rs:388-401) contents: packed words of rows [first, first+n). */
int lynse_hip_flat_read_packed(lynse_hip_flat *h, uint64_t first, uint64_t n, uint64_t *out_words);

/* ROW MUTATION (Collection::upsert_items / update_items, src/engine.rs:5880-6103; compact, :6494-6596; read_vectors_by_ids_only,
 * :6353-6401): rows of a float shard rewritten in place, dropped in place, and read by index.  The rules:
 *  1. lynse_hip_flat_update_rows_f32: data is n x dim dense f32, rows are shard rows, each < len and pairwise distinct — both checked on
 *     the host before anything is written (LYNSE_ERR_INVALID_ARGUMENT, the shard unchanged).  An f32 shard gets the row at its pitch
 *     with zero pad columns; an F16 shard gets the f16 bits lynse_hip_flat_append_f32 would store (one conversion, RNE).  Host data
 *     goes through a staging buffer of at most 64 MiB per step.  Distinct rows: no two items write one address, no atomics.
 *  2. lynse_hip_flat_compact_rows: keep_words is a BitSet in the convention of lynse_hip_flat_search_filtered_bitset_f32, a set bit =
 *     the row stays; n_words < ceil(len / 64) is LYNSE_ERR_INVALID_ARGUMENT, bits at or beyond len are ignored.  New row j is the j-th
 *     kept old row (stable; the reference's id_map, :6509-6514).  In place: the call allocates the keep words, 4 bytes per 64 rows
 *     and a scratch of at most one window of rows, never a second shard; the capacity is kept.  *out_len (may be NULL) = the new len.
 *     window_rows must be a multiple of 64; 0 = the default, 64 MiB over the row's bytes rounded down to a multiple of 64, at least 64.
 *     When every row stays the call changes nothing at all (rule 4 does not apply).
 *  3. The plan (lynse_hip_compact_plan, host only, no device; the compaction runs this very function): live = the kept rows below n;
 *     word_base[w] = the kept rows below 64 w (the destination of the first kept row of word w); window j covers source rows
 *     [j W, min((j + 1) W, n)) and is {src = j W, dst = word_base[j W / 64], live, path}, four u64 each: path 0 = untouched (dst == src
 *     and every row kept: the prefix before the first cleared bit), 1 = direct iff dst + live <= src (destinations and sources of the
 *     window are disjoint, rows are written straight to their place), 2 = staged (the live rows go densely to the scratch, then one
 *     device copy puts them at dst; stream order makes it safe: it writes only rows below (j + 1) W, all read by then).
 *     row_bytes only sizes the default window.  out_word_base (ceil(n / 64)) and out_windows (4 x ceil(n / W)) may be NULL.
 *  4. After an update of n > 0 rows or a compaction that dropped a row, everything derived from the rows is what a fresh handle
 *     holding the final rows would build: norms, statistics and flags are recomputed over ALL rows, the f16 shadow, the packed words
 *     and their copy and the four int8 code sets are rebuilt (the code sets from a NEW fit), overflow strikes start at 0 — all lazily,
 *     by the next search that needs them.  PQ, RaBitQ, PolarVec, HNSW and DiskANN indexes of the handle are dropped.
 *  5. lynse_hip_flat_gather_rows: out[i] = row rows[i] as f32 (an F16 shard decoded exactly), any order, repeats allowed; a row >= len is
 *     LYNSE_ERR_INVALID_ARGUMENT.  Lock discipline of lynse_hip_flat_read_rows.
 *  Update and compact are writers: refused while tickets are outstanding ("in flight").  LYNSE_ERR_UNSUPPORTED: a packed-only handle
 *  (both), a row-mapped handle (compaction renumbers rows).  There are no sharded, _device or ticket forms. */
int lynse_hip_flat_update_rows_f32(lynse_hip_flat *h, const uint64_t *rows, const float *data, uint64_t n);
int lynse_hip_flat_compact_rows(lynse_hip_flat *h, const uint64_t *keep_words, uint64_t n_words, uint32_t window_rows,
                                uint64_t *out_len);
int lynse_hip_flat_gather_rows(const lynse_hip_flat *h, const uint64_t *rows, uint64_t n, float *out);
int lynse_hip_compact_plan(const uint64_t *keep_words, uint64_t n_words, uint64_t n, uint32_t window_rows, uint64_t row_bytes,
                           uint64_t *out_live, uint32_t *out_window_rows, uint64_t *out_n_windows, uint32_t *out_word_base,
                           uint64_t *out_windows);

/* FlatMmap::search (flat_mmap.rs:824-923) for a batch of queries (Collection::batch_search,
 * engine.rs:5352-5498).  queries: nq*dim f32.  Binary metrics threshold the f32 query at 0.5
 * (pack_binary_query, flat_mmap.rs:1292-1296).  out_rows/out_dists: nq*k; out_counts: nq. */
int lynse_hip_flat_search_f32(lynse_hip_flat *h, const float *queries, uint64_t nq, uint32_t k,
                              int metric, uint64_t *out_rows, float *out_dists,
                              uint32_t *out_counts);
/* FlatMmap::search_filtered (src/storage/flat_mmap.rs:491-815; VectorStore::search_filtered
 * vector_store.rs:1006-1040; Collection brute_force_search_filtered engine.rs:5541-5566): top-k among the rows
 * listed in `subset_rows` (local row indices of this shard, host memory; ids >= len are skipped like the
 * reference skips them, duplicates count once).  k is clamped to min(k, n_subset, len) (:501).  One subset serves
 * the whole batch.  Binary metrics pack the f32 queries (pack_binary_query).  The subset becomes a row bitmask on
 * the device — the reference's own bitset strategy (:672-679) — applied in the scan epilogue; distances use the
 * single-row kernels as the reference does on this path (:553-560), results are in canonical (distance, row)
 * order. */
int lynse_hip_flat_search_filtered_f32(lynse_hip_flat *h, const float *queries, uint64_t nq, uint32_t k,
                                       int metric, const uint64_t *subset_rows, uint64_t n_subset,
                                       uint64_t *out_rows, float *out_dists, uint32_t *out_counts);
/* Same with the subset as the reference's BitSet words (src/storage/bitset.rs:15-24: bit r of word r/64, LSB first;
 * SearchParams.subset, engine.rs:5541-5566).  Bits at or beyond len are ignored. */
int lynse_hip_flat_search_filtered_bitset_f32(lynse_hip_flat *h, const float *queries, uint64_t nq,
                                              uint32_t k, int metric, const uint64_t *bitset_words,
                                              uint64_t n_words, uint64_t *out_rows, float *out_dists,
                                              uint32_t *out_counts);
/* The same search with the BitSet words ALREADY IN THIS DEVICE'S MEMORY (d_bitset_words; what lynse_hip_fields_filter leaves behind,
 * lynse_hip_fields_words_device) and the number of set bits below len supplied by the caller (`count`: the filter's match count, one
 * 8-byte read-back).  The words reach the scan by a device copy instead of an upload; `count` feeds k.min(subset.len()) and the
 * gathered / masked strategy choice exactly as the count of the host words does.  Results equal lynse_hip_flat_search_filtered_bitset_f32
 * on the same words bit for bit.  `count` is a PRECONDITION like a buffer length: it sizes the id list the gathered strategy expands the
 * words into, so it must be the number of set bits below len exactly (lynse_hip_fields_filter's *out_count over the same n is).  The
 * words must hold n_words u64 and stay valid and unchanged until the call returns; rows they do not cover are out, as in the host
 * form.  count > len is LYNSE_ERR_INVALID_ARGUMENT.  The additive metrics (ids 7-10) and k beyond a quarter of the candidate capacity keep their
 * host-side subset plumbing: there the words are read back first. */
int lynse_hip_flat_search_filtered_bitset_device_f32(lynse_hip_flat *h, const float *queries, uint64_t nq,
                                                     uint32_t k, int metric, const uint64_t *d_bitset_words,
                                                     uint64_t n_words, uint64_t count, uint64_t *out_rows,
                                                     float *out_dists, uint32_t *out_counts);
/* FLAT-*-SQ8 (`use_sq8`, src/storage/flat_mmap.rs:891-905, sq8_two_pass_search :5868-5926): pass 1 ranks ALL rows by the
 * integer score of their per-dimension u8 codes (u32 dot for ip, u32 squared L2 for l2 and cosine; SQ8Data :5676-5750,
 * built lazily like ensure_sq8 and rebuilt after appends) and keeps n_cand = max(20 k, 200) rows (cosine max(100 k, 500));
 * pass 2 rescores those exactly with the single-row f32 kernels and returns the best k.  Approximate by design: a true
 * neighbour outside the n_cand best codes is lost, exactly as in the reference.  Ties at the n_cand cut and between equal
 * exact distances are broken by row id (the reference leaves them to heap / unstable-sort order).  Other metrics take the
 * ordinary exact path, as `use_sq8` does.  Non-finite values: the fit ignores a NaN element (its code is 0) and a dimension
 * holding +-inf gets scale 0 (every code 0), so pass 1 stays an integer ranking; pass 2 follows the NON-FINITE VALUES rule of the
 * FLAT searches above (a NaN distance is the worst value of the metric, ties by ascending row). */
int lynse_hip_flat_search_sq8_f32(lynse_hip_flat *h, const float *queries, uint64_t nq, uint32_t k,
                                  int metric, uint64_t *out_rows, float *out_dists,
                                  uint32_t *out_counts);
/* The SQ8 quantiser state (per-dimension minimum and scale = 255 / range, 0 for a constant dimension). */
int lynse_hip_flat_sq8_params(lynse_hip_flat *h, float *mins, float *scales);
/* FLAT-{IP,L2,COS,COSINE}-PQ and FLAT-*-PQ<n> (PQIndex, src/storage/pq_mmap.rs; Collection, engine.rs:4559-4600, :5504-5526).
 * f32 handles and ip / l2 / cosine only.  The rules:
 *  1. M = the n of "PQ<n>" when n > 0 divides dim, else the first divisor of dim in [16, 8, 32, 4, 12, 24, 6, 2, 1]
 *     (parse_n_subspaces, pq_mmap.rs:1107-1128; Python: parse_n_subspaces); ss = dim / M; K = min(clamp(n_clusters, 1, 256), n).
 *  2. Training sample: train_n = min(n, 50,000) rows; when train_n < n, rows 0, s, 2s, ... with s = max(n / train_n, 1).
 *  3. Per subspace m, k-means (kmeans_subspace, :577-662): 6 iterations when K <= 64, else 15.  Assignment: l2_squared_f32
 *     against every centroid in order, the first strictly smaller than the best so far (from f32::MAX) wins, so NaN never wins.
 *     Assignments start at 0; a pass that moves none stops that subspace BEFORE the update (K = 1 keeps the initial
 *     centroids).  Update: per-cluster f32 sums in ascending row order, then *= fl(1 / count).  An empty cluster becomes
 *     new[src] * (1 + 0.01 ((d % 2) - 0.5)), src = the LAST most-populated cluster; new[src] is already divided when src < c
 *     and still the raw sum when src > c.
 *  4. Initialisation (random_init_centroids, :665-689): SmallRng::seed_from_u64(m) = xoshiro256++ seeded by SplitMix64;
 *     gen_range(0..train_n) by widening multiply with rejection zone (n << lzcnt(n)) - 1; distinct indices, at most 10 K
 *     attempts; centroids still missing become prev[d] * (1 + 0.001 d).  lynse_hip_pq_xoshiro_stream / _splitmix_stream /
 *     _init_indices expose this host code for known-answer tests.
 *  5. Encode: argmin of l2_squared_f32 over the K codewords, first strictly smaller wins (a NaN sub-vector gets code 0).
 *  6. Tables: lut[m][c] = inner_product_f32 (IP) or l2_squared_f32 (L2 AND cosine) of the RAW query's sub-vector m and codeword
 *     c; the ADC score is 0.0f + lut[0][c0] + lut[1][c1] + ..., added in f32 in ascending m.
 *  7. Search: k' = min(k, n_pq), N = min(k' * oversample, n_pq) (the Collection passes 32, PQ_OVERSAMPLE); the N best ADC
 *     scores (largest for IP, smallest otherwise), rescored with compute_distance_f32 on the original rows; the best k' come
 *     back with their exact distances.  Both cuts use the canonical (score, row) key (the reference's heap + sort_unstable
 *     leave ties unpinned); NaN and +-inf order as in the FLAT searches.  Output layout of lynse_hip_flat_search_f32.
 *  8. The index covers the first n_pq rows: rows appended after a build or a load stay outside it (n_pq is unchanged).  Build and
 *     load replace an earlier PQ index; lynse_hip_flat_drop_pq removes it.  The exact searches of the handle are unchanged.
 *  Refused with LYNSE_ERR_UNSUPPORTED: an F16 shard, a packed-only handle, a row-sharded handle (set_row_map with stride != 1
 *  or offset != 0: there is no sharded PQ search), and the binary metrics.  There is no ticket (submit / wait) or upsert form.
 *  The PQ search holds the handle's lock exclusively (its scratch is per handle) and runs on context 0.
 * lynse_hip_flat_load_pq applies PQIndex::load's checks (M == 0, K outside 1..=256, M * ss != dim, n > u32::MAX: "Invalid PQ index
 * dimensions"; a code >= K: "PQ index contains an out-of-range code") and needs n <= the handle's rows.  lynse_hip_flat_pq_params
 * returns mks = {M, K, ss} and n_pq (all 0 without an index) and, when the pointers are not NULL, codebooks[M][K][ss] and
 * codes[n_pq][M].  lynse_hip_flat_pq_stage_times, with profiling on: out3[0] searches, out3[1] the scan stage (tables, ADC scan and
 * the pool cut) and out3[2] the rescore (plus the host selection of a pool beyond 16,384), microseconds from HIP events; reset != 0
 * clears them. */
int lynse_hip_flat_build_pq(lynse_hip_flat *h, uint32_t n_subspaces, uint32_t n_clusters);
int lynse_hip_flat_load_pq(lynse_hip_flat *h, uint32_t n_subspaces, uint32_t n_clusters, const float *codebooks,
                           const uint8_t *codes, uint64_t n);
int lynse_hip_flat_pq_params(lynse_hip_flat *h, uint32_t *mks, uint64_t *n_pq, float *codebooks, uint8_t *codes);
int lynse_hip_flat_drop_pq(lynse_hip_flat *h);
int lynse_hip_flat_search_pq_f32(lynse_hip_flat *h, const float *queries, uint64_t nq, uint32_t k, int metric,
                                 uint32_t oversample, uint64_t *out_rows, float *out_dists, uint32_t *out_counts);
int lynse_hip_flat_pq_stage_times(lynse_hip_flat *h, double *out3, int reset);
int lynse_hip_pq_xoshiro_stream(const uint64_t *state4, uint64_t count, uint64_t *out);
int lynse_hip_pq_splitmix_stream(uint64_t seed, uint64_t count, uint64_t *out);
int lynse_hip_pq_init_indices(uint64_t seed, uint64_t n, uint32_t k, uint32_t *idx, uint32_t *chosen);
/* FLAT-{IP,L2,COS,COSINE}-RABITQ (RaBitQIndex, src/storage/rabitq_mmap.rs; Collection, engine.rs:4476, :4552, :5504-5526): 1-bit
 * codes of a randomised Hadamard rotation, scanned whole, and an exact rescore.  f32 handles and ip / l2 / cosine only; no
 * training.  The rules:
 *  1. padded_dim = next_power_of_two(dim), code_bytes = ceil(padded_dim / 8), ceil(padded_dim / 64) sign words.  Sign word w is
 *     the w-th next_u64() of SmallRng::seed_from_u64(42) (xoshiro256++ seeded by SplitMix64; lynse_hip_rabitq_sign_words exposes
 *     this host code for known-answer tests).  Bit i % 64 of word i / 64 set = "negate element i".
 *  2. Encode a row (:101-132): norm = sqrt(sum x * x), summed in f32 in ascending index order from 0, correctly rounded sqrt.
 *     The row is zero-padded to padded_dim, the signs applied, then the in-place unnormalised FWHT (:359-377): stages
 *     h = 1, 2, 4, ...; each butterfly (x + y, x - y) with x the lower index.  Bit d % 8 of byte d / 8 is buf[d] >= 0.0
 *     (-0.0 sets it, NaN does not); bits at d >= padded_dim stay 0.
 *  3. Query (:202-213): the same pad, signs and FWHT; total_q = the f32 sum of all padded_dim rotated values in ascending order;
 *     lut[b][v] = the f32 sum, from 0.0f, of q_rot[8 b + bit] over the set bits of v in ascending bit order.
 *  4. Score (compute_binary_score, :560-585), no FMA contraction anywhere: sum_set = 0.0f + lut[0][c0] + lut[1][c1] + ... in
 *     ascending byte order; ip_raw = 2 sum_set - total_q; IP maximises ip_raw * norm; L2 and cosine minimise
 *     norm * norm - ((2 ip_raw) * norm) / (float)padded_dim.
 *  5. Search: k' = min(k, n_rbq), N = min(k' * oversample, n_rbq) (the Collection passes 200, DEFAULT_OVERSAMPLE); the N best
 *     scores form the pool, rescored with compute_distance_f32 on the original rows; the best k' come back with their exact
 *     distances.  Both cuts use the canonical (score, row) key (the reference's per-thread heaps and sort_unstable leave ties
 *     unpinned, as for PQ); NaN and +-inf order as in the FLAT searches, -0 == +0.  Output layout of lynse_hip_flat_search_f32.
 *  6. The index covers the first n_rbq rows: rows appended after a build or a load stay outside it (n_rbq is unchanged).  Build
 *     and load replace an earlier RaBitQ index; lynse_hip_flat_drop_rabitq removes it.  The exact searches are unchanged.
 *  Refused with LYNSE_ERR_UNSUPPORTED: padded_dim * 4 bytes beyond the 160 KiB of LDS, an F16 shard, a packed-only handle, a
 *  row-sharded handle and the binary metrics.  There is no ticket (submit / wait) or upsert form.  The search holds the handle's
 *  lock exclusively (its scratch is per handle) and runs on context 0.
 * lynse_hip_flat_load_rabitq takes what rabitq_index.bin holds: dim (must be the handle's: "Invalid RaBitQ dimensions"), the
 * sign words (a word the file lacks negates nothing, as apply_signs has it), codes[n][code_bytes] and norms[n]; n <= the handle's
 * rows.  lynse_hip_flat_rabitq_params returns dims = {dim, padded_dim, code_bytes} and n_rbq (all 0 without an index) and, for
 * the pointers that are not NULL, the ceil(padded_dim / 64) sign words, codes[n_rbq][code_bytes] and norms[n_rbq] (the device
 * keeps the codes in a tiled layout of its own; this is the file's).  lynse_hip_flat_rabitq_stage_times, with profiling on:
 * out3[0] searches, out3[1] the scan stage (query transform, scan and the pool cut) and out3[2] the rescore (plus the host
 * selection of a pool beyond 16,384), microseconds from HIP events; reset != 0 clears them. */
int lynse_hip_flat_build_rabitq(lynse_hip_flat *h);
int lynse_hip_flat_load_rabitq(lynse_hip_flat *h, uint32_t dim, const uint64_t *sign_words, uint32_t n_sign_words,
                               const uint8_t *codes, const float *norms, uint64_t n);
int lynse_hip_flat_rabitq_params(lynse_hip_flat *h, uint32_t *dims, uint64_t *n_rbq, uint64_t *sign_words, uint8_t *codes,
                                 float *norms);
int lynse_hip_flat_drop_rabitq(lynse_hip_flat *h);
int lynse_hip_flat_search_rabitq_f32(lynse_hip_flat *h, const float *queries, uint64_t nq, uint32_t k, int metric,
                                     uint32_t oversample, uint64_t *out_rows, float *out_dists, uint32_t *out_counts);
int lynse_hip_flat_rabitq_stage_times(lynse_hip_flat *h, double *out3, int reset);
int lynse_hip_rabitq_sign_words(uint64_t seed, uint64_t count, uint64_t *out);
/* FLAT-{IP,L2,COS,COSINE}-POLARVEC<b> (PolarVecIndex, src/storage/polarvec_mmap.rs; Collection, engine.rs:4593-4602, :5514-5515):
 * b-bit codes (b = 1..8) of the randomised Hadamard rotation on a per-dimension grid, scanned whole through per-dimension tables of
 * the query, and an exact rescore.  f32 handles and ip / l2 / cosine only; no training.  Every sum is a chain of separate f32
 * operations in the order given, no FMA contraction anywhere.  The rules:
 *  1. padded_dim P = next_power_of_two(dim), levels = 1 << bits, bytes_per_vec = ceil(P * bits / 8); the sign words and the rotation
 *     (zero-pad, signs, unnormalised FWHT) are RaBitQ's, rules 1 and 2 above.
 *  2. Fit (:137-208): sample rows si * stride for si < min(n, 50000), stride = 1 for n <= 50000, else n / 50000 (integer).  Per
 *     rotated dimension min and max over the samples by strict < / > from +inf / -inf: a NaN is never taken, and of values that
 *     compare equal (+0, -0) the earliest sample row's stays.  range = max - min; if range > 1e-8f: dim_min = min - 0.05f * range,
 *     dim_scale = (range * (1.0f + 2.0f * 0.05f)) / (float)(levels - 1); else dim_min = min, dim_scale = 1.0f.
 *  3. Encode (:703-777): per d ascending over all P rotated values, code = (u8)min(max(roundf((val - dim_min) / dim_scale), 0),
 *     levels - 1) (half away from zero; a NaN codes as 0), v_hat = dim_min + (float)code * dim_scale, residual_sq = sum (val - v_hat)^2,
 *     v_hat_sq = sum v_hat^2, inv_v_hat_norm = 1.0f / fmaxf(sqrtf(v_hat_sq), 1e-12f).  residual_sq is kept only by an index built for
 *     L2, inv_v_hat_norms only by one built for cosine.  The code stream is LSB-first: dimension d at bits [d * bits, (d + 1) * bits).
 *  4. Query (:310-332, :926-972): for cosine the query is first divided by fmaxf(sqrtf(sum x^2), 1e-12f); rotate; lut[d][c] from
 *     v = dim_min + (float)c * dim_scale: IP q * v, L2 (q - v)^2, cosine -(q * v).
 *  5. Row score (:1010-1135): bits 4: byte b contributes lut[2b][low nibble] + lut[2b+1][high nibble] (the second only if 2b + 1 < P)
 *     to s[b % 4] over the first (bytes / 4) * 4 bytes, leftover bytes to s0, score ((s0 + s1) + s2) + s3; bits 8: the same over
 *     lut[b][code_b]; bits 3: groups of 8 dimensions, dimension j of a group to s[j % 4], P / 8 groups (none below P = 8: the sum
 *     is 0.0f); bits 1, 2, 5, 6, 7: one chain over d.  Then + residual_sq[row] when searching L2 and the array exists, *
 *     inv_v_hat_norms[row] when searching cosine and it exists: a search with another metric than the build's finds it absent.
 *  6. Search: k' = min(k, n_plv), N = min(k' * oversample, n_plv) (the Collection passes 20, DEFAULT_OVERSAMPLE); pool, rescore,
 *     cuts, ordering and output as RaBitQ's rule 5; coverage, replacement and drop as its rule 6.
 *  Refused: what RaBitQ refuses, and bits outside 1..8 ("bits must be in [1, 8]").  The search holds the handle's lock exclusively.
 * lynse_hip_flat_load_polarvec takes what a version-5 polarvec_index.bin holds: dim (must be the handle's: "Invalid PolarVec index
 * dimensions"), bits, the sign words, dim_mins[P], dim_scales[P], codes[n][bytes_per_vec] and the two optional arrays [n] (NULL =
 * absent); n <= the handle's rows.  lynse_hip_flat_polarvec_params returns dims = {dim, padded_dim, bits, bytes_per_vec, flags} (flags:
 * 1 = residual_sq, 2 = inv_v_hat_norms) and n_plv (all 0 without an index) and, for the pointers that are not NULL, the arrays in the
 * file's layout (an absent optional array is left untouched).  lynse_hip_flat_polarvec_stage_times: as lynse_hip_flat_rabitq_stage_times. */
int lynse_hip_flat_build_polarvec(lynse_hip_flat *h, uint32_t bits, int metric);
int lynse_hip_flat_load_polarvec(lynse_hip_flat *h, uint32_t dim, uint32_t bits, const uint64_t *sign_words, uint32_t n_sign_words,
                                 const float *dim_mins, const float *dim_scales, const uint8_t *codes, const float *residual_sq,
                                 const float *inv_v_hat_norms, uint64_t n);
int lynse_hip_flat_polarvec_params(lynse_hip_flat *h, uint32_t *dims, uint64_t *n_plv, uint64_t *sign_words, float *dim_mins,
                                   float *dim_scales, uint8_t *codes, float *residual_sq, float *inv_v_hat_norms);
int lynse_hip_flat_drop_polarvec(lynse_hip_flat *h);
int lynse_hip_flat_search_polarvec_f32(lynse_hip_flat *h, const float *queries, uint64_t nq, uint32_t k, int metric,
                                       uint32_t oversample, uint64_t *out_rows, float *out_dists, uint32_t *out_counts);
int lynse_hip_flat_polarvec_stage_times(lynse_hip_flat *h, double *out3, int reset);
/* HNSW-{IP,L2,COS,COSINE} (HNSWIndex, src/index/hnsw.rs; Collection, engine.rs:4606-4655, :4743-4745): a layered neighbour graph over
 * the rows of a FLAT handle — the graph holds ids, the rows stay the handle's — a deterministic bulk build from exact neighbour lists,
 * and the reference's beam search.  f32 handles and ip / l2 / cosine only.  The reference's search is a function of the graph, the
 * levels, the entry point and the query (ties aside) and is restated here; its build (SmallRng::from_entropy, concurrent inserts,
 * hnsw.rs:952-1031) differs from run to run and is no parity target: rules 1-4 define this library's own.  The rules:
 *  0. The graph distance d(a, b) is compute_distance_f32 in the single-row form of the metric (for ip the two-accumulator kernel,
 *     whatever lynse_hip_flat_set_ip_form says), negated for ip (hnsw.rs:536-543).  A NaN distance becomes +inf the moment it is
 *     computed, in the build and in the search.  The three forms are symmetric bit for bit, so d(i, j) stands for d(j, i).
 *     Parameters: m in 2..32 (1 / ln(1) is infinite; m0 = 2 m <= 64), ef_construction and ef_search in 1..4096, max_level (< 0 = no
 *     cap), seed.  The reference's defaults: m 16, ef_construction 128, ef_search 50 (src/index/mod.rs:503, :681-686); the Collection
 *     passes seed 42.
 *  1. Levels, in integers only: w_i = the i-th next_u64() of SmallRng::seed_from_u64(seed) (the stream of lynse_hip_rabitq_sign_words);
 *     t = max(w_i >> 11, 1), level = 0; while level < max_level (when capped) and t * m < 2^53: t *= m, ++level.  P(level >= l) = m^-l,
 *     the distribution of floor(-ln U / ln m), without libm.  The entry point is the first row of the highest level (hnsw.rs:967-975).
 *     lynse_hip_hnsw_levels exposes this host code for known-answer tests.
 *  2. Candidates at level l: S_l = {i : level_i >= l}; cand_l(i) = the best ef_construction of S_l \ {i} by (d, row ascending): the
 *     exact FLAT search of the handle (over the BitSet of S_l above level 0) asked for ef_construction + 1 rows, i removed — the last
 *     entry dropped instead when i did not come back.
 *  3. Forward lists: F_l(i) = select_neighbors_heuristic(cand_l(i), cap) (hnsw.rs:550-602), cap = 2 m at level 0 and m above: all
 *     candidates when there are no more than cap; else walk them nearest first, keep c unless some already kept s has
 *     d(c, s) < d(i, c), stop at cap, then fill the free slots with the nearest candidates not kept.
 *  4. Adjacency: U(i) = F(i) and every j with i in F(j), each member once, ordered by (d(i, .), node).  No more than cap: that list.
 *     Else the heuristic's output on it, in selection order.  Stored order matters: the search admits neighbours in stored order.
 *  5. Search (hnsw.rs:1040-1140, unfiltered): ef = max(ef_query > 0 ? ef_query : ef_search, k).  Greedy descent on levels top .. 1
 *     (:758-777): a pass scans the list of the node it started from and moves to every neighbour strictly closer than the best so far;
 *     passes repeat until one moves nothing.  Beam at level 0 (:625-699): C a min-heap of candidates, R a max-heap of at most ef
 *     results, both start with the node the descent ended on; pop the closest c of C; stop when c.dist > worst.dist and R is full; for
 *     each unvisited neighbour in stored order: mark it visited, compute d, admit it to C and R iff R is not full or d < worst.dist
 *     (strict, on the distance alone), then evict R's maximum when |R| > ef.  The reference orders its heaps by distance alone, which
 *     leaves ties to BinaryHeap internals; here every pop, eviction and the final sort use the total order (dist, node), so results
 *     equal the reference's whenever no two visited nodes tie.  Output: the best min(k, |R|) of R by (dist, node), ip distances
 *     un-negated, in the layout of lynse_hip_flat_search_f32 (row ~0 and the worst distance after out_counts[q] entries).
 *  6. The graph covers the first n_hnsw rows: rows appended after a build or a load stay outside it until
 *     lynse_hip_flat_hnsw_extend takes them in (rule 7).  Build and load replace an earlier graph; lynse_hip_flat_drop_hnsw removes
 *     it.  The exact searches of the handle are unchanged.
 *  7. Incremental insert: lynse_hip_flat_hnsw_extend(h, mode) leaves a graph over all rows of the handle whose
 *     lynse_hip_flat_hnsw_params output (info, n_hnsw, levels, adj0, upper_node, upper_level, upper_adj, stored order included) equals
 *     what lynse_hip_flat_build_hnsw gives over the same rows with the metric, m, ef_construction, ef_search, max_level and seed of the
 *     build the graph came from: rules 1-4 make the graph a function of the rows and those, and level i is the i-th draw of one
 *     stream.  A build keeps, in host memory, those parameters, every level's forward lists with their graph distances (8 bytes per
 *     slot) and one threshold per (node, level): the raw score of the last of the ef_construction + 1 entries its exact search
 *     returned, "short" when it returned fewer or that score is NaN.  For new rows N and a level l with N_l = N in S_l not empty: an
 *     old member i is searched again when its threshold is short or some x in N_l scores against it not strictly worse than the
 *     threshold (ties and NaN count; the score is the single-row form the search ranks by; x has a higher row number than every old
 *     row, so it enters a list only by a strictly better score) — a superset of the members whose candidates change.  They and N_l go
 *     through rules 2-3 over the new S_l; rule 4 is recomputed for the lists whose forward list changed or that are in
 *     F_old(i) xor F_new(i) of such an i.  mode 0 = auto: the plain build when (n - n_hnsw) * ef_construction >= n_hnsw (the mean
 *     in-degree of the candidate digraph is ef_construction, so most old rows are searched again from there), the incremental path
 *     otherwise; mode 1 = always incremental; any other mode: LYNSE_ERR_INVALID_ARGUMENT.  The result is the same on either path.  No
 *     new rows: LYNSE_OK, nothing changes.  No graph: LYNSE_ERR_INVALID_ARGUMENT.  A graph installed by lynse_hip_flat_load_hnsw:
 *     LYNSE_ERR_UNSUPPORTED (no forward lists, no thresholds).  Every refusal of the build holds with its code and message.  A failed
 *     extend leaves the graph as it was, still searchable.  Lock and context as for the build, the ip form pinned to SINGLE.
 *     lynse_hip_flat_hnsw_extend_stats: out12 = {rows_before, rows_after, path (0 incremental, 1 plain build, 2 nothing to do),
 *     new_items (sum of |N_l|), researched (old members searched again), dirty_lists, reselected (lists through the heuristic again),
 *     scan_us (the reverse scan), cand_us, select_us, reverse_us, total_us} of the last extend.
 *  Refused with LYNSE_ERR_UNSUPPORTED: an F16 shard, a packed-only handle, a row-mapped handle, the binary and additive metrics, m or
 *  an ef outside its bounds, a build, load or search while tickets of lynse_hip_flat_search_submit_* are outstanding, a beam (24 bytes per ef, ef >= k)
 *  that does not share the 160 KiB of LDS with the query, and a build with ef_construction + 1 > 4096 over more than 16,384 rows (the
 *  exact search's candidate capacity).  A search metric other than the build metric: LYNSE_ERR_INVALID_ARGUMENT.  There is no ticket,
 *  _device, sharded or filtered form.  Build, load, drop and search hold the handle's lock exclusively and run on context 0.
 * lynse_hip_flat_load_hnsw takes levels[n], adj0[n][2 m], and the n_upper = sum of the levels upper lists upper_adj[n_upper][m] with
 * their upper_node[] / upper_level[] in ascending (node, level) order, lists padded with 0xFFFFFFFF, n <= the handle's rows.  It
 * answers LYNSE_ERR_INVALID_ARGUMENT unless every neighbour is < n, a neighbour of a level-l list has level >= l, the upper lists match
 * the levels and the entry has the top level.  Pad entries inside a list and a neighbour named twice are dropped (first place kept):
 * neither changes a search.  lynse_hip_flat_hnsw_params returns info = {metric, m, ef_search, entry, top_level, n_upper} and n_hnsw
 * (all 0 without an index) and, for the pointers that are not NULL, the same arrays.  lynse_hip_flat_hnsw_stage_times: out6[0..2] the
 * candidate-list, selection and reverse-edge microseconds of the last build (host clock around synchronised stages), then, with
 * profiling on, out6[3] searches, out6[4] their kernel microseconds (HIP events) and out6[5] the distances they scored; reset != 0
 * clears the last three. */
int lynse_hip_flat_build_hnsw(lynse_hip_flat *h, int metric, uint32_t m, uint32_t ef_construction, uint32_t ef_search,
                              int32_t max_level, uint64_t seed);
int lynse_hip_flat_load_hnsw(lynse_hip_flat *h, int metric, uint32_t m, uint32_t ef_search, const uint32_t *levels, uint64_t n,
                             const uint32_t *adj0, uint64_t n_upper, const uint32_t *upper_node, const uint32_t *upper_level,
                             const uint32_t *upper_adj, uint32_t entry);
int lynse_hip_flat_hnsw_params(lynse_hip_flat *h, uint32_t *info, uint64_t *n_hnsw, uint32_t *levels, uint32_t *adj0,
                               uint32_t *upper_node, uint32_t *upper_level, uint32_t *upper_adj);
int lynse_hip_flat_drop_hnsw(lynse_hip_flat *h);
int lynse_hip_flat_search_hnsw_f32(lynse_hip_flat *h, const float *queries, uint64_t nq, uint32_t k, int metric, uint32_t ef_query,
                                   uint64_t *out_rows, float *out_dists, uint32_t *out_counts);
int lynse_hip_flat_hnsw_stage_times(lynse_hip_flat *h, double *out6, int reset);
int lynse_hip_flat_hnsw_extend(lynse_hip_flat *h, int mode);
int lynse_hip_flat_hnsw_extend_stats(lynse_hip_flat *h, double *out12);
int lynse_hip_hnsw_levels(uint64_t seed, uint32_t m, int32_t max_level, uint64_t n, uint32_t *out);
/* DISKANN-{L2,COS,COSINE} (DiskANNIndex, src/index/diskann.rs, its in-memory full-precision form: search_graph over the rows
 * themselves): a flat neighbour graph of degree r over the rows of a FLAT handle, built by the reference's batched Vamana passes and
 * searched by its beam search.  f32 handles and l2 / cosine only.  The build is a function of the rows, the parameters and a random
 * stream, and is restated here list for list; the reference draws from StdRng, this library from its own stream (rule 1).  The rules:
 *  0. d(a, b) is the graph distance of the HNSW block (compute_distance_f32 in the single-row form, NaN -> +inf at once, symmetric bit
 *     for bit).  r in 1..64 (one lane per stored neighbour), l in 1..4096 and l := max(l, r), alpha a finite f32 >= 1,
 *     max_degree := max(max_degree, r), which makes the stored degree r (diskann.rs:236-237, :980).  The reference's defaults: r 16,
 *     l 64, alpha 1.2; the Collection passes seed 42.  No environment variable is read.
 *  1. Random stream: w_i = the i-th next_u64() of SmallRng::seed_from_u64(seed) (the stream of lynse_hip_rabitq_sign_words).
 *     draw(b) = ((w >> 32) * b) >> 32 for 1 <= b <= 2^32, one word.  shuffle(a): for i = len - 1 down to 1: j = draw(i + 1), swap a[i]
 *     and a[j].  n <= 1 consumes no word; otherwise, in this order: shuffle A of 0..n, shuffle B of 0..n, the initial graph, shuffle C.
 *  2. Entry point (choose_medoid, :767-795): refs = the first min(32, n) of A, cands = the first min(64, n) of B; for each candidate in
 *     order sum = 0.0f, sum += d(c, ref) over the refs in order (f32); the entry is the first candidate with sum < best_sum (from
 *     +inf), cands[0] when no sum is finite.
 *  3. Initial graph (:798-816): for i = 0 .. n - 1 draw j = draw(n) until min(r, n - 1) distinct j != i are chosen, stored as drawn.
 *  4. Order: C, then the entry swapped into position 0 with whatever is there (:1103-1107).
 *  5. Passes (:1084-1113, :1025-1076): one with alpha' = 1, a second with alpha' = alpha iff alpha > 1 + FLT_EPSILON.  A pass walks the
 *     order in batches of 256; for every p of a batch, against the graph as it stood when the batch began: the search of rule 8 with
 *     the row of p as the query, ef = L_b = max(min(l, 128), r) and 32 anchors; candidates = its results and (d(p, nb), nb) for nb in
 *     adj[p]; the forward list is prune(p, candidates, alpha').
 *  6. prune (robust_prune, :830-875, ascending branch): drop p, keep one entry per node (equal nodes carry equal bits), order by
 *     (d, node) — the reference's unstable sort leaves ties open, this order is the library's pin; until r are selected or none remain:
 *     select the first remaining b, keep a remaining v != b iff alpha' * d(b, v) > d(p, v) (one f32 multiply rounded once, then the
 *     comparison).  The output is in selection order.
 *  7. Commit (apply_vamana_updates, :979-1017), in batch order: install all forward lists; for each (src, list) in batch order and each
 *     dst != src in list order append src to adj[dst] unless it is there (after the installs: every src of a batch is another node) —
 *     the append slot is the number of earlier effective edges to the same dst, computed as such (a sort), never the arrival order of
 *     an atomic; every dst whose list is now longer than r (at most r + 256): adj[dst] = prune(dst, {(d(dst, x), x)}, alpha').  A list
 *     of at most r entries keeps its stored order, which the search follows.
 *  8. Search (search_graph, :880-973, unfiltered; search, :1258-1269, :1326): ef = min(max(ef_query, l, 10 k), n).  Starts
 *     (search_entry_points, :159-174): the entry, then a n / A for a = 0 .. A - 1, A = min(anchors, n), in u64, skipping a value equal
 *     to the entry; anchors = 8 for queries and 32 in the build.  Every start is marked visited, scored and pushed to C; R is the best
 *     ef of the starts by (d, node), no admission test.  Then the loop of HNSW rule 5 unchanged, every pop, eviction and the final
 *     sort by (dist, node).  Output: the best min(k, |R|), in the layout of lynse_hip_flat_search_f32.
 *  9. The graph covers the first n_diskann rows.  Build and load replace an earlier DiskANN graph; an HNSW graph on the handle is a
 *     separate state and is left alone.  The exact searches of the handle are unchanged.
 *  Refused with LYNSE_ERR_UNSUPPORTED: an F16 shard, a packed-only or row-mapped handle, any metric but l2 / cosine, r, l, alpha or an
 *  ef outside its bounds, outstanding tickets, a beam (24 bytes per ef) or a row that does not fit the 160 KiB of LDS.
 *  LYNSE_ERR_INVALID_ARGUMENT: a search metric other than the build metric; in load, a neighbour >= n or an entry >= n.
 * lynse_hip_flat_build_diskann: max_batches = 0 is the whole build; otherwise the build stops after that many batches, counted across
 * both passes, and the graph is installed as it stands (a test instrument: a build is some 2 n / 256 dependent steps).
 * lynse_hip_flat_load_diskann takes adj[n][r] padded with 0xFFFFFFFF; pads inside a list and a neighbour named twice are dropped.
 * lynse_hip_flat_diskann_params: info = {metric, r, l, entry}, alpha (0 for a loaded graph) and n_diskann, all 0 without an index, and
 * adj when it is not NULL.  lynse_hip_flat_diskann_stage_times: out8[0..2] the search / prune / commit microseconds of the last build
 * (host clock; measured only by a build that ran with profiling on, which waits after every stage — a plain build enqueues every
 * batch without a host round trip and reports 0), out8[3] its host random draws, out8[4] the whole build; with profiling on,
 * out8[5] searches, out8[6] their kernel microseconds (HIP events), out8[7] the distances they scored; reset != 0 clears the last three.
 * lynse_hip_vamana_draws (host only): the products of rules 1-4 that do not depend on the rows — refs[min(32, n)], cands[min(64, n)],
 * the order before the entry swap [n] and the initial graph adj0[n][r], padded — for known-answer tests. */
int lynse_hip_flat_build_diskann(lynse_hip_flat *h, int metric, uint32_t r, uint32_t l, float alpha, uint32_t max_degree,
                                 uint64_t seed, uint64_t max_batches);
int lynse_hip_flat_load_diskann(lynse_hip_flat *h, int metric, uint32_t r, uint32_t l, const uint32_t *adj, uint64_t n,
                                uint32_t entry);
int lynse_hip_flat_diskann_params(lynse_hip_flat *h, uint32_t *info, float *alpha, uint64_t *n_diskann, uint32_t *adj);
int lynse_hip_flat_drop_diskann(lynse_hip_flat *h);
int lynse_hip_flat_search_diskann_f32(lynse_hip_flat *h, const float *queries, uint64_t nq, uint32_t k, int metric,
                                      uint32_t ef_query, uint64_t *out_rows, float *out_dists, uint32_t *out_counts);
int lynse_hip_flat_diskann_stage_times(lynse_hip_flat *h, double *out8, int reset);
int lynse_hip_vamana_draws(uint64_t seed, uint64_t n, uint32_t r, uint32_t *refs, uint32_t *cands, uint32_t *order,
                           uint32_t *adj0);
/* Range search (Collection::search_range, src/engine.rs:6410-6483): every row of the handle is scored with the single-row kernel
 * (compute_distance_f32) and the rows on the passing side of the caller's threshold come back, best first, at most max_results of
 * them.  One threshold per query.  The rules:
 *  1. Distances: the single-row form of the metric at every n (for ip the two-accumulator kernel, never the batch-of-8 form, whatever
 *     lynse_hip_flat_set_ip_form says).  An F16 shard is scored on its exactly decoded rows with the f32 kernels (as_f32_cow), not
 *     with the f16 sequential sums.  The binary metrics take the packed popcount forms on the rows and the query thresholded at
 *     0.5 (pack_binary_query), so a packed-only handle works; ip / l2 / cosine on a packed-only handle are refused.
 *  2. The pass test: d <= threshold, for ip d >= threshold; plain IEEE comparisons.  A NaN distance never passes, a NaN threshold
 *     passes nothing, +-inf distances and thresholds are ordinary values.
 *  3. bitset_words (the reference's BitSet layout: bit r of word r / 64, LSB first; NULL = every row) restricts the scan to its
 *     rows before the cap; rows the words do not cover are out, bits at or beyond len are ignored.
 *  4. out_passed[q] (may be NULL) = the rows that passed.  When more than max_results passed the best max_results are kept; what is
 *     kept comes back best first.  Both steps use the canonical (distance in metric order, row ascending) key, -0 == +0 (the
 *     reference's select_nth_unstable_by / sort_unstable_by leave ties unpinned).  The distances are the computed values.
 *  5. Layout: out_rows / out_dists hold nq * max_results entries, out_counts[q] = min(passed, max_results) of them valid, the rest
 *     padded with row ~0 and the worst distance of the metric, like the other searches.  nq == 0 or max_results == 0: LYNSE_OK, only
 *     the counts are written and no device is touched.  A NULL required pointer: LYNSE_ERR_INVALID_ARGUMENT.
 *  Refused with LYNSE_ERR_UNSUPPORTED: a row-sharded handle (set_row_map with stride != 1 or offset != 0) and a row too wide for
 *  a query and a row to share the 160 KiB of LDS (dim beyond ~20,000).  A FLAT-handle entry: IVF and SPANN handles have none, and
 *  there is no ticket (submit / wait) form.  The search holds the handle's lock EXCLUSIVELY (its scratch — the score matrix, the
 *  selection state, the keys — is per handle) and runs on context 0, so it is refused while tickets are outstanding.  Queries go
 *  in chunks that keep the score matrix at or under 512 MiB and the kept keys at or under 256 MiB. */
int lynse_hip_flat_search_range_f32(lynse_hip_flat *h, const float *queries, uint64_t nq,
                                    const float *thresholds /* nq */, uint32_t max_results, int metric,
                                    const uint64_t *bitset_words /* NULL = every row */, uint64_t n_words,
                                    uint64_t *out_rows /* nq*max_results */, float *out_dists, uint32_t *out_counts /* nq */,
                                    uint64_t *out_passed /* nq, may be NULL: rows that passed before the cap */);
/* Same with every buffer already resident in this handle's device memory; enqueued on `stream`
 * (a hipStream_t, NULL = the handle's own non-blocking stream) and synchronised before returning.
 * Device inputs of every *_device entry must be COMPLETE when the call is made (synchronise the
 * stream that produced them): the handle's stream does not order against other streams. */
int lynse_hip_flat_search_f32_device(lynse_hip_flat *h, const float *d_queries, uint64_t nq,
                                     uint32_t k, int metric, uint64_t *d_out_rows,
                                     float *d_out_dists, uint32_t *d_out_counts, void *stream);
/* packed_binary_search (flat_mmap.rs:1345-1409) with pre-packed queries (nq * words u64). */
int lynse_hip_flat_search_packed_u64(lynse_hip_flat *h, const uint64_t *query_words, uint64_t nq,
                                     uint32_t k, int metric, uint64_t *out_rows, float *out_dists,
                                     uint32_t *out_counts);
int lynse_hip_flat_search_packed_u64_device(lynse_hip_flat *h, const uint64_t *d_query_words,
                                            uint64_t nq, uint32_t k, int metric,
                                            uint64_t *d_out_rows, float *d_out_dists,
                                            uint32_t *d_out_counts, void *stream);
/* THE APPROXIMATE FLAT SEARCH (the contract block next to the metric enum).  One query of dim f32; out_rows / out_dists hold k entries,
 * *out_count = min(k, len) of them valid, best first, distances unrounded. */
int lynse_hip_flat_search_approx_f32(lynse_hip_flat *h, const float *query, uint32_t k, int metric, float eps,
                                     uint64_t *out_rows, float *out_dists, uint32_t *out_count,
                                     lynse_hip_approx_info *out_info /* may be NULL */);
/* normalize_eps (approx_search.rs:113-119): non-finite or <= 0 -> 1e-4, else max(eps, 1e-8). */
float lynse_hip_normalize_eps(float eps);
/* round_distances_to_eps (approx_search.rs:123-143), in place; eps <= 0 or NaN changes nothing. */
void lynse_hip_round_distances_to_eps(float *dists, size_t n, float eps);
/* The size policy of the approximate search (host only, eps already normalised): flat_mmap.rs:3739-3771, :3930-3962, :4024-4056,
 * :3911-3927, :4003-4021 and sampled_dim_blocks, :4468-4496 (out_start / out_len hold three entries; returns the number of blocks). */
uint64_t lynse_hip_approx_ip_order_pool(uint64_t k, uint64_t n, float eps);
uint64_t lynse_hip_approx_hybrid_ip_pool(uint64_t k, uint64_t n, float eps);
uint64_t lynse_hip_approx_hybrid_pool(uint64_t k, uint64_t n, float eps);
uint32_t lynse_hip_approx_hybrid_ip_sample_dims(uint32_t dim, float eps);
uint32_t lynse_hip_approx_hybrid_sample_dims(uint32_t dim, float eps);
uint32_t lynse_hip_approx_sampled_dim_blocks(uint32_t dim, uint32_t sample, uint32_t *out_start, uint32_t *out_len);

/* Profiling: when enabled, searches bracket the scan kernel with HIP events on its stream.  on = n > 1 times every n-th
 * search only (an event recorded between two kernels costs a few microseconds of the stream's time). */
int lynse_hip_flat_profile_enable(lynse_hip_flat *h, int on);
int lynse_hip_flat_profile_get(lynse_hip_flat *h, lynse_hip_profile *out, int reset);
/* Coarse-pass state of a shard (no reference counterpart: the reference has one exact kernel, flat_mmap.rs:4845-4982;
 * here a certified low-precision pass runs in front of the exact rescoring and can be switched off by the data):
 * strikes = candidate overflows of the certified int8 pass so far (3 switch it off for the handle; -1 = off because the
 * rows are not finite), sq8_rows = rows covered by the SQ8 codes currently built (0 = none). */
int lynse_hip_flat_coarse_state(lynse_hip_flat *h, int *out_strikes, uint64_t *out_sq8_rows);
/* Rows covered by the +-1 byte copy of the packed rows that feeds batched Hamming searches (>= 96 queries) to the int8 MFMA
 * (packed_binary_search for a batch, flat_mmap.rs:1345-1409); 0 = not built (diagnostics / tests). */
uint64_t lynse_hip_flat_bpm_rows(const lynse_hip_flat *h);
/* Builds the derived copies a batch of nq queries of `metric` will read NOW instead of inside the first such search
 * (the reference's ensure_binary / ensure_sq8 are lazy as well, flat_mmap.rs:375-401): statistics + f16 shadow, SQ8 codes of
 * the certified int8 pass, packed words, the +-1 byte copy of batched Hamming.  lynse_hip_flat_hbm_bytes: HBM held by the
 * shard, source rows + derived copies. */
int lynse_hip_flat_prepare(lynse_hip_flat *h, int metric, uint64_t nq);
uint64_t lynse_hip_flat_hbm_bytes(const lynse_hip_flat *h);
/* Tuning knobs (defaults are fine): first-stage rows and growth factor of the contiguous stage plan (the fallback of the
 * default sampled plan), candidate capacity per query (power of two in [256, 16384], default 16384; k <= cap / 4 when the
 * shard holds more than cap rows). */
/* Few queries (<= 4) over a small shard (<= 64 MB of rows) with k <= 64 are answered by ONE fused launch
 * (k_small_search: exact scores straight from the f32 rows, per-wave top-k in registers, last-workgroup merge) instead
 * of the staged pipeline — the single-query latency path (flat_search_bench.py: 100k x 128, k = 10).  Results are
 * identical; on = 0 forces the staged pipeline (tests, A/B). */
int lynse_hip_flat_set_fused_search(lynse_hip_flat *h, int on);
int lynse_hip_flat_set_plan(lynse_hip_flat *h, uint32_t stage0_rows, uint32_t growth, uint32_t cap);

/* ---- stand-alone functions (src/python/mod.rs:2161-2223) ---- */
/* py_compute_distance -> distance::compute_distance_f32 (distance/mod.rs:193-213). */
int lynse_hip_compute_distance(const float *a, const float *b, uint32_t dim, int metric, int device,
                               float *out);
/* py_top_k_search -> distance::top_k_search (distance/mod.rs:373-422): u32 indices. */
int lynse_hip_top_k_search(const float *query, const float *candidates, uint64_t n, uint32_t dim,
                           uint32_t k, int metric, int device, uint32_t *out_idx, float *out_dist,
                           uint32_t *out_count);
/* pack_binary_f32 (simd.rs:760-763) for n rows on the device. */
int lynse_hip_pack_binary_f32(const float *rows, uint64_t n, uint32_t dim, int device,
                              uint64_t *out_words);
/* VectorStore::merge_results (vector_store.rs:953-970) / cluster::merge_search_blocks
 * (cluster.rs:327-393): host k-way merge of per-shard candidates, canonical (dist, id) order.
 * ids/dists: n_lists blocks of `stride` entries, counts[i] valid in block i. */
int lynse_hip_merge_topk(const uint64_t *ids, const float *dists, const uint32_t *counts,
                         uint32_t n_lists, uint32_t stride, uint32_t k, int metric,
                         uint64_t *out_ids, float *out_dists, uint32_t *out_count);

/* Device-side variant used after the RCCL all-gather of per-rank result blocks.  `blocks` holds
 * n_lists blocks of `block_bytes`; inside a block: rows u64[nq*k] at rows_off, dists f32[nq*k] at
 * dists_off, counts u32[nq] at counts_off (the message shape of rpc.rs:1156-1177, fixed size).
 * Output: merged rows u64[nq*k], dists f32[nq*k], counts u32[nq] in device memory.  Enqueued on
 * `stream` (hipStream_t; NULL = default stream) without synchronising. */
int lynse_hip_merge_topk_device(const void *d_blocks, uint64_t block_bytes, uint64_t rows_off,
                                uint64_t dists_off, uint64_t counts_off, uint32_t n_lists,
                                uint64_t nq, uint32_t k, int metric, uint64_t *d_out_rows,
                                float *d_out_dists, uint32_t *d_out_counts, void *stream);

/* ---- IVF-Flat: IVFIndex (src/index/ivf.rs) / IvfFlatMmap (src/storage/ivf_flat_mmap.rs) ---- */

/* Build from host rows with device k-means (kmeans.rs:74-139 semantics: FastRng(42) init,
 * Lloyd <= max_iter, empty-cluster reseed, final re-assign).  routing follows ivf.rs:81-87
 * (`l2_partitions` = 1 forces L2 Voronoi cells like IvfFlatMmap::build, ivf_flat_mmap.rs:98).
 * A binary metric (hamming / jaccard / dice / tanimoto) builds the IVF-*-BINARY mode
 * (src/index/mod.rs:376-385, ivf.rs:147-175): BinaryQuantizer::fit on the device (quantizer/mod.rs:321-356:
 * 0.5 for {0,1} corpora, else per-dimension median with midrange fallback), rows stored as their {0,1}
 * codes + packed u64 words, k-means and routing with L2 on the codes, packed popcount list scans. */
int lynse_hip_ivf_build(const float *rows, uint64_t n, uint32_t dim, uint32_t nlist,
                        uint32_t max_iter, int metric, int l2_partitions, int device,
                        lynse_hip_ivf **out);
/* Load given centroids (nlist*dim) + assignments (n): parity tests feed the oracle's. */
int lynse_hip_ivf_load(const float *rows, uint64_t n, uint32_t dim, const float *centroids,
                       uint32_t nlist, const uint32_t *assignments, int metric, int device,
                       lynse_hip_ivf **out);
/* Binary-metric load: `rows` are the RAW rows, binarised on the device with `thresholds` (dim floats,
 * BinaryQuantizer state) before the slabs are laid out. */
int lynse_hip_ivf_load_binary(const float *rows, uint64_t n, uint32_t dim, const float *centroids,
                              uint32_t nlist, const uint32_t *assignments, int metric,
                              const float *thresholds, int device, lynse_hip_ivf **out);
/* Fitted BinaryQuantizer state of a binary index: thresholds[dim], already_binary flag. */
int lynse_hip_ivf_thresholds(const lynse_hip_ivf *h, float *thresholds, int *already_binary);
/* IVF-{IP,L2,COS}-SQ8 (src/index/mod.rs:361-375; IVFIndex with QuantizerType::Scalar, ivf.rs:132-337; ScalarQuantizer,
 * quantizer/mod.rs:110-250).  ip / l2 / cosine only.
 *  - fit: per dimension min from f32::MAX and max from f32::MIN with strict < / > over all rows (NaN never wins),
 *    scale = (max - min) / 255 in f32, 1.0 where max == min (NOT the FLAT SQ8 scale 255 / range);
 *  - encode: ((v - min) / scale) clamped to [0, 255], truncated (NaN -> 0, +inf -> 255); decode: fl(fl(code * scale) + min);
 *  - build: k-means (train_for_metric, routing metric = index metric) on decode(encode(rows)); the slab store holds those
 *    decoded rows, the original f32 rows are kept beside them in HBM (twice the footprint of IVF-Flat, as the reference
 *    keeps data + encoded_data);
 *  - search (lynse_hip_ivf_search_f32 / _search_filtered_f32 / _search_f32_device): the query is encoded and decoded, the
 *    pool = min(max(10 k, k), |candidates|) best candidates by the distance of DECODED query and rows (the ordinary IVF
 *    search with k = pool: same probe rule, empty-probe fallback and subset), then rescored with compute_distance_f32 on the
 *    ORIGINAL query and rows; the best min(k, pool) come back with their exact distances.  Ties at BOTH cuts are pinned by the
 *    canonical (distance, original row) key — the reference's quickselect / sort_unstable leave them unpinned;
 *  - insert encodes with the fitted quantizer (no refit: values outside the range clamp) and assigns the decoded rows; delete
 *    reassigns the decoded rows that are left;
 *  - refused with LYNSE_ERR_UNSUPPORTED on an SQ8 handle: lynse_hip_ivf_search_metric_f32 (IvfFlatMmap semantics),
 *    lynse_hip_ivf_search_submit_f32_device (tickets), lynse_hip_ivf_search_sharded_f32_device and lynse_hip_ivf_set_row_map
 *    with a non-identity map (an SQ8 index is not row-sharded); there is no device-resident (_device) or sharded build /
 *    load of an SQ8 index.
 * lynse_hip_ivf_load_sq8 is the twin of lynse_hip_ivf_load_binary: `rows` are the ORIGINAL rows, `mins` / `scales` (dim each)
 * the quantizer; lynse_hip_ivf_sq8_params returns the fitted one. */
int lynse_hip_ivf_build_sq8(const float *rows, uint64_t n, uint32_t dim, uint32_t nlist, uint32_t max_iter, int metric,
                            int device, lynse_hip_ivf **out);
int lynse_hip_ivf_load_sq8(const float *rows, uint64_t n, uint32_t dim, const float *centroids, uint32_t nlist,
                           const uint32_t *assignments, const float *mins, const float *scales, int metric, int device,
                           lynse_hip_ivf **out);
int lynse_hip_ivf_sq8_params(const lynse_hip_ivf *h, float *mins, float *scales);
/* No reference counterpart (QueryProfile.rerank_us, src/engine.rs:6906-6919, is what it feeds): with lynse_hip_ivf_profile_enable on,
 * the SQ8 searches timed so far and their summed stage times in microseconds, from HIP events on the search stream:
 * out3[0] searches, out3[1] the pool stage (after the query codec -> after the pool stage), out3[2] the rerank (k_pool_rerank, plus
 * the host selection of a pool beyond 16,384).  reset != 0 clears them. */
int lynse_hip_ivf_sq8_stage_times(lynse_hip_ivf *h, double *out3, int reset);
/* SPANN-{IP,L2,COS}[-SQ8] (src/index/mod.rs:387-419; SPANNIndex, src/index/spann.rs): an IVF handle whose rows sit in up to
 * R + 1 posting lists (R = replica_count, at most 63).  rank(c) = distance(row, centroid c) (compute_distance_f32), negated for IP.
 *  - build (spann.rs:266-324): sq8 != 0 fits the ScalarQuantizer and works on decode(encode(rows)) from here on, as IVF-*-SQ8 does;
 *    k-means is train_for_metric(rows, n, dim, nlist, max_iter, metric), nlist = min(nlist, n).  R == 0: the lists are the k-means
 *    assignments; R >= 1: every row is placed by the posting rule against the FINAL centroids.  Lists hold rows in ascending order.
 *  - posting rule (posting_centroids_for_vector, :130-186): keep = min(R + 1, nlist) slots (+inf, none); for c = 0 .. nlist - 1 in
 *    order, c is skipped when rank(c) >= rank of the last slot (false for NaN), else inserted behind every slot whose rank is not
 *    greater.  No centroid in slot 0: list 0 only.  Else [slot 0], and for R >= 1 every later slot with rank <= p + max(|p|, EPS) *
 *    0.35000002 (p = rank of slot 0, f32, no fused multiply-add) while fewer than R + 1 lists are chosen.  For finite ranks the slots
 *    are the canonical (rank, centroid) top-keep; a row that can meet a non-finite rank follows the sequential rule literally.
 *  - search (:326-433; lynse_hip_ivf_search_f32 / _search_filtered_f32): an index of 0 rows is LYNSE_ERR_INDEX_NOT_BUILT; k == 0
 *    answers nothing; nprobe == 0 -> 1 (the build default nprobe of the reference is the caller's to pass), clamped to nlist.  The
 *    centroids are ranked as IVF ranks them; the candidates are the DISTINCT rows of the probed lists (intersected with the subset);
 *    fewer than k of them -> all (subset) rows.  Plain modes: the top k by (distance, row).  SQ8: the query is encoded and decoded,
 *    the pool = min(max(10 k, k), |candidates|) best candidates by decoded distance is rescored on the original query and rows and
 *    the best min(k, pool) kept; both cuts pinned by the (distance, row) key.  Short results are padded as everywhere (row ~0, the
 *    worst distance of the metric).
 *  - insert (:459-509, lynse_hip_ivf_insert_f32): the new rows are encoded with the fitted quantizer (no refit), placed by the posting
 *    rule against the unchanged centroids and appended to the end of each of their lists.  delete (:435-457, lynse_hip_ivf_delete_rows):
 *    the rows go, the rest are renumbered in order and ALL lists are rebuilt with the posting rule (R == 0 included).
 *  - lynse_hip_ivf_len is the number of rows, lynse_hip_ivf_nlist the number of lists; lynse_hip_ivf_sq8_params /
 *    _sq8_stage_times / _profile_* work as for IVF-*-SQ8.  Refused with LYNSE_ERR_UNSUPPORTED: lynse_hip_ivf_search_f32_device,
 *    lynse_hip_ivf_search_submit_f32_device, lynse_hip_ivf_search_sharded_f32_device, lynse_hip_ivf_search_metric_f32,
 *    lynse_hip_ivf_set_row_map, lynse_hip_ivf_set_routing, lynse_hip_ivf_assign_f32 and lynse_hip_ivf_export (they assume one list
 *    per row, a row map or another centroid ranking), lynse_hip_ivf_set_fused_search(h, 1) (the fused few-query selection assumes
 *    unique (distance, row) keys), and a binary metric at build / load.
 * lynse_hip_spann_load: `rows` are the ORIGINAL rows; the lists as list-major CSR (list_offsets nlist + 1, list_rows the rows of every
 * list); every row must sit in 1 .. replica_count + 1 distinct lists (else LYNSE_ERR_INVALID_ARGUMENT); mins / scales (dim each)
 * make it an SQ8 index, NULL a plain one.  lynse_hip_spann_postings returns the lists in the same form
 * (offsets nlist + 1, rows n_postings; NULL pointers are skipped). */
int lynse_hip_spann_build(const float *rows, uint64_t n, uint32_t dim, uint32_t nlist, uint32_t max_iter, int metric,
                          uint32_t replica_count, int sq8, int device, lynse_hip_ivf **out);
int lynse_hip_spann_load(const float *rows, uint64_t n, uint32_t dim, const float *centroids, uint32_t nlist,
                         const uint64_t *list_offsets, const uint32_t *list_rows, uint32_t replica_count, int metric,
                         const float *mins, const float *scales, int device, lynse_hip_ivf **out);
int lynse_hip_spann_postings(const lynse_hip_ivf *h, uint64_t *offsets, uint32_t *rows, uint64_t *n_postings);
int lynse_hip_spann_replica_count(const lynse_hip_ivf *h, uint32_t *replica_count);
/* IVFIndex::insert (src/index/ivf.rs:392-441): `rows` (n x dim f32; a binary index pushes them through its quantizer) are
 * assigned to the EXISTING centroids with the routing metric (every centroid in ascending order, strictly better wins) and
 * appended behind the rows already indexed (new row ids old_len .. old_len + n - 1); no retraining.
 * IVFIndex::delete (:350-390): the listed rows go, the rest keep their order under consecutive row ids and are all
 * reassigned to the existing centroids (kmeans::assign_metric).  lynse_hip_ivf_assign_f32 is the assignment rule alone. */
int lynse_hip_ivf_insert_f32(lynse_hip_ivf *h, const float *rows, uint64_t n);
int lynse_hip_ivf_delete_rows(lynse_hip_ivf *h, const uint64_t *row_ids, uint64_t n_ids);
int lynse_hip_ivf_assign_f32(lynse_hip_ivf *h, const float *rows, uint64_t n, uint32_t *out_assignments);
int lynse_hip_ivf_destroy(lynse_hip_ivf *h);
uint64_t lynse_hip_ivf_len(const lynse_hip_ivf *h);
uint32_t lynse_hip_ivf_nlist(const lynse_hip_ivf *h);
/* Trained state back to the host: centroids nlist*dim, assignments n, slab offsets nlist+1,
 * original row id per slab position (ivf_flat_mmap.rs:22-39).  NULL pointers are skipped. */
int lynse_hip_ivf_export(const lynse_hip_ivf *h, float *centroids, uint32_t *assignments,
                         uint64_t *offsets, uint32_t *original_ids);
int lynse_hip_ivf_set_row_map(lynse_hip_ivf *h, uint64_t stride, uint64_t offset);
/* Probe selection semantics: 0 = IVFIndex (rank every centroid, ivf.rs:227-249, empty-probe fallback
 * :258-265); 1 = IvfFlatMmap (IP 16-dim shortlist heuristic, ivf_flat_mmap.rs:381-421).  build() sets
 * it from `l2_partitions`, load() defaults to 0.  2 = keep the current routing but never fall back to the whole corpus
 * when the probed lists are empty: one ROW SHARD of a larger index must not answer from rows outside the probed lists
 * just because its own part of them is empty. */
int lynse_hip_ivf_set_routing(lynse_hip_ivf *h, int ivfflat_routing);
/* One to four queries (k <= 64, nprobe <= 64 < nlist, float metrics, exact centroid ranking, no subset) are answered by TWO
 * fused launches with no host round trip in between: k_small_search ranks the centroids, then scans the probed lists
 * straight from that ranking in device memory, every row scored exactly from the f32 slab — the reference's usual IVF
 * call is one query at a time (ivf.rs:181-348).  Same results as the staged path; on = 0 forces the staged path. */
int lynse_hip_ivf_set_fused_search(lynse_hip_ivf *h, int on);
/* IVFIndex::search (ivf.rs:181-348): rank all centroids with the routing metric, scan the nprobe
 * nearest lists, exact top-k of the probed rows.  nprobe == 0 -> 1 (ivf.rs:192-196). */
int lynse_hip_ivf_search_f32(lynse_hip_ivf *h, const float *queries, uint64_t nq, uint32_t k,
                             uint32_t nprobe, uint64_t *out_rows, float *out_dists,
                             uint32_t *out_counts);
/* Device-resident twins (float metrics): rows / queries / outputs already in HBM.  IvfFlatMmap::build reads its rows from an
 * mmapped store (src/storage/ivf_flat_mmap.rs:56-159); here k-means, the slab reordering (a gather inside HBM) and the
 * search never stage row data or candidates through host memory — one GPU's share of BASELINE config 4 is 19 GB.
 * Centroids and assignments (lynse_hip_ivf_load_device) are host arrays, as in lynse_hip_ivf_load. */
int lynse_hip_ivf_build_device(const float *d_rows, uint64_t n, uint32_t dim, uint32_t nlist,
                               uint32_t max_iter, int metric, int l2_partitions, int device,
                               lynse_hip_ivf **out);
int lynse_hip_ivf_load_device(const float *d_rows, uint64_t n, uint32_t dim, const float *centroids,
                              uint32_t nlist, const uint32_t *assignments, int metric, int device,
                              lynse_hip_ivf **out);
int lynse_hip_ivf_search_f32_device(lynse_hip_ivf *h, const float *d_queries, uint64_t nq, uint32_t k,
                                    uint32_t nprobe, uint64_t *d_out_rows, float *d_out_dists,
                                    uint32_t *d_out_counts);
/* IvfFlatMmap::search(query, k, nprobe, metric) (src/storage/ivf_flat_mmap.rs:225-305; PyIvfFlatIndex.search,
 * src/python/mod.rs:2130-2155): the metric of the CALL drives centroid routing, scoring and the sort direction (the
 * partitions are metric-agnostic).  Float indexes take ip / l2 / cosine; a binary index only its build metric. */
int lynse_hip_ivf_search_metric_f32(lynse_hip_ivf *h, const float *queries, uint64_t nq, uint32_t k,
                                    uint32_t nprobe, int metric, uint64_t *out_rows, float *out_dists,
                                    uint32_t *out_counts);
/* IVFIndex::search with SearchParams.subset (ivf.rs:251-265): the rows of the probed lists are intersected with
 * `subset_rows` (original row ids, host memory); a query whose probed lists hold no subset row is answered from the
 * whole corpus restricted to the subset, as the reference does.  One subset per batch. */
int lynse_hip_ivf_search_filtered_f32(lynse_hip_ivf *h, const float *queries, uint64_t nq, uint32_t k,
                                      uint32_t nprobe, const uint64_t *subset_rows, uint64_t n_subset,
                                      uint64_t *out_rows, float *out_dists, uint32_t *out_counts);
int lynse_hip_ivf_profile_enable(lynse_hip_ivf *h, int on);
int lynse_hip_ivf_profile_get(lynse_hip_ivf *h, lynse_hip_profile *out, int reset);

/* ---- multi-GPU exchange: one process per GPU, rows sharded, RCCL all-gather over xGMI ----
 *
 * Stands where the reference's TCP scatter / gather stands: fan-out of the batch to every shard (src/cluster.rs:101-123,
 * :173-217), the result block a shard returns (src/rpc.rs:1156-1177), the coordinator's merge (src/cluster.rs:327-393).
 * RCCL is bound at run time (dlopen; no link-time dependency): lynse_hip_comm_load_rccl(path) names the copy to use — a
 * host process that already carries one (PyTorch) passes its path so the process keeps ONE RCCL — else librccl.so.1 of
 * the loader path.  Bootstrap: rank 0 calls lynse_hip_comm_unique_id, the launcher hands the 128 bytes to every rank
 * (torch.distributed, MPI, a file), every rank calls lynse_hip_comm_create. */
typedef struct lynse_hip_comm lynse_hip_comm;
int lynse_hip_comm_load_rccl(const char *path /* NULL = search */);
int lynse_hip_comm_unique_id(uint8_t *id128);
int lynse_hip_comm_create(const uint8_t *id128, int rank, int world, int device, lynse_hip_comm **out);
/* A BLOCKING collective of a communicator that timed out (LYNSE_ERR_TIMEOUT: a rank is gone) leaves its all-gather / merge enqueued: the
 * communicator is marked failed — every later sharded call or submit on it returns LYNSE_ERR_DEVICE at once — and the output buffers of the
 * call that timed out must stay allocated until lynse_hip_comm_destroy. */
int lynse_hip_comm_destroy(lynse_hip_comm *c);
int lynse_hip_comm_rank(const lynse_hip_comm *c);
int lynse_hip_comm_world(const lynse_hip_comm *c);
/* Self-check: all-reduce(sum) of one word per rank; *out must equal the world size on every rank. */
int lynse_hip_comm_ranks_seen(lynse_hip_comm *c, int *out);
/* Whole-collection search of a row-sharded collection (a COLLECTIVE: every rank calls it with the same nq / k / metric):
 * scan of this rank's shard -> ncclAllGather of the fixed-size per-rank blocks [rows u64 | dists f32 | counts u32]
 * (nq*k*12 + nq*4 bytes) -> device k-way merge in the canonical (distance, global row) order, stream-ordered on the
 * shard's stream with no host synchronisation between the three.  Rows are global through the shard's row map
 * (lynse_hip_flat_set_row_map).  Outputs are device memory, identical on every rank, complete on return. */
int lynse_hip_flat_search_sharded_f32_device(lynse_hip_flat *h, lynse_hip_comm *c, const float *d_queries,
                                             uint64_t nq, uint32_t k, int metric, uint64_t *d_out_rows,
                                             float *d_out_dists, uint32_t *d_out_counts);
int lynse_hip_flat_search_sharded_packed_u64_device(lynse_hip_flat *h, lynse_hip_comm *c,
                                                    const uint64_t *d_query_words, uint64_t nq, uint32_t k,
                                                    int metric, uint64_t *d_out_rows, float *d_out_dists,
                                                    uint32_t *d_out_counts);
/* Row-sharded IVF search (BASELINE config 4): the local part of the probed lists -> ncclAllGather of the result blocks ->
 * device merge in the canonical (distance, global row) order, on the shard's stream.  Every rank holds its rows of every
 * list under the same centroids (lynse_hip_ivf_load_device with the shared centroids, lynse_hip_ivf_set_row_map for global
 * row ids, lynse_hip_ivf_set_routing(h, 2): no all-lists-empty fallback on a shard).  Stands where the reference fans an
 * index search out to its shard nodes and merges (src/cluster.rs:101-123, :173-217, :327-393).  A collective. */
int lynse_hip_ivf_search_sharded_f32_device(lynse_hip_ivf *h, lynse_hip_comm *c, const float *d_queries, uint64_t nq,
                                            uint32_t k, uint32_t nprobe, uint64_t *d_out_rows, float *d_out_dists,
                                            uint32_t *d_out_counts);
/* Row-sharded IVF TRAINING: k-means over the whole collection (src/index/kmeans.rs:74-139) with every rank holding only its rows
 * (global row g = local row g / world on rank g % world).  Same FastRng sample + farthest-first init, assignment, last-maximum /
 * empty-cluster rules and stop test as training on the union; the centroid sums are formed per rank (sequential over the rank's
 * members, kmeans.rs:273-286) and added over the ranks IN RANK ORDER, ((p0 + p1) + p2) + ... with f32 adds — the result is defined
 * bit for bit at every world size (an all-reduce associates as it likes from three ranks on).  Per Lloyd iteration: nlist * dim
 * floats per rank + nlist + 1 integer words.  Every rank gets the same centroids (out_centroids: nlist x dim, *out_k
 * lists trained) and the assignments of its rows; load the shard with lynse_hip_ivf_load / _load_device afterwards.  The
 * reduction: the library's communicator `c` (on device buffers: ncclAllGather of the per-rank sums + a rank-ordered add kernel +
 * one integer ncclAllReduce), or — c == NULL — the launcher's callback, which sums a HOST buffer of `count` elements over all
 * ranks in place (dtype 0: f32 in any order — only ever one non-zero contribution per element —, 1: u32, 2: f32 in RANK order as
 * above; 0 = success).  rows_on_device: rows_local is device memory.  A collective.  (No reference counterpart: the reference's
 * cluster mode trains one index per shard node.) */
typedef int (*lynse_hip_reduce_fn)(void *ctx, void *buf, uint64_t count, int dtype);
int lynse_hip_ivf_kmeans_sharded(const float *rows_local, uint64_t n_local, int rows_on_device, uint64_t n_global,
                                 uint32_t rank, uint32_t world, uint32_t dim, uint32_t nlist, uint32_t max_iter, int metric,
                                 int device, lynse_hip_comm *c, lynse_hip_reduce_fn reduce, void *reduce_ctx,
                                 float *out_centroids, uint32_t *out_assignments, uint32_t *out_k);

/* IVFIndex::build (src/index/ivf.rs:132-179) for ONE RANK of a row-sharded collection, in one call: lynse_hip_ivf_kmeans_sharded over the
 * rank's device-resident rows (global row g = local row g / world on rank g % world), then the rank's slab store under the shared
 * centroids with global row ids (lynse_hip_ivf_set_row_map(h, world, rank)) and the shard routing rule (no all-lists-empty fallback
 * when world > 1) — the index lynse_hip_ivf_search_sharded_f32_device and the IVF tickets search.  A collective; every rank needs at
 * least one row.  ivfflat_routing != 0: IvfFlatMmap semantics (L2 cells, src/storage/ivf_flat_mmap.rs:56-159). */
int lynse_hip_ivf_build_sharded_device(const float *d_rows_local, uint64_t n_local, uint64_t n_global, uint32_t rank,
                                       uint32_t world, uint32_t dim, uint32_t nlist, uint32_t max_iter, int metric,
                                       int ivfflat_routing, int device, lynse_hip_comm *c, lynse_hip_reduce_fn reduce,
                                       void *reduce_ctx, lynse_hip_ivf **out);

/* ---- searches in flight: submit / wait ----
 *
 * The reference serves concurrent readers (Arc<RwLock<Collection>> with inner.read() on the search path,
 * src/python/mod.rs:950, :1187; RPC / HTTP workers call search concurrently, src/rpc.rs:588-590): a batch does not wait
 * for the previous one to be answered.  submit enqueues a whole batch of <= 256 queries on one of the handle's search
 * contexts (stream + workspace; LYNSE_HIP_CONTEXTS of them) — the staged pipeline and, with a communicator, the
 * ncclAllGather of the result blocks and the device merge — and returns a ticket; wait blocks until that batch is final in
 * the caller's DEVICE arrays (identical to the blocking entry points: an overflowed plan is re-run on the next plan level
 * inside wait, on every rank of a sharded collection) and frees the ticket.  `c` = NULL: this shard only.  Queries and
 * outputs must stay valid until wait returns.  Tickets are waited for by the thread that submitted them, in any order;
 * append / finalize and the filtered searches need every ticket waited for first.  With a communicator submit is a
 * COLLECTIVE: every rank submits and waits for the same sequence.  A search that cannot be pipelined (more than 256
 * queries, k beyond one pass, the fused few-query search, derived data still to build) is answered inside submit. */
typedef struct lynse_hip_ticket lynse_hip_ticket;
int lynse_hip_flat_search_submit_f32_device(lynse_hip_flat *h, lynse_hip_comm *c, const float *d_queries, uint64_t nq,
                                            uint32_t k, int metric, uint64_t *d_out_rows, float *d_out_dists,
                                            uint32_t *d_out_counts, lynse_hip_ticket **out);
int lynse_hip_flat_search_submit_packed_u64_device(lynse_hip_flat *h, lynse_hip_comm *c,
                                                   const uint64_t *d_query_words, uint64_t nq, uint32_t k, int metric,
                                                   uint64_t *d_out_rows, float *d_out_dists, uint32_t *d_out_counts,
                                                   lynse_hip_ticket **out);
int lynse_hip_flat_search_wait(lynse_hip_ticket *t);
/* Upper bound of one lynse_hip_flat_search_wait in milliseconds, process-wide.  0 (default): tickets of ONE shard wait without a
 * limit, tickets that end in a collective (submitted with a communicator) give up after 30 s — a rank that died inside the
 * exchange would otherwise hang its peers forever (the reference's scatter-gather times its shard calls out the same way,
 * src/cluster.rs:173-217).  On expiry wait returns LYNSE_ERR_TIMEOUT; the ticket is freed, its context is NOT reused (the device
 * may still be writing into it).  LYNSE_HIP_WAIT_TIMEOUT_MS sets the initial value. */
int lynse_hip_set_wait_timeout_ms(uint32_t ms);

/* IVF searches in flight (IVFIndex::search, src/index/ivf.rs:181-348, under the same concurrent readers): submit ENQUEUES a batch of
 * <= 256 queries of a float IVF index on one of the slab store's search contexts 1 .. LYNSE_HIP_CONTEXTS-1 (context 0 stays with
 * the blocking searches, which keep working next to tickets) — query images, the centroid ranking, device-side grouping, the list
 * scans, exact rescoring and, with a communicator, the ncclAllGather of the result blocks + the device merge — with NO host
 * synchronisation in between; wait blocks until the batch is final in the caller's DEVICE arrays and frees the ticket.  Results
 * are those of lynse_hip_ivf_search_f32_device / lynse_hip_ivf_search_sharded_f32_device: whatever the blocking path would have
 * checked on the host (candidate overflow of the scans or of the centroid ranking, the all-lists-empty fallback of ivf.rs:258-265)
 * travels as a status word and is re-answered by the blocking ladder inside wait, on every rank of a sharded index.  The index
 * metric is used.  A shape the device-side grouping does not take (nprobe >= nlist, more than 16384 (query, list) pairs, more
 * than 8192 lists) is answered synchronously inside submit (a sharded ticket still exchanges in flight); binary indexes and k
 * beyond the staged pipeline return LYNSE_ERR_UNSUPPORTED.  insert / delete are refused while tickets are outstanding.  With a
 * communicator submit is a COLLECTIVE: every rank submits and waits for the same sequence; one communicator serves the tickets of
 * ONE handle at a time.  lynse_hip_set_wait_timeout_ms applies. */
typedef struct lynse_hip_ivf_ticket lynse_hip_ivf_ticket;
int lynse_hip_ivf_search_submit_f32_device(lynse_hip_ivf *h, lynse_hip_comm *c, const float *d_queries, uint64_t nq, uint32_t k,
                                           uint32_t nprobe, uint64_t *d_out_rows, float *d_out_dists, uint32_t *d_out_counts,
                                           lynse_hip_ivf_ticket **out);
int lynse_hip_ivf_search_wait(lynse_hip_ivf_ticket *t);
/* out[0..2]: tickets of this index whose local part was enqueued without a host synchronisation / answered inside submit /
 * re-answered inside wait (monitoring; that a batch ran in flight is not visible in its results). */
int lynse_hip_ivf_ticket_stats(lynse_hip_ivf *h, uint64_t *out);

/* Diagnostics of the certified coarse pass (no reference counterpart: the reference scans f32 rows).  For a shard of at most `cap`
 * (16,384) rows and 1..256 host queries: out_scores[q][row] = the COARSE score of (row, query) exactly as the scan kernels compute
 * it (one emit-all stage of the real pipeline), in the metric's own space (IP: score; L2 / cosine: distance); out_bound[q] = the
 * bound E the pipeline certified for |coarse - reference-order f32 score| (the margin it keeps is 2E).  coarse = 0: the f16 shadow,
 * 1: the certified int8 pass; *out_form (may be NULL): bit 0 int8, bit 1 augmented-L2 codes, bit 2 plain-code L2 (exact f32 row
 * norms), bit 3 unit-row cosine codes.  tests/test_gpu_certificate.py holds the bound against constructed worst cases. */
int lynse_hip_flat_coarse_scores(lynse_hip_flat *h, const float *queries, uint64_t nq, int metric, int coarse,
                                 float *out_scores, float *out_bound, int *out_form);

/* The same diagnostics for the SQ7 form of the FLAT-IP int8 pass: the scan of batches of 129..256 queries may read a NON-NEGATIVE 7-bit
 * copy of the codes (scale 127 / range, codes 0..127 stored without an offset) instead of the SQ8 codes — chosen on non-negative shards
 * of >= 10M rows, LYNSE_HIP_SQ7=1 / 0 forces / disables it; results never change, last_plan bit 26 tells.  129..256 queries;
 * LYNSE_ERR_UNSUPPORTED where the shape has no SQ7 scan.  *out_form gains bit 4. */
int lynse_hip_flat_coarse_scores_sq7(lynse_hip_flat *h, const float *queries, uint64_t nq, float *out_scores, float *out_bound, int *out_form);
/* SQ7 state of a shard: rows the copy covers (0 = not built) and the overflows of its scan so far (each is re-answered on the SQ8 codes;
 * 3 switch SQ7 off for the handle). */
int lynse_hip_flat_sq7_state(lynse_hip_flat *h, uint64_t *out_rows, int *out_strikes);

/* THE PREDICTED PLAN of the certified int8 pass (FLAT-IP / cosine, 129..256 queries, k <= 32, unfiltered, blocking searches; last_plan
 * bit 28).  Each code set keeps the exact 64-bit column sums of its codes and of their squares; for a query image u the integer dot
 * product over the rows then has mean m_q = sum u_d mu_d and, on the diagonal model, variance v_q = sum u_d^2 sigma_d^2, and the search
 * runs prep -> ONE threshold stage over every row on thr = B_q + s_q (m_q + z sqrt(v_q)), n (1 - Phi(z)) = 40 k -> the select / rescoring
 * launch, which checks from the emitted keys that the threshold was valid (k keys arrived and the final cut tau_x - E is not below it).  A
 * chunk with a query that fails the check, or overflows, is answered again on the sampled plan: results never depend on the model.  Three
 * such chunks switch prediction off until the codes are fitted again.  LYNSE_HIP_PREDICT=1 / 0 forces / disables it; unset: shards of
 * >= 4M rows.  Tickets (lynse_hip_flat_search_submit_*), IVF, subset filters, squared L2 and the binary metrics keep their plans.
 *
 * The model on the host — no device involved: z for n rows and a target of keys_per_query emitted rows per query (0 when the target is
 * n / 2 or more); mu_d / sigma_d^2 (clamped at 0) from sums[0 .. cols) = sum c_d and sums[cols .. 2 cols) = sum c_d^2 over n rows; and
 * the threshold of one image u (sequential f64 sums, one f32 rounding of bq + sq (m + z sqrt(v))). */
int lynse_hip_predict_z(uint64_t n, double keys_per_query, double *out_z);
int lynse_hip_predict_col_stats(const int64_t *sums, uint32_t cols, uint64_t n, double *out_mu, double *out_var);
int lynse_hip_predict_threshold(const int8_t *u, const double *mu, const double *var, uint32_t cols, double z, float bq, float sq,
                                double *out_m, double *out_v, float *out_thr);
/* Diagnostics: what the prep kernel of a predicted batch computes for `queries` (129..256) at this k — the int8 image out_u[nq][cols],
 * B_q, s_q, m_q, v_q, the threshold and z — and the column statistics it read (out_mu / out_var[cols]; *out_cols = cols).  Builds the
 * codes and statistics a search of the shape would; LYNSE_ERR_UNSUPPORTED where such a search would not predict.  Outputs may be NULL. */
int lynse_hip_flat_predict_debug(lynse_hip_flat *h, const float *queries, uint64_t nq, uint32_t k, int metric, int8_t *out_u, double *out_mu,
                                 double *out_var, float *out_bq, float *out_sq, double *out_m, double *out_v, float *out_thr, double *out_z,
                                 uint32_t *out_cols);
/* Strikes of the predicted plan so far (3 switch it off) and the rows the column statistics of the SQ8 / unit-row / SQ7 code sets cover
 * (0 = not collected). */
int lynse_hip_flat_predict_state(lynse_hip_flat *h, int *out_strikes, uint64_t *out_rows_sq8, uint64_t *out_rows_cos, uint64_t *out_rows_sq7);

/* ---- sparse vectors: SparseVectorStore (src/engine.rs:550-718), index mode SPARSE-FLAT-IP ---- */

/* SPARSE VECTORS (Collection::add_sparse_vectors / search_sparse, src/engine.rs:4250-4279, :4962-5002).  A sparse vector is a list of
 * (u32 index, f32 value) pairs; the store is a CSR matrix in HBM (indptr u64[n + 1] | indices u32 | values f32, three arrays), rows
 * 0 .. n - 1.  The rules:
 *  1. Normalising (normalize_sparse_entries, :6925-6943), input pairs in any order: a non-finite value is the error "sparse vector
 *     values must be finite"; values == 0.0 are skipped; the rest are merged per index in input order (each index starts at 0.0f and
 *     takes += value in f32); entries whose merged value is 0.0 are dropped; the output ascends by index.
 *     lynse_hip_sparse_normalize does this for n vectors in CSR into caller buffers (never longer than the input); host only, no
 *     handle, no device.
 *  2. Scoring (sparse_inner_product, :6945-6965): score = 0.0f; for each index present in both vectors, in ascending index order,
 *     score += q * v — the multiply and the add are separate f32 operations, never fused.
 *  3. Search (SparseVectorStore::search, :660-695): a row is a result only if score != 0.0 (a plain IEEE comparison: a score that
 *     cancels to +-0 and a row with no common index are dropped, a NaN score — inf - inf after overflow — is kept); the order is score
 *     descending, then row ascending; at most k come back.  NaN follows the NON-FINITE VALUES rule: reported as -inf, ranked last,
 *     ties by row; +-inf are ordinary values.  An empty query or k == 0: an empty result.
 *  4. lynse_hip_sparse_set_rows replaces the whole store (upsert_many rewrites its whole map too).  Checked before any device work:
 *     indptr[0] == 0 and non-decreasing, indices strictly ascending within a row, values finite and non-zero, n < 2^32 (a selection
 *     key carries a 32-bit row) — LYNSE_ERR_INVALID_ARGUMENT otherwise.  Empty rows are legal and never score; n == 0 empties the store.
 *  5. lynse_hip_sparse_search takes nq NORMALISED queries in CSR, validated like rows (LYNSE_ERR_INVALID_ARGUMENT).  Layout as
 *     lynse_hip_flat_search_f32: stride k, out_counts[q] entries valid, the rest padded with row ~0 and -inf.  out_passed[q] (may be
 *     NULL) = the rows with a non-zero score before the cut.  bitset_words are the reference's BitSet words over sparse rows, treated
 *     as lynse_hip_flat_search_range_f32 treats its words (NULL = every row, rows the words do not cover are out, bits at or beyond n
 *     are ignored).  The call holds the handle's lock EXCLUSIVELY (the scratch is per handle) and goes in query chunks that keep the
 *     score matrix at or under 512 MiB.
 *  6. Limit: a query of more than 4,096 entries is refused with LYNSE_ERR_UNSUPPORTED before any launch — a query tile's lookup table
 *     (at most half full, a power of two of slots) has to fit the 160 KiB of LDS next to the staged results, and 8,192 slots is the
 *     largest that does.  Tiles hold up to 16 queries and shrink down to 1 before anything is refused.
 *  7. Profile: scan_launches, scan_us, scan_rows, scan_bytes = (nnz * 8 + (n + 1) * 8) per query tile (each tile streams the CSR once),
 *     total_us = first launch to last launch of a chunk.
 * Without a usable HIP device lynse_hip_sparse_create returns LYNSE_ERR_DEVICE: there is no CPU fallback. */
typedef struct lynse_hip_sparse lynse_hip_sparse;
int lynse_hip_sparse_normalize(const uint64_t *indptr /* n+1 */, const uint32_t *indices, const float *values, uint64_t n,
                               uint64_t *out_indptr /* n+1 */, uint32_t *out_indices, float *out_values);
int lynse_hip_sparse_create(int device, lynse_hip_sparse **out);
int lynse_hip_sparse_destroy(lynse_hip_sparse *h);
int lynse_hip_sparse_set_rows(lynse_hip_sparse *h, const uint64_t *indptr /* n+1 */, const uint32_t *indices,
                              const float *values, uint64_t n);
int lynse_hip_sparse_len(lynse_hip_sparse *h, uint64_t *out_rows, uint64_t *out_nnz);
uint64_t lynse_hip_sparse_hbm_bytes(lynse_hip_sparse *h);
int lynse_hip_sparse_search(lynse_hip_sparse *h, const uint64_t *q_indptr /* nq+1 */, const uint32_t *q_indices,
                            const float *q_values, uint64_t nq, uint32_t k,
                            const uint64_t *bitset_words /* NULL = every row */, uint64_t n_words,
                            uint64_t *out_rows /* nq*k */, float *out_scores, uint32_t *out_counts /* nq */,
                            uint64_t *out_passed /* nq, may be NULL */);
int lynse_hip_sparse_profile_enable(lynse_hip_sparse *h, int on);
int lynse_hip_sparse_profile_get(lynse_hip_sparse *h, lynse_hip_profile *out, int reset);

/* ---- text search: InvertedTextIndex (src/engine.rs:720-1118), index mode BM25-INVERTED ---- */

/* TEXT SEARCH (Collection::text_search, src/engine.rs:5056-5076, over InvertedTextIndex::search, :927-1054).  The caller tokenises
 * (tokenize_text, :7031-7049), indexes the documents (index_document, :1077-1107) and applies the field selection
 * (TextFieldSelection, :6967-6989); the library holds the postings of ONE selection and answers BM25 queries over term ids.  The rules:
 *  1. Store (lynse_hip_text_set, replaces the whole store).  Rows 0 .. n - 1 are the documents of selected length > 0 — in ascending
 *     user id the library's (score, row) order is the reference's (score, id) order.  doc_len u32[n], every entry >= 1.  Postings in
 *     CSC form: term_ptr u64[V + 1], post_row u32[nnz] strictly ascending within a term, post_tf u32[nnz] >= 1.  Checked on the host
 *     before any device work: term_ptr[0] == 0 and non-decreasing, rows < n, n < 2^32 and V < 2^32, tf >= 1, and per row the tf values
 *     sum to doc_len[row] — LYNSE_ERR_INVALID_ARGUMENT otherwise.  n == 0 or V == 0 empties the store.  doc_len, post_row and post_tf
 *     live in HBM; term_ptr stays on the host (a query's slot table carries its posting ranges to the device).
 *  2. A query is its distinct KNOWN terms as (term id, count >= 1) in SLOT ORDER — the order of first occurrence in the query text;
 *     terms the store has never seen are dropped by the caller (in the reference they have df = 0 and no effect).  nq queries go as
 *     CSR (q_ptr u64[nq + 1], q_terms, q_counts).  A term id >= V, a term id twice in one query or a count of 0:
 *     LYNSE_ERR_INVALID_ARGUMENT.
 *  3. Search.  "Live" = a row the mask leaves in; bitset_words are BitSet words over text rows, treated as lynse_hip_sparse_search
 *     treats its words (NULL = every row, rows the words do not cover are out, bits at or beyond n are ignored); tombstones and
 *     subsets are folded in by the caller.  Every f32 step below is a separate round-to-nearest operation, never fused.
 *     a. docs = live rows, total = the sum of doc_len over them; docs == 0: an empty result.
 *     b. n_docs = (f32)docs, avg = max((f32)total / (f32)docs, 1.0f).
 *     c. df_t = live postings of term t; terms with df_t == 0 are ignored from here on; none left: an empty result.
 *     d. min_df = the least df_t, cutoff = max(sat_mul(min_df, 4), sat_mul(k, 8)) in 64-bit unsigned arithmetic; term t is a
 *        CANDIDATE TERM if df_t < docs && df_t <= cutoff; if no term qualifies, every term is one.
 *     e. idf_t = logf(((n_docs - df_t) + 0.5f) / (df_t + 0.5f) + 1.0f) with df_t as f32, by the host's libm; w_t = (f32)count_t * idf_t.
 *     f. score(row) = 0.0f; then for each slot IN SLOT ORDER whose term occurs in the row with frequency tf:
 *          score += (w_t * (tf * K)) / (tf + 1.2f * (0.25f + (0.75f * dl) / avg)),  K = 1.2f + 1.0f, tf and dl = doc_len[row] as f32.
 *        The reference sums in the iteration order of a HashMap, which varies from run to run; SLOT ORDER IS THIS LIBRARY'S PIN.
 *     g. A row is a result iff it is live, contains at least one candidate term and score > 0.0f; order: score descending, row
 *        ascending; at most k come back.  k == 0 or a batch of empty queries: an empty result without touching the device.  Layout as
 *        lynse_hip_sparse_search: stride k, out_counts[q] entries valid, the rest padded with row ~0 and -inf; out_passed[q] (may be
 *        NULL) = the results before the cut.
 *     h. Limit: a query of more than 256 distinct known terms is refused with LYNSE_ERR_UNSUPPORTED before any launch (the scan's
 *        prologue places one slot per lane of its 256-thread workgroup).
 *     Rules a and c under a mask are exact integer counts from the device (k_text_stats); without a mask df_t is the length of the
 *     posting list and the corpus totals are kept from set.  Rules b, d and e run on the host: lynse_hip_text_weights is that step
 *     alone (no handle, no device): out_w[t] = 0 and out_cand[t] = 0 for df[t] == 0, *out_avg = 1 and nothing else for docs == 0.
 *     The call holds the handle's lock EXCLUSIVELY (the scratch is per handle) and goes in query chunks that keep the score matrix
 *     at or under 512 MiB.
 *  4. Profile: scan_launches, scan_us and scan_rows (n per query) of k_text_scan; scan_bytes = what the scan reads = 12 bytes per
 *     posting of the query's terms with a live posting (row 4 + tf 4 + the gathered doc_len 4; the binary searches of the prologue
 *     and the mask words are not counted); total_us = first launch to last launch of a chunk.
 * Without a usable HIP device lynse_hip_text_create returns LYNSE_ERR_DEVICE: there is no CPU fallback. */
typedef struct lynse_hip_text lynse_hip_text;
int lynse_hip_text_weights(uint64_t docs, uint64_t total, const uint64_t *df /* T */, const uint32_t *count /* T */, uint32_t T,
                           uint32_t k, float *out_avg, float *out_w /* T */, uint32_t *out_cand /* T */);
int lynse_hip_text_create(int device, lynse_hip_text **out);
int lynse_hip_text_destroy(lynse_hip_text *h);
int lynse_hip_text_set(lynse_hip_text *h, const uint32_t *doc_len /* n */, uint64_t n, const uint64_t *term_ptr /* V+1 */, uint64_t V,
                       const uint32_t *post_row, const uint32_t *post_tf);
int lynse_hip_text_len(lynse_hip_text *h, uint64_t *out_rows, uint64_t *out_terms, uint64_t *out_nnz);
uint64_t lynse_hip_text_hbm_bytes(lynse_hip_text *h);
int lynse_hip_text_search(lynse_hip_text *h, const uint64_t *q_ptr /* nq+1 */, const uint32_t *q_terms, const uint32_t *q_counts,
                          uint64_t nq, uint32_t k, const uint64_t *bitset_words /* NULL = every row */, uint64_t n_words,
                          uint64_t *out_rows /* nq*k */, float *out_scores, uint32_t *out_counts /* nq */,
                          uint64_t *out_passed /* nq, may be NULL */);
int lynse_hip_text_profile_enable(lynse_hip_text *h, int on);
int lynse_hip_text_profile_get(lynse_hip_text *h, lynse_hip_profile *out, int reset);

/* ---- field filters: FieldStore::query_from_index (src/storage/field_store.rs:1527-1590) ---- */

/* FIELD FILTERS (`where=`).  The reference answers a `where` string from in-memory maps of value -> ids when the string is one of the
 * four forms of query_from_index, and hands everything else to third-party SQL (ApexBase), which this library does not have.  Here the
 * fields are typed COLUMNS in HBM, row-aligned with a shard, and one kernel (k_field_filter) evaluates the compiled predicate for every
 * row and writes the reference's BitSet words.  The caller parses the string (lynsedb_amd/fields.py follows the reference's parsers
 * function for function) and owns the string dictionaries; the library holds columns and evaluates leaves.  The rules:
 *  1. A column (lynse_hip_fields_set_column, replaces the whole column `column` < 4096): per row a one-byte tag and an 8-byte payload.
 *       LYNSE_FIELD_MISSING 0  the row does not carry the field          LYNSE_FIELD_NULL 1   JSON null
 *       LYNSE_FIELD_BOOL 2     payload 0 / 1                              LYNSE_FIELD_INT 3    payload = the i64 (IndexKey::Int)
 *       LYNSE_FIELD_FLOAT 4    payload = normalize_f64_bits (:223-230: b | 1 << 63 for a clear sign bit, ~b otherwise; -0.0 and +0.0
 *                              are different keys)                        LYNSE_FIELD_STR 5    payload = a u32 code into the caller's dictionary
 *       LYNSE_FIELD_ARRAY 6    payload = the row's index a into arr_ptr (u64[n_arrays + 1]): its elements are (elem_tags, elem_payloads)
 *                              [arr_ptr[a], arr_ptr[a + 1]), scalars only (nested arrays and objects are skipped by the caller, :486-491)
 *       LYNSE_FIELD_OBJECT 7   never matched
 *     Checked on the host before any device work (LYNSE_ERR_INVALID_ARGUMENT, the column unchanged): tags <= 7, element tags 1 .. 5,
 *     an ARRAY row's payload < n_arrays, arr_ptr[0] == 0 and non-decreasing.  n == 0 drops the column.
 *  2. A leaf (lynse_hip_field_leaf) names a column; column == LYNSE_FIELD_NO_COLUMN or a column never set is a field no row carries
 *     and matches nothing (this library's rule: the reference asks SQL).  Kinds:
 *       EQ        tag == key_tag && payload == key.  Equality is equality of keys of one variant: Int 1 is not Float 1.0, `= null`
 *                 matches a stored null and not a missing field.
 *       NUM_RANGE (a number literal; key = its normalised bits) INT rows compare as normalize_f64_bits((double)i) — an integer beyond
 *                 2^53 rounds as `as f64` rounds it — FLOAT rows by their payload; unsigned order of the bits = RangeKey::Number's order.
 *                 By RangeKey's derived order every Text sorts after every Number: under GT / GE every STR row passes too.  NULL, BOOL,
 *                 MISSING, ARRAY and OBJECT rows never pass (get_range's BTreeMap path, :613-626; the dense-integer branch is the same
 *                 answer for all-integer fields).
 *       KEYSET    (`IN`, an OR of equalities on one field) aux = 9 u64 segment starts s[0 .. 8] then aux_len payloads, those of tag t at
 *                 [s[t], s[t + 1]) strictly ascending; s[0] == 0, non-decreasing, s[8] == aux_len <= 65,536.  A row passes if its
 *                 (tag, payload) is a key (binary search per lane).
 *       STRTABLE  (a text literal under a range operator; text compares bytewise) the caller evaluates the predicate over the column's
 *                 distinct strings: aux = a bit table over codes [0, aux_len).  STR rows pass by their code's bit; flags bit 0 = every
 *                 INT / FLOAT row passes (LT / LE: every Number is before every Text).
 *       CONTAINS  ARRAY rows with an element (tag, payload) == (key_tag, key).
 *  3. lynse_hip_fields_filter evaluates `combine` (LYNSE_FIELD_ALL = AND, LYNSE_FIELD_ANY = OR) of 1 .. 32 leaves for rows 0 .. n - 1;
 *     every column named must hold exactly n rows.  It leaves ceil(n / 64) BitSet words in the handle's device memory (bit r of word
 *     r / 64, LSB first; bits at and beyond n are zero), *out_count = the set bits (one 8-byte read-back), *out_kernel_us (may be
 *     NULL) = the kernel's duration between two HIP events.  The leaf offsets are checked against aux_words on the host before the
 *     launch.  n == 0: no launch, count 0.  lynse_hip_fields_words reads the words back; lynse_hip_fields_words_device gives the
 *     device pointer for lynse_hip_flat_search_filtered_bitset_device_f32 (valid until the next filter or destroy on this handle).
 *  4. The calls of one handle are serialised by the handle's lock.  The kernel uses vector stores and vector atomics only.
 * Without a usable HIP device lynse_hip_fields_create returns LYNSE_ERR_DEVICE: there is no CPU fallback. */
#define LYNSE_FIELD_MISSING 0
#define LYNSE_FIELD_NULL 1
#define LYNSE_FIELD_BOOL 2
#define LYNSE_FIELD_INT 3
#define LYNSE_FIELD_FLOAT 4
#define LYNSE_FIELD_STR 5
#define LYNSE_FIELD_ARRAY 6
#define LYNSE_FIELD_OBJECT 7
#define LYNSE_FIELD_LEAF_EQ 0
#define LYNSE_FIELD_LEAF_NUM_RANGE 1
#define LYNSE_FIELD_LEAF_KEYSET 2
#define LYNSE_FIELD_LEAF_STRTABLE 3
#define LYNSE_FIELD_LEAF_CONTAINS 4
#define LYNSE_FIELD_OP_LT 0
#define LYNSE_FIELD_OP_LE 1
#define LYNSE_FIELD_OP_GT 2
#define LYNSE_FIELD_OP_GE 3
#define LYNSE_FIELD_ALL 0
#define LYNSE_FIELD_ANY 1
#define LYNSE_FIELD_NO_COLUMN 0xffffffffu
#define LYNSE_FIELD_MAX_LEAVES 32
#define LYNSE_FIELD_MAX_KEYS 65536
typedef struct lynse_hip_field_leaf {
    uint32_t kind;      /* LYNSE_FIELD_LEAF_* */
    uint32_t column;
    uint32_t op;        /* NUM_RANGE: LYNSE_FIELD_OP_* */
    uint32_t flags;     /* STRTABLE: bit 0 = every number row passes */
    uint32_t key_tag;   /* EQ, CONTAINS */
    uint32_t reserved;  /* 0 */
    uint64_t key;       /* EQ, CONTAINS: the payload; NUM_RANGE: the normalised bits of the literal */
    uint64_t aux_off;   /* KEYSET, STRTABLE: offset of the leaf's data in `aux`, in u64 words */
    uint64_t aux_len;   /* KEYSET: keys; STRTABLE: codes the table covers */
} lynse_hip_field_leaf;
typedef struct lynse_hip_fields lynse_hip_fields;
int lynse_hip_fields_create(int device, lynse_hip_fields **out);
int lynse_hip_fields_destroy(lynse_hip_fields *h);
int lynse_hip_fields_set_column(lynse_hip_fields *h, uint32_t column, const uint8_t *tags /* n */, const uint64_t *payloads /* n */,
                                uint64_t n, const uint64_t *arr_ptr /* n_arrays+1, NULL without arrays */, uint64_t n_arrays,
                                const uint8_t *elem_tags, const uint64_t *elem_payloads);
int lynse_hip_fields_drop_column(lynse_hip_fields *h, uint32_t column);
int lynse_hip_fields_column_rows(lynse_hip_fields *h, uint32_t column, uint64_t *out_rows /* 0 = not set */);
uint64_t lynse_hip_fields_hbm_bytes(lynse_hip_fields *h);
int lynse_hip_fields_filter(lynse_hip_fields *h, uint64_t n, int combine, const lynse_hip_field_leaf *leaves, uint32_t n_leaves,
                            const uint64_t *aux, uint64_t aux_words, uint64_t *out_count, float *out_kernel_us /* may be NULL */);
int lynse_hip_fields_words(lynse_hip_fields *h, uint64_t *out_words, uint64_t n_words);
int lynse_hip_fields_words_device(lynse_hip_fields *h, const uint64_t **out_d_words, uint64_t *out_n_words);

/* ---- named vector fields: create_vector_field / add_named_vectors / search_vector_field (src/engine.rs:4042-4420, :4836-4960) ---- */

/* NAMED VECTOR FIELDS.  A named field is a further vector per record with its own dimension, metric and dtype; its shard is an
 * ordinary lynse_hip_flat handle (the caller owns it and the field row -> user id map).  A field's rows are a SUBSET of the
 * collection's rows in ANOTHER ORDER, so a filter over collection rows (lynse_hip_fields_filter's BitSet words, or a caller's subset)
 * has to be renumbered before the field's filtered scan can take it.  The reference ranks every row of the field and drops the
 * disallowed ones on the host (search_k = id_map.len(), :4881-4947); here one kernel (k_bitset_remap) rewrites the words on the device
 * and lynse_hip_flat_search_filtered_bitset_device_f32 takes them without a round trip.  The rules:
 *  1. lynse_hip_rowmap_set uploads row_of (u32[n_out], n_out < 2^32 - 1) WHOLE: field row r belongs to collection row row_of[r];
 *     LYNSE_ROWMAP_NONE (0xffffffff) = to none.  It replaces the earlier map and drops the words of an earlier remap.  The host keeps
 *     1 + the largest entry that is not NONE (lynse_hip_rowmap_len reports it with n_out).
 *  2. lynse_hip_rowmap_remap takes the source mask in two parts: `src_words` covering n_src bits (the flushed collection rows; a
 *     pointer into this device's memory when src_on_device != 0, e.g. what lynse_hip_fields_words_device returns, else host memory,
 *     which is uploaded) and optionally `tail_words` in host memory covering n_tail bits (the pending collection rows: the caller
 *     evaluates those itself), numbered n_src .. n_src + n_tail - 1.  Output bit r = source bit row_of[r]; NONE gives 0.  It leaves
 *     ceil(n_out / 64) BitSet words in the handle's device memory (bit r of word r / 64, LSB first; bits at and beyond n_out are
 *     zero), *out_count = the set bits (one 8-byte read-back), *out_kernel_us (may be NULL) = the kernel's duration between two HIP
 *     events.  n_out == 0: no launch, no words, count 0.
 *  3. Checked on the host before anything is uploaded or launched (LYNSE_ERR_INVALID_ARGUMENT, nothing launched, the handle still
 *     usable): a map has been set; n_src_words == ceil(n_src / 64) and n_tail_words == ceil(n_tail / 64); n_src + n_tail < 2^32;
 *     every row_of entry is NONE or < n_src + n_tail.  A device `src_words` must hold n_src_words words: that is the caller's
 *     contract, as for lynse_hip_flat_search_filtered_bitset_device_f32.
 *  4. lynse_hip_rowmap_words reads the words back; lynse_hip_rowmap_words_device gives the device pointer (valid until the next
 *     set, remap or destroy on this handle).  When row_of is the identity over n_out == n_src rows and there is no tail, the
 *     remapped words ARE the source words: callers may skip the remap and hand the source words on (lynsedb_amd does).
 *  5. The calls of one handle are serialised by the handle's lock.  The kernel uses vector stores and vector atomics only, no LDS.
 * Without a usable HIP device lynse_hip_rowmap_create returns LYNSE_ERR_DEVICE: there is no CPU fallback. */
#define LYNSE_ROWMAP_NONE 0xffffffffu
typedef struct lynse_hip_rowmap lynse_hip_rowmap;
int lynse_hip_rowmap_create(int device, lynse_hip_rowmap **out);
int lynse_hip_rowmap_destroy(lynse_hip_rowmap *h);
int lynse_hip_rowmap_set(lynse_hip_rowmap *h, const uint32_t *row_of /* n_out */, uint64_t n_out);
int lynse_hip_rowmap_len(lynse_hip_rowmap *h, uint64_t *out_rows, uint64_t *out_bound /* 1 + the largest entry, 0 without one */);
uint64_t lynse_hip_rowmap_hbm_bytes(lynse_hip_rowmap *h);
int lynse_hip_rowmap_remap(lynse_hip_rowmap *h, const uint64_t *src_words, uint64_t n_src_words, uint64_t n_src, int src_on_device,
                           const uint64_t *tail_words /* host; NULL when n_tail == 0 */, uint64_t n_tail_words, uint64_t n_tail,
                           uint64_t *out_count, float *out_kernel_us /* may be NULL */);
int lynse_hip_rowmap_words(lynse_hip_rowmap *h, uint64_t *out_words, uint64_t n_words);
int lynse_hip_rowmap_words_device(lynse_hip_rowmap *h, const uint64_t **out_d_words, uint64_t *out_n_words);

/* ---- shard-node glue around a search (host only, no device work) ---- */

/* Collection::filter_tombstoned_limit (src/engine.rs:3286-3308): drop the tombstoned ids, keep the order, at most
 * `limit` pairs.  Outputs hold min(n, limit) entries. */
int lynse_hip_filter_tombstoned_limit(const uint64_t *ids, const float *dists, uint64_t n,
                                      const uint64_t *tombstones, uint64_t n_tombstones, uint64_t limit,
                                      uint64_t *out_ids, float *out_dists, uint64_t *out_n);
/* Collection::merge_row_results (src/engine.rs:3363-3418): flushed + pending rows.  Duplicate ids keep the better
 * distance; order (distance in metric order, id); truncated to `limit` — except that an empty side returns the other
 * side untouched, as the reference does.  Outputs hold n_left + n_right entries. */
int lynse_hip_merge_row_results(const uint64_t *left_ids, const float *left_dists, uint64_t n_left,
                                const uint64_t *right_ids, const float *right_dists, uint64_t n_right,
                                uint64_t limit, int metric, uint64_t *out_ids, float *out_dists,
                                uint64_t *out_n);
/* encode_search_result_binary (src/rpc.rs:1156-1177): [u32 n][n x u64 id][n x f32 distance][u32 fields_len][fields
 * JSON], little endian — the block a shard returns to the coordinator.  *out_len = bytes needed / written. */
int lynse_hip_encode_search_result(const uint64_t *ids, const float *dists, uint32_t n,
                                   const uint8_t *fields_json, uint32_t fields_len, uint8_t *buf,
                                   uint64_t cap, uint64_t *out_len);
/* decode_search_result_binary (src/cluster.rs:404-435) at `offset` of a frame that may hold several blocks. */
int lynse_hip_decode_search_result(const uint8_t *buf, uint64_t len, uint64_t offset, uint64_t *out_ids,
                                   float *out_dists, uint32_t cap_n, uint32_t *out_n,
                                   uint64_t *fields_offset, uint32_t *fields_len, uint64_t *next_offset);

#ifdef __cplusplus
}
#endif
#endif /* LYNSE_HIP_H */
