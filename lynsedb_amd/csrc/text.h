// text.h — BM25 text search (InvertedTextIndex::search, src/engine.rs:927-1054): a term-at-a-time scan of the posting lists of the
// query's terms over owned row ranges.  The cut and the order are the range search's (k_pq_hist / k_pq_find / k_pq_emit of pq.h,
// k_pool_select of kernels.h).  include/lynse_hip.h TEXT SEARCH, DESIGN.md §20.
//   k_text_stats   under a mask only: the live rows and the sum of their lengths, and the live postings of every (query, slot)
//   k_text_scan    a workgroup owns TEXT_ROWS consecutive rows and keeps their sums and candidate bits in LDS; it walks the slots of
//                  its query in slot order with a barrier between two slots, the lanes striding over the slot's postings that fall in
//                  the tile.  A row occurs at most once in a posting list, so no two lanes of a slot touch the same sum and every
//                  row's sum runs in slot order with separate f32 multiplies, divides and adds (rule f).
//                  doc_len is gathered per posting (the gather stays in the tile's 16 KiB window), not loaded per tile.
// It writes S[q][row] = the score_ord image (descending) of a score > 0 of a row that holds a candidate term, RANGE_FAIL for every
// other row, and adds the passers of a query to count[q].
#pragma once

#include "range.h"

namespace lynse {

constexpr int TEXT_NT = 256;
constexpr uint32_t TEXT_ROWS = 4096;        // rows of a tile: 16 KiB of sums + 512 B of candidate bits in LDS
constexpr uint32_t TEXT_MAX_TERMS = 256;    // distinct known terms of a query (rule h): one lane per slot in the prologue
constexpr uint32_t TEXT_STATS_PARTS = 8;    // workgroups that share the postings of one slot in k_text_stats

// One slot of a query, as the host builds it: the posting range of its term and what rules d and e made of it.
struct TextSlot {
    uint64_t p0, p1;   // postings [p0, p1) of the term; empty for the scan when the term has no live posting (rule c)
    float w;           // count * idf (rule e)
    uint32_t cand;     // 1 = a candidate term (rule d)
};

struct TextScanArgs {
    const uint32_t* post_row;   // ascending within a term
    const uint32_t* post_tf;
    const uint32_t* doc_len;    // n
    uint64_t n;
    const TextSlot* slots;      // the slots of every query of the chunk, query after query
    const uint64_t* slot_ptr;   // nq + 1
    const float* avg;           // [nq] rule b (one value per query: a chunk shares its mask, the layout leaves room for more)
    uint32_t nq;
    const uint64_t* mask;       // NULL = every row
    uint64_t mask_words;
    uint32_t* S;                // [nq][n]
    uint32_t* count;            // [nq], zeroed by the caller
};

// the first posting of [lo, hi) whose row is >= row
__device__ __forceinline__ uint64_t text_lower_bound(const uint32_t* __restrict__ post_row, uint64_t lo, uint64_t hi, uint64_t row) {
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if ((uint64_t)post_row[mid] < row) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(TEXT_NT) k_text_scan(TextScanArgs a) {
    __shared__ float acc_l[TEXT_ROWS];
    __shared__ uint32_t cand_l[TEXT_ROWS / 32];
    __shared__ uint64_t lo_l[TEXT_MAX_TERMS], hi_l[TEXT_MAX_TERMS];
    __shared__ float w_l[TEXT_MAX_TERMS];
    __shared__ uint32_t flag_l[TEXT_MAX_TERMS];
    __shared__ uint32_t cnt_l;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, q = blockIdx.y;
    const uint64_t base = (uint64_t)blockIdx.x * TEXT_ROWS;
    const uint32_t rn = a.n - base < TEXT_ROWS ? (uint32_t)(a.n - base) : TEXT_ROWS;
    const uint64_t s0 = a.slot_ptr[q];
    const uint32_t T = (uint32_t)(a.slot_ptr[q + 1] - s0);   // <= TEXT_MAX_TERMS (the host refuses more)
    // prologue: one lane per slot finds the slot's postings inside the tile, so the T binary searches run side by side
    if (tid < T) {
        const TextSlot s = a.slots[s0 + tid];
        const uint64_t lo = text_lower_bound(a.post_row, s.p0, s.p1, base);   // (a term with no live posting comes with p0 == p1)
        lo_l[tid] = lo;
        hi_l[tid] = text_lower_bound(a.post_row, lo, s.p1, base + rn);
        w_l[tid] = s.w;
        flag_l[tid] = s.cand;
    }
    for (uint32_t i = tid; i < TEXT_ROWS; i += TEXT_NT) acc_l[i] = 0.0f;
    if (tid < TEXT_ROWS / 32) cand_l[tid] = 0u;
    if (tid == 0) cnt_l = 0u;
    const float avg = a.avg[q];
    const float K = 1.2f + 1.0f;
    __syncthreads();
    for (uint32_t s = 0; s < T; ++s) {
        const uint64_t hi = hi_l[s];
        const float w = w_l[s];
        const uint32_t cand = flag_l[s];
        for (uint64_t p = lo_l[s] + tid; p < hi; p += TEXT_NT) {
            const uint32_t row = a.post_row[p];
            if (!range_live(a.mask, a.mask_words, row)) continue;
            const float tf = (float)a.post_tf[p], dl = (float)a.doc_len[row];
            // rule f: (w * (tf * K)) / (tf + 1.2f * (0.25f + (0.75f * dl) / avg))
            const float den = __fadd_rn(tf, __fmul_rn(1.2f, __fadd_rn(0.25f, __fdiv_rn(__fmul_rn(0.75f, dl), avg))));
            const float term = __fdiv_rn(__fmul_rn(w, __fmul_rn(tf, K)), den);
            const uint32_t r = (uint32_t)(row - base);   // < rn: the sub-range lies in the tile
            acc_l[r] = __fadd_rn(acc_l[r], term);
            if (cand) atomicOr(&cand_l[r >> 5], 1u << (r & 31u));
        }
        __syncthreads();   // the next slot adds to the same sums: slot order is the order of every row's sum
    }
    // epilogue: coalesced images, the passers counted by ballot (whole waves make every trip)
    uint32_t mine = 0;
    for (uint32_t r0 = 0; r0 < rn; r0 += TEXT_NT) {
        const uint32_t r = r0 + tid;
        const bool in = r < rn;
        const float sc = in ? acc_l[r] : 0.0f;
        const bool pass = in && ((cand_l[r >> 5] >> (r & 31u)) & 1u) && sc > 0.0f;
        if (in) a.S[(size_t)q * a.n + base + r] = pass ? score_ord(sc, false) : RANGE_FAIL;
        const uint64_t b = __ballot(pass);
        if (lane == 0) mine += (uint32_t)__popcll(b);
    }
    if (lane == 0 && mine) atomicAdd(&cnt_l, mine);
    __syncthreads();
    if (tid == 0 && cnt_l) atomicAdd(&a.count[q], cnt_l);
}

struct TextStatsArgs {
    const uint32_t* post_row;
    const uint32_t* doc_len;
    uint64_t n;
    const TextSlot* slots;      // n_slots slots (of every query of the chunk); only p0 and p1 are read
    uint64_t n_slots;
    uint32_t row_blocks;        // the first row_blocks workgroups count rows, the rest postings (0: the corpus totals are not wanted)
    const uint64_t* mask;       // never NULL here
    uint64_t mask_words;
    unsigned long long* corpus;   // [2]: live rows, the sum of their lengths; zeroed by the caller
    unsigned long long* df;       // [n_slots], zeroed by the caller
};

// the wave's sum of v in lane 0
__device__ __forceinline__ unsigned long long text_wave_sum(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

__global__ void __launch_bounds__(TEXT_NT) k_text_stats(TextStatsArgs a) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    if (blockIdx.x < a.row_blocks) {
        unsigned long long docs = 0, total = 0;
        for (uint64_t r = (uint64_t)blockIdx.x * TEXT_NT + tid; r < a.n; r += (uint64_t)a.row_blocks * TEXT_NT)
            if (range_live(a.mask, a.mask_words, r)) {
                docs += 1;
                total += a.doc_len[r];
            }
        docs = text_wave_sum(docs);
        total = text_wave_sum(total);
        if (lane == 0 && docs) {
            atomicAdd(&a.corpus[0], docs);
            atomicAdd(&a.corpus[1], total);
        }
        return;
    }
    const uint64_t b = blockIdx.x - a.row_blocks;
    const uint64_t s = b / TEXT_STATS_PARTS;
    const uint32_t part = (uint32_t)(b % TEXT_STATS_PARTS);
    if (s >= a.n_slots) return;
    const uint64_t p1 = a.slots[s].p1;
    unsigned long long df = 0;
    for (uint64_t p = a.slots[s].p0 + (uint64_t)part * TEXT_NT + tid; p < p1; p += (uint64_t)TEXT_STATS_PARTS * TEXT_NT)
        if (range_live(a.mask, a.mask_words, a.post_row[p])) df += 1;
    df = text_wave_sum(df);
    if (lane == 0 && df) atomicAdd(&a.df[s], df);
}

}  // namespace lynse
