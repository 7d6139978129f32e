// sparse.h — sparse-vector search (SparseVectorStore::search, src/engine.rs:660-695; sparse_inner_product, :6945-6965): a flat scan
// of the CSR rows against a tile of queries held in LDS.  The cut and the order are the range search's (k_pq_hist / k_pq_find /
// k_pq_emit of pq.h, k_pool_select of kernels.h).  DESIGN.md §18.
//   k_sparse_scan   a group of SPARSE_G lanes owns a row and walks its index stream SPARSE_G entries a step; an entry is looked up in
//                   the tile's prefilter bitmap, then in its open-addressing table; the hits of a step are taken lowest lane first, so
//                   every query's sum runs in ascending index order with separate f32 multiplies and adds, as the two-pointer merge does
// It writes S[q][row] = the score_ord image (descending) of a score != 0 — a NaN score passes that test and goes in as -inf —,
// RANGE_FAIL for a row that scores 0, has no common index or is masked out, and adds the passers of a query to count[q].
#pragma once

#include "range.h"

namespace lynse {

constexpr int SPARSE_NT = 256;            // 16 groups of 16 lanes
constexpr uint32_t SPARSE_G = 16;         // lanes of a row group: fixed (a row of ~120 entries takes 8 steps); lane j < TQ sums query j
constexpr uint32_t SPARSE_MAX_Q = 16;     // queries of a tile (<= SPARSE_G: one lane per query)
constexpr uint32_t SPARSE_ROWS = 128;     // rows of a tile: the [TQ][rows] images staged in LDS
constexpr uint32_t SPARSE_PRE_BITS = 15;  // prefilter: one bit per index & (2^15 - 1), 4 KiB
constexpr uint32_t SPARSE_PRE_WORDS = (1u << SPARSE_PRE_BITS) / 32u;
constexpr uint32_t SPARSE_MAX_NNZ = 4096; // entries of one query: its table of 8,192 slots is the largest that fits the 160 KiB

// the home slot of an index in a table of 2^bits slots (Fibonacci hashing; host and device)
__host__ __device__ inline uint32_t sparse_slot(uint32_t index, uint32_t bits) { return (index * 2654435761u) >> (32u - bits); }

// The table of one query tile, as it lies in global memory (built on the host) and in LDS, in 32-bit words:
//   keys[H] | vidx[H] | vals[U][TQ] | bitmap[SPARSE_PRE_WORDS]
// vidx = 0: the slot is empty (every u32 is a legal index, so emptiness is not a key value); else 1 + the entry of vals that holds
// the TQ query values of the index, 0.0f where a query lacks it.  At most half the slots are taken, so a probe ends.
struct SparseScanArgs {
    const uint64_t* indptr;   // n + 1
    const uint32_t* indices;  // ascending within a row
    const float* values;      // finite, non-zero
    uint64_t n;
    const uint32_t* tables;   // one table per query tile, `tab_words` apart
    uint32_t tab_words, H, hbits, U, TQ;
    uint32_t nq;
    const uint64_t* mask;     // NULL = every row
    uint64_t mask_words;
    uint32_t* S;              // [nq][n]
    uint32_t* count;          // [nq], zeroed by the caller
};

// LDS: the table | stage[TQ][SPARSE_ROWS] | cnt[TQ]
__global__ void __launch_bounds__(SPARSE_NT) k_sparse_scan(SparseScanArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t sm_sparse[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, g = tid & (SPARSE_G - 1u), grp = tid / SPARSE_G;
    const uint32_t gbase = lane & ~(SPARSE_G - 1u);   // the group's first lane in its wave
    const uint32_t q0 = blockIdx.y * a.TQ;
    const uint32_t tq = a.nq - q0 < a.TQ ? a.nq - q0 : a.TQ;
    uint32_t* keys_l = sm_sparse;
    uint32_t* vidx_l = keys_l + a.H;
    const float* vals_l = reinterpret_cast<const float*>(vidx_l + a.H);
    const uint32_t* pre_l = vidx_l + a.H + (size_t)a.U * a.TQ;
    uint32_t* stage_l = sm_sparse + a.tab_words;
    uint32_t* cnt_l = stage_l + (size_t)a.TQ * SPARSE_ROWS;
    const uint32_t* tab = a.tables + (size_t)blockIdx.y * a.tab_words;
    for (uint32_t i = tid; i < a.tab_words; i += SPARSE_NT) sm_sparse[i] = tab[i];
    if (tid < a.TQ) cnt_l[tid] = 0u;
    const uint32_t hmask = a.H - 1u;
    const uint64_t tiles = (a.n + SPARSE_ROWS - 1) / SPARSE_ROWS;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint64_t r0 = t * SPARSE_ROWS;
        const uint32_t rn = a.n - r0 < SPARSE_ROWS ? (uint32_t)(a.n - r0) : SPARSE_ROWS;
        __syncthreads();   // the previous tile's images are stored (first trip: the table is staged)
        // every branch below depends on the row alone, so the 16 lanes of a group stay together and a shuffle inside the group
        // reads live lanes; the other groups of the wave may be anywhere else
        for (uint32_t rr = grp; rr < SPARSE_ROWS; rr += SPARSE_NT / SPARSE_G) {
            float acc = 0.0f;
            if (rr < rn && range_live(a.mask, a.mask_words, r0 + rr)) {   // a masked-out row skips the arithmetic
                const uint64_t e1 = a.indptr[r0 + rr + 1];
                for (uint64_t e = a.indptr[r0 + rr]; e < e1; e += SPARSE_G) {
                    const uint64_t p = e + g;
                    uint32_t vi = 0u;
                    if (p < e1) {
                        const uint32_t idx = a.indices[p];
                        const uint32_t b = idx & ((1u << SPARSE_PRE_BITS) - 1u);
                        if ((pre_l[b >> 5] >> (b & 31u)) & 1u) {
                            uint32_t s = sparse_slot(idx, a.hbits);
                            for (uint32_t probe = 0; probe < a.H; ++probe) {   // (ends at an empty slot: half the slots are)
                                vi = vidx_l[s];
                                if (vi == 0u || keys_l[s] == idx) break;
                                vi = 0u;
                                s = (s + 1u) & hmask;
                            }
                        }
                    }
                    uint32_t hits = (uint32_t)(__ballot(vi != 0u) >> gbase) & ((1u << SPARSE_G) - 1u);
                    if (hits) {
                        const float v = vi ? a.values[p] : 0.0f;   // the value stream is read for hits only
                        // Lane j adds the product for query j whether or not that query holds the index: an absent query value is
                        // 0.0f and the stored value is finite, so the product is +-0; the sum starts at +0 and round-to-nearest never
                        // makes it -0 (x + -x = +0, +0 + -0 = +0), and s + +-0 == s bit for bit for every other s (inf and NaN
                        // included).  No mask is needed.
                        while (hits) {
                            const int l = __ffs(hits) - 1;
                            hits &= hits - 1u;
                            const uint32_t hv = __shfl(vi, l, SPARSE_G);
                            const float rv = __shfl(v, l, SPARSE_G);
                            if (g < a.TQ) acc = __fadd_rn(acc, __fmul_rn(vals_l[(size_t)(hv - 1u) * a.TQ + g], rv));
                        }
                    }
                }
            }
            if (g < a.TQ) stage_l[g * SPARSE_ROWS + rr] = acc != 0.0f ? score_ord(acc, false) : RANGE_FAIL;   // (NaN != 0: kept)
        }
        __syncthreads();
        // the images go out a query's 128 rows at a time; a wave holds 64 rows of ONE query, so its ballot counts that query's passers
        for (uint32_t i = tid; i < tq * SPARSE_ROWS; i += SPARSE_NT) {
            const uint32_t j = i / SPARSE_ROWS, r = i % SPARSE_ROWS;
            const uint32_t img = stage_l[i];
            const bool in = r < rn;
            if (in) a.S[(size_t)(q0 + j) * a.n + r0 + r] = img;
            const uint64_t b = __ballot(in && img != RANGE_FAIL);
            if (lane == 0 && b) atomicAdd(&cnt_l[j], (uint32_t)__popcll(b));
        }
    }
    __syncthreads();
    if (tid < tq && cnt_l[tid]) atomicAdd(&a.count[q0 + tid], cnt_l[tid]);
}

}  // namespace lynse
