// range.h — range search (Collection::search_range, src/engine.rs:6410-6483): every row of the shard scored with the single-row
// kernels (compute_distance_f32), the rows on the passing side of a caller-given threshold kept.  The cut at max_results is the
// radix selection of pq.h (k_pq_hist / k_pq_find / k_pq_emit), the order the LDS sort of k_pool_select (kernels.h).  DESIGN.md §16.
//   k_range_scan      f32 / f16 rows: a tile of rows goes through LDS with 16-B loads (an F16 shard is decoded there, exactly), a
//                     tile of queries sits next to it, exact_score in its single-row form (ids 7-10: additive_score) for every (query, row) of the tiles
//   k_range_scan_bin  packed rows: the popcount distances of k_scan_binary_wide (binary_distance)
// Both write S[q][row] = the score_ord image of a passing distance, RANGE_FAIL for a row that fails the test, is masked out or
// scores NaN, and add the passers of a query to count[q]: ballot + popcount in the wave, LDS across the block, one device atomic
// per block and query.
#pragma once

#include "pq.h"

namespace lynse {

// No passing distance has this image: ascending it is the image of the NaN 0x7fffffff, descending of the NaN 0xffffffff, and a
// NaN never passes.  It is the largest image, so the radix selection ranks such rows behind every passer.
constexpr uint32_t RANGE_FAIL = 0xffffffffu;

constexpr int RANGE_NT = 256;           // 32 groups of 8 lanes, one row per group and trip
constexpr uint32_t RANGE_MAX_ROWS = 128;   // rows of an LDS tile
constexpr uint32_t RANGE_MAX_Q = 16;       // queries of an LDS tile

// the pass test of search_range (:6446-6450), plain IEEE comparisons: a NaN distance or threshold passes nothing
__device__ __forceinline__ bool range_pass(float d, float thr, bool asc) { return asc ? d <= thr : d >= thr; }

// bit r of word r / 64 (src/storage/bitset.rs:15-24); rows the words do not cover are out
__device__ __forceinline__ bool range_live(const uint64_t* __restrict__ mask, uint64_t mask_words, uint64_t row) {
    if (!mask) return true;
    const uint64_t w = row >> 6;
    return w < mask_words && ((mask[w] >> (row & 63u)) & 1ull);
}

// ids 7-10 (additive.h, included after this file): one (query, row) pair by the 8 lanes of a group, as exact_score
template <int UB = 8>
__device__ __forceinline__ float additive_score(int metric, const float* __restrict__ q, const float* __restrict__ v, uint32_t D, int g);

struct RangeScanArgs {
    const void* V;          // n rows: f32 (pitch ld floats, ld % 4 == 0) or the f16 bits of an F16 shard (pitch ld halves, ld % 8 == 0)
    uint32_t ld, D;
    int f16;
    uint64_t n;
    const float* Q;         // nq x D
    const float* thr;       // nq
    uint32_t nq;
    int metric;
    const uint64_t* mask;   // NULL = every row
    uint64_t mask_words;
    uint32_t R, TQ;         // rows / queries of an LDS tile
    uint32_t stride;        // LDS row stride in floats (a multiple of 4, >= round_up(D, 4))
    uint32_t* S;            // [nq][n]
    uint32_t* count;        // [nq], zeroed by the caller
};

// LDS: TQ queries of D floats (padded to 16 B) | R rows of `stride` floats | TQ thresholds | TQ counts
__global__ void __launch_bounds__(RANGE_NT) k_range_scan(RangeScanArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm_range[];
    const uint32_t tid = threadIdx.x, grp = tid >> 3, lane = tid & 63u;
    const int g = tid & 7;
    const uint32_t q0 = blockIdx.y * a.TQ;
    const uint32_t tq = a.nq - q0 < a.TQ ? a.nq - q0 : a.TQ;
    const uint32_t q_floats = (a.TQ * a.D + 3u) / 4u * 4u;
    float* q_l = sm_range;
    float* rows_l = sm_range + q_floats;
    float* thr_l = rows_l + (size_t)a.R * a.stride;
    uint32_t* cnt_l = reinterpret_cast<uint32_t*>(thr_l + a.TQ);
    for (uint32_t i = tid; i < tq * a.D; i += RANGE_NT) q_l[i] = a.Q[(size_t)q0 * a.D + i];
    if (tid < a.TQ) {
        thr_l[tid] = tid < tq ? a.thr[q0 + tid] : 0.0f;
        cnt_l[tid] = 0u;
    }
    const bool asc = metric_ascending(a.metric);
    const uint32_t vpr = a.f16 ? (a.D + 7u) / 8u : (a.D + 3u) / 4u;   // 16-B pieces of a row
    const uint64_t tiles = (a.n + a.R - 1) / a.R;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint64_t r0 = t * a.R;
        const uint32_t rn = a.n - r0 < a.R ? (uint32_t)(a.n - r0) : a.R;
        __syncthreads();   // the previous tile has been scored (first trip: the queries are staged)
        if (a.f16) {
            const _Float16* V = reinterpret_cast<const _Float16*>(a.V);
            for (uint32_t p = tid; p < rn * vpr; p += RANGE_NT) {
                const uint32_t r = p / vpr, c = p - r * vpr;
                const half8 h = *reinterpret_cast<const half8*>(V + (r0 + r) * a.ld + (size_t)c * 8u);
                f32x4 lo, hi;
#pragma unroll
                for (int e = 0; e < 4; ++e) { lo[e] = (float)h[e]; hi[e] = (float)h[e + 4]; }   // (f16 -> f32 is exact)
                float* dst = rows_l + (size_t)r * a.stride + (size_t)c * 8u;
                *reinterpret_cast<f32x4*>(dst) = lo;
                *reinterpret_cast<f32x4*>(dst + 4) = hi;
            }
        } else {
            const float* V = reinterpret_cast<const float*>(a.V);
            for (uint32_t p = tid; p < rn * vpr; p += RANGE_NT) {
                const uint32_t r = p / vpr, c = p - r * vpr;
                *reinterpret_cast<f32x4*>(rows_l + (size_t)r * a.stride + (size_t)c * 4u) =
                    *reinterpret_cast<const f32x4*>(V + (r0 + r) * a.ld + (size_t)c * 4u);
            }
        }
        __syncthreads();
        const uint32_t bound = (rn + 31u) / 32u * 32u;   // whole waves run the same trip count (exact_score shuffles inside its 8 lanes)
        for (uint32_t rr = grp; rr < bound; rr += 32u) {
            const bool in = rr < rn;
            const uint64_t row = r0 + (in ? rr : 0u);   // a group past the end re-scores row 0 of the tile and drops it
            const float* v = rows_l + (size_t)(in ? rr : 0u) * a.stride;
            const bool live = in && range_live(a.mask, a.mask_words, row);
            for (uint32_t j = 0; j < tq; ++j) {
                const float d = metric_additive(a.metric) ? additive_score<16>(a.metric, q_l + (size_t)j * a.D, v, a.D, g)
                                                          : exact_score<16>(a.metric, LYNSE_IPFORM_SINGLE, q_l + (size_t)j * a.D, v, a.D, g);
                const bool pass = live && g == 0 && range_pass(d, thr_l[j], asc);
                if (in && g == 0) a.S[(size_t)(q0 + j) * a.n + row] = pass ? score_ord(d, asc) : RANGE_FAIL;
                const uint64_t b = __ballot(pass);
                if (lane == 0 && b) atomicAdd(&cnt_l[j], (uint32_t)__popcll(b));
            }
        }
    }
    __syncthreads();
    if (tid < tq && cnt_l[tid]) atomicAdd(&a.count[q0 + tid], cnt_l[tid]);
}

struct RangeBinArgs {
    const uint64_t* P;      // n x W packed rows
    uint32_t W;
    uint64_t n;
    const uint64_t* QW;     // nq x W packed queries
    const float* thr;
    uint32_t nq;
    const uint64_t* mask;
    uint64_t mask_words;
    uint32_t* S;
    uint32_t* count;
};

// Eight lanes own one row and walk its words with stride 8, as k_scan_binary_wide does (any width); every metric is ascending.
template <int KIND>  // 0 hamming, 1 jaccard/tanimoto, 2 dice
__global__ void __launch_bounds__(RANGE_NT) k_range_scan_bin(RangeBinArgs a) {
    __shared__ uint32_t cnt_l[RANGE_MAX_Q];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const int g = tid & 7;
    const uint32_t q0 = blockIdx.y * RANGE_MAX_Q;
    const uint32_t tq = a.nq - q0 < RANGE_MAX_Q ? a.nq - q0 : RANGE_MAX_Q;
    if (tid < RANGE_MAX_Q) cnt_l[tid] = 0u;
    __syncthreads();
    const uint64_t tiles = (a.n + 31) / 32;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint64_t row = t * 32 + (tid >> 3);
        const bool in = row < a.n;
        const bool live = in && range_live(a.mask, a.mask_words, row);
        const uint64_t* rp = a.P + (in ? row : 0) * a.W;
        uint32_t popr = 0;
        if (KIND == 2)
            for (uint32_t w = g; w < a.W; w += 8) popr += __popcll(rp[w]);
        for (uint32_t j = 0; j < tq; ++j) {
            const uint64_t* qp = a.QW + (size_t)(q0 + j) * a.W;
            uint32_t c0 = 0, c1 = 0;
            for (uint32_t w = g; w < a.W; w += 8) {
                const uint64_t x = qp[w], r = rp[w];
                if (KIND == 0) {
                    c0 += __popcll(x ^ r);
                } else if (KIND == 1) {
                    c0 += __popcll(x & r);
                    c1 += __popcll(x | r);
                } else {
                    c0 += __popcll(x & r);
                    c1 += __popcll(x);
                }
            }
            if (KIND == 2) c1 += popr;
            c0 += __shfl_xor(c0, 1, 8);
            c0 += __shfl_xor(c0, 2, 8);
            c0 += __shfl_xor(c0, 4, 8);
            if (KIND != 0) {
                c1 += __shfl_xor(c1, 1, 8);
                c1 += __shfl_xor(c1, 2, 8);
                c1 += __shfl_xor(c1, 4, 8);
            }
            const float d = binary_distance<KIND>(c0, c1);
            const bool pass = live && g == 0 && range_pass(d, a.thr[q0 + j], true);
            if (in && g == 0) a.S[(size_t)(q0 + j) * a.n + row] = pass ? score_ord(d, true) : RANGE_FAIL;
            const uint64_t b = __ballot(pass);
            if (lane == 0 && b) atomicAdd(&cnt_l[j], (uint32_t)__popcll(b));
        }
    }
    __syncthreads();
    if (tid < tq && cnt_l[tid]) atomicAdd(&a.count[q0 + tid], cnt_l[tid]);
}

}  // namespace lynse
