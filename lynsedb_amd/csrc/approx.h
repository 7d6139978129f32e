// approx.h — the approximate flat search (Collection.search(approx=True, eps=...); the reference's FlatMmap::search approx branch,
// src/storage/flat_mmap.rs:847-889, and src/storage/approx_search.rs).  Nothing is quantised: the coarse pass reads fewer bytes of the
// f32 rows (a few contiguous blocks of each row's dimensions) or none at all (a cached order of the rows by their sums), a pool of the
// best coarse rows is rescored exactly.  The contract block next to the additive one in include/lynse_hip.h states the four paths;
// DESIGN.md §27.
//   k_approx_rowstats   one pass over the shard: row_sum (row_sum_avx2's order), norm2 (the single-row IP form of the row with itself)
//                       and inv_norm per row, and the number of rows whose sum is finite
//   k_approx_sum_keys   the score image of the row sums for the cut of the sum order (a non-finite sum: RANGE_FAIL, never taken)
//   k_approx_coarse     one query, every row, one f32 per row as its score_ord image: the block forms read ONLY the sampled blocks
//   k_approx_rescore    the pool scored exactly (single-row IP form, or additive_score) into keys for k_pool_select / the host selection
// The tie rule where the reference leaves one open (select_nth_unstable_by on the score alone, per-thread merges): the pool is the best
// `pool` rows by the canonical key (coarse score in metric order, row ascending); a NaN coarse score orders last, with the worst
// infinity (make_key), and -0.0 is +0.0.
//
// Layout: an 8-lane group per row straight from HBM (as exact_score / additive_score, whose accumulation orders the forms are made
// of); the query's sampled elements sit in LDS, block after block.  DESIGN.md §27.3 says why not the lane-major LDS image of
// k_additive_scan.
#pragma once

#include "additive.h"

namespace lynse {

enum : int { AF_IP = 0, AF_L2EXP = 1, AF_COSEXP = 2, AF_L1 = 3, AF_CHEBYSHEV = 4, AF_CANBERRA = 5, AF_BRAY_CURTIS = 6 };
constexpr int APX_NT = 256;   // 32 groups of 8 lanes, one row per group and trip

struct ApproxBlocks {   // sampled_dim_blocks: up to three contiguous blocks of a row's dimensions, in order
    uint32_t nb;
    uint32_t start[3], len[3];
};

struct ApproxStatsArgs {
    const float* V;
    uint32_t ld, D;
    uint64_t n;
    float *row_sum, *norm2, *inv_norm;
    unsigned long long* finite;   // += rows with a finite sum
};

__global__ void __launch_bounds__(APX_NT) k_approx_rowstats(ApproxStatsArgs a) {
    const uint32_t tid = threadIdx.x;
    const int g = tid & 7;
    const uint64_t bound = (a.n + 31u) / 32u * 32u;   // whole workgroups run the same trip count (shuffles inside the 8 lanes)
    const uint32_t chunks32 = a.D / 32u;
    for (uint64_t r = (uint64_t)blockIdx.x * 32u + (tid >> 3); r < bound; r += (uint64_t)gridDim.x * 32u) {
        const uint64_t row = r < a.n ? r : a.n - 1;
        const float* v = a.V + row * a.ld;
        // row_sum_avx2: four 8-lane accumulators over chunks of 32, (acc0 + acc1) + (acc2 + acc3), the lanes 0 -> 7, then the tail
        float acc0 = 0.0f, acc1 = 0.0f, acc2 = 0.0f, acc3 = 0.0f;
        for (uint32_t c = 0; c < chunks32; ++c) {
            const float x0 = v[c * 32u + g], x1 = v[c * 32u + 8u + g], x2 = v[c * 32u + 16u + g], x3 = v[c * 32u + 24u + g];
            acc0 = __fadd_rn(acc0, x0);
            acc1 = __fadd_rn(acc1, x1);
            acc2 = __fadd_rn(acc2, x2);
            acc3 = __fadd_rn(acc3, x3);
        }
        const float t = __fadd_rn(__fadd_rn(acc0, acc1), __fadd_rn(acc2, acc3));
        float s = 0.0f;
#pragma unroll
        for (int l = 0; l < 8; ++l) s = __fadd_rn(s, __shfl(t, l, 8));
        for (uint32_t i = chunks32 * 32u; i < a.D; ++i) s = __fadd_rn(s, v[i]);
        const float n2 = exact_score<16>(M_IP, LYNSE_IPFORM_SINGLE, v, v, a.D, g);
        const float inv = n2 > 1e-30f ? __fdiv_rn(1.0f, __builtin_sqrtf(n2)) : 0.0f;
        const bool mine = g == 0 && r < a.n;
        if (mine) {
            a.row_sum[row] = s;
            a.norm2[row] = n2;
            a.inv_norm[row] = inv;
        }
        const unsigned long long fin = __ballot(mine && __builtin_isfinite(s));
        if ((tid & 63u) == 0 && fin) atomicAdd(a.finite, (unsigned long long)__builtin_popcountll(fin));
    }
}

// desc: the largest sums first (a non-negative query), else the smallest
__global__ void __launch_bounds__(256) k_approx_sum_keys(const float* __restrict__ row_sum, uint64_t n, int desc, uint32_t* __restrict__ S) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) {
        const float s = row_sum[i];
        S[i] = __builtin_isfinite(s) ? score_ord(s, !desc) : RANGE_FAIL;
    }
}

struct ApproxCoarseArgs {
    const float* V;   // n rows of f32, pitch ld floats
    uint32_t ld, D;
    uint64_t n;
    const float* q;   // D floats
    ApproxBlocks blk;
    int ip_form;              // AF_IP / the expansions: the form of the dot product (single or batch8)
    float scale;              // AF_L1 / AF_CANBERRA: dim / sampled
    float q_norm2, q_inv;     // the expansions
    const float *norm2, *inv_norm;
    uint32_t* S;              // [n] score_ord images
};

// One sequential chain over the elements of a block slice (block_bray_curtis): the 8 lanes form the terms of 8 elements, every lane then
// adds them in element order.
__device__ __forceinline__ void approx_bray_block(const float* __restrict__ q, const float* __restrict__ v, uint32_t L, int g, float& num, float& den) {
    for (uint32_t c0 = 0; c0 < L; c0 += 8u) {
        const uint32_t e = c0 + (uint32_t)g;
        float tn = 0.0f, td = 0.0f;
        if (e < L) {
            const float x = q[e], y = v[e];
            tn = __builtin_fabsf(__fsub_rn(x, y));
            td = __builtin_fabsf(__fadd_rn(x, y));
        }
        const uint32_t cnt = L - c0 < 8u ? L - c0 : 8u;
#pragma unroll
        for (int l = 0; l < 8; ++l) {
            const float xn = __shfl(tn, l, 8), xd = __shfl(td, l, 8);
            if ((uint32_t)l < cnt) {
                num = __fadd_rn(num, xn);
                den = __fadd_rn(den, xd);
            }
        }
    }
}

// LDS: the query's sampled elements, block after block (AF_L2EXP / AF_COSEXP: one block = the whole row)
template <int FORM>
__global__ void __launch_bounds__(APX_NT) k_approx_coarse(ApproxCoarseArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm_apx[];
    const uint32_t tid = threadIdx.x;
    const int g = tid & 7;
    uint32_t off[3] = {0u, a.blk.len[0], a.blk.len[0] + a.blk.len[1]};
    for (uint32_t b = 0; b < a.blk.nb; ++b)
        for (uint32_t i = tid; i < a.blk.len[b]; i += APX_NT) sm_apx[off[b] + i] = a.q[a.blk.start[b] + i];
    __syncthreads();
    const uint64_t bound = (a.n + 31u) / 32u * 32u;   // whole workgroups run the same trip count (shuffles inside the 8 lanes)
    for (uint64_t r = (uint64_t)blockIdx.x * 32u + (tid >> 3); r < bound; r += (uint64_t)gridDim.x * 32u) {
        const uint64_t row = r < a.n ? r : a.n - 1;   // (a row past the end scores the last row again and is dropped)
        const float* v = a.V + row * a.ld;
        float d;
        if constexpr (FORM == AF_IP) {
            float acc = 0.0f;
            for (uint32_t b = 0; b < a.blk.nb; ++b)
                acc = __fadd_rn(acc, exact_score<16>(M_IP, a.ip_form, sm_apx + off[b], v + a.blk.start[b], a.blk.len[b], g));
            d = acc;
        } else if constexpr (FORM == AF_L2EXP) {
            const float dot = exact_score<16>(M_IP, a.ip_form, sm_apx, v, a.D, g);
            const float x = __fsub_rn(__fadd_rn(a.q_norm2, a.norm2[row]), __fmul_rn(2.0f, dot));
            d = x > 0.0f ? x : 0.0f;   // f32::max(x, 0.0): 0.0 for a NaN too
        } else if constexpr (FORM == AF_COSEXP) {
            const float dot = exact_score<16>(M_IP, a.ip_form, sm_apx, v, a.D, g);
            const float ri = a.inv_norm[row];
            d = ri <= 0.0f ? 1.0f : __fsub_rn(1.0f, __fmul_rn(__fmul_rn(dot, a.q_inv), ri));
        } else if constexpr (FORM == AF_L1 || FORM == AF_CANBERRA) {
            float sum = 0.0f;
            for (uint32_t b = 0; b < a.blk.nb; ++b)
                sum = __fadd_rn(sum, additive_score_m<(FORM == AF_L1 ? M_L1 : M_CANBERRA), 8>(sm_apx + off[b], v + a.blk.start[b], a.blk.len[b], g));
            d = __fmul_rn(sum, a.scale);
        } else if constexpr (FORM == AF_CHEBYSHEV) {
            float m = 0.0f;   // (chebyshev_f32 never returns a NaN: f32::max keeps m)
            for (uint32_t b = 0; b < a.blk.nb; ++b)
                m = additive_rmax(m, additive_score_m<M_CHEBYSHEV, 8>(sm_apx + off[b], v + a.blk.start[b], a.blk.len[b], g));
            d = m;
        } else {
            float num = 0.0f, den = 0.0f;
            for (uint32_t b = 0; b < a.blk.nb; ++b) approx_bray_block(sm_apx + off[b], v + a.blk.start[b], a.blk.len[b], g, num, den);
            d = den == 0.0f ? (num == 0.0f ? 0.0f : LY_INF) : __fdiv_rn(num, den);
        }
        if (g == 0 && r < a.n) a.S[row] = score_ord(d, FORM != AF_IP);
    }
}

struct ApproxRescoreArgs {
    const float* V;
    uint32_t ld, D;
    uint64_t n;
    const float* q;              // D floats
    const uint64_t* pool_rows;   // pool_ld entries, *pool_cnt valid
    const uint32_t* pool_cnt;
    uint32_t pool_ld;
    int metric;                  // M_IP (single-row form) or an additive id
    uint64_t* keys_out;          // [pool_ld] canonical keys of the exact scores
};

// LDS: the query
__global__ void __launch_bounds__(APX_NT) k_approx_rescore(ApproxRescoreArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm_apx[];
    const uint32_t tid = threadIdx.x;
    const int g = tid & 7;
    for (uint32_t i = tid; i < a.D; i += APX_NT) sm_apx[i] = a.q[i];
    __syncthreads();
    const uint32_t P = *a.pool_cnt < a.pool_ld ? *a.pool_cnt : a.pool_ld;
    if (P == 0) return;
    const bool asc = metric_ascending(a.metric);
    const uint32_t bound = (P + 31u) / 32u * 32u;
    for (uint32_t i = blockIdx.x * 32u + (tid >> 3); i < bound; i += gridDim.x * 32u) {
        const uint64_t r64 = a.pool_rows[i < P ? i : P - 1];
        const uint32_t row = r64 < a.n ? (uint32_t)r64 : 0u;   // (a pool entry is a row id < n)
        const float* v = a.V + (size_t)row * a.ld;
        float s = metric_additive(a.metric) ? additive_score<8>(a.metric, sm_apx, v, a.D, g)
                                            : exact_score<32>(M_IP, LYNSE_IPFORM_SINGLE, sm_apx, v, a.D, g);
        if (r64 >= a.n) s = __builtin_nanf("");   // (never: would rank last, make_key)
        if (g == 0 && i < P) a.keys_out[i] = make_key(s, row, asc);
    }
}

}  // namespace lynse
