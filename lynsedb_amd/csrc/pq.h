// pq.h — FLAT-{IP,L2,COS}-PQ (PQIndex, src/storage/pq_mmap.rs): the product quantiser's training, encode, ADC lookup tables,
// the ADC scan over the u8 codes and the exact selection of the N best ADC scores.  The exact rescore of those N rows is
// k_pool_rerank (kernels.h).  DESIGN.md §12.
//   k_pq_gather     the training sample (rows 0, s, 2s, ...) as a dense n x dim matrix
//   k_pq_init       random_init_centroids after the host drew the indices (the SmallRng stream is host code)
//   k_pq_assign     assignment of rows against one subspace's K codewords (training and encode)
//   k_pq_update     per-cluster sums in ascending member order, count, * (1 / count)
//   k_pq_empty      the empty-cluster rule (source = the LAST most-populated cluster)
//   k_pq_lut        lut[q][m][c] with the single-pair kernels' order
//   k_pq_adc        THE HOT KERNEL: codes streamed from HBM, the tables of QB queries in LDS, one thread adds a row's M lookups in m order
//   k_pq_hist / k_pq_find / k_pq_emit   radix selection of the N best (ADC score, row) keys per query, 11 bits per pass
#pragma once

#include "kernels.h"

namespace lynse {

// simd::l2_squared_f32 / inner_product_f32 (simd.rs:1343-1396, :1529-1581) for one pair in ONE thread: the two 8-lane
// accumulators of the AVX2 kernels, the hsum256 order ((l0+l4)+(l1+l5))+((l2+l6)+(l3+l7)), then the n % 8 tail as separate
// multiply + add.  Bit-equal to exact_score's 8-lane form (and to lo_l2_single / lo_ip_single).
template <bool IP>
__device__ __forceinline__ float pq_hsum_tail(float (&acc0)[8], const float (&acc1)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) acc0[j] = __fadd_rn(acc0[j], acc1[j]);
    return __fadd_rn(__fadd_rn(__fadd_rn(acc0[0], acc0[4]), __fadd_rn(acc0[1], acc0[5])),
                     __fadd_rn(__fadd_rn(acc0[2], acc0[6]), __fadd_rn(acc0[3], acc0[7])));
}

template <bool IP>
__device__ __forceinline__ float pq_step(float x, float y, float acc) {
    if (IP) return __fmaf_rn(x, y, acc);
    const float d = __fsub_rn(x, y);
    return __fmaf_rn(d, d, acc);
}

template <bool IP>
__device__ __forceinline__ float pq_tail(float x, float y, float sum) {
    if (IP) return __fadd_rn(sum, __fmul_rn(x, y));
    const float d = __fsub_rn(x, y);
    return __fadd_rn(sum, __fmul_rn(d, d));
}

// both operands in memory (any length)
template <bool IP>
__device__ __forceinline__ float pq_pair(const float* a, const float* b, uint32_t n) {
    const uint32_t chunks = n / 8, dbl = chunks / 2;
    float acc0[8], acc1[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { acc0[j] = 0.0f; acc1[j] = 0.0f; }
    for (uint32_t i = 0; i < dbl; ++i) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            acc0[j] = pq_step<IP>(a[i * 16 + j], b[i * 16 + j], acc0[j]);
            acc1[j] = pq_step<IP>(a[i * 16 + 8 + j], b[i * 16 + 8 + j], acc1[j]);
        }
    }
    if (chunks & 1) {
#pragma unroll
        for (int j = 0; j < 8; ++j) acc0[j] = pq_step<IP>(a[dbl * 16 + j], b[dbl * 16 + j], acc0[j]);
    }
    float sum = pq_hsum_tail<IP>(acc0, acc1);
    for (uint32_t e = chunks * 8; e < n; ++e) sum = pq_tail<IP>(a[e], b[e], sum);
    return sum;
}

// the first operand in registers (n <= SS): every index is a compile-time constant, so `a` stays in VGPRs
template <int SS, bool IP>
__device__ __forceinline__ float pq_pair_reg(const float (&a)[SS], const float* b, uint32_t n) {
    const uint32_t chunks = n / 8, dbl = chunks / 2;
    float acc0[8], acc1[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { acc0[j] = 0.0f; acc1[j] = 0.0f; }
#pragma unroll
    for (int i = 0; i < SS / 16; ++i) {
        if ((uint32_t)i < dbl) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                acc0[j] = pq_step<IP>(a[i * 16 + j], b[i * 16 + j], acc0[j]);
                acc1[j] = pq_step<IP>(a[i * 16 + 8 + j], b[i * 16 + 8 + j], acc1[j]);
            }
        }
    }
#pragma unroll
    for (int i = 0; i * 16 + 8 <= SS; ++i) {
        if ((uint32_t)i == dbl && (chunks & 1)) {
#pragma unroll
            for (int j = 0; j < 8; ++j) acc0[j] = pq_step<IP>(a[i * 16 + j], b[i * 16 + j], acc0[j]);
        }
    }
    float sum = pq_hsum_tail<IP>(acc0, acc1);
#pragma unroll
    for (int e = 0; e < SS; ++e)
        if ((uint32_t)e >= chunks * 8 && (uint32_t)e < n) sum = pq_tail<IP>(a[e], b[e], sum);
    return sum;
}

// rows r = 0, s, 2s, ... (n_out of them) of V (pitch ld) -> T (pitch D)
__global__ void __launch_bounds__(256) k_pq_gather(const float* __restrict__ V, uint32_t ld, uint32_t D, uint64_t s, uint64_t n_out,
                                                   float* __restrict__ T) {
    const uint64_t total = n_out * D;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) {
        const uint64_t r = i / D;
        const uint32_t d = (uint32_t)(i % D);
        T[i] = V[r * s * ld + d];
    }
}

// random_init_centroids (pq_mmap.rs:665-689) after the draws: block = subspace m, thread = a column d of it; centroid c < chosen[m]
// is sample row idx[m][c]'s sub-vector, every later one cb[c-1][d] * (1 + 0.001 d) in f32
__global__ void __launch_bounds__(64) k_pq_init(const float* __restrict__ T, uint32_t D, uint32_t ss, uint32_t K,
                                                const uint32_t* __restrict__ idx, const uint32_t* __restrict__ chosen, float* __restrict__ cb) {
    const uint32_t m = blockIdx.x;
    float* c_m = cb + (size_t)m * K * ss;
    for (uint32_t d = threadIdx.x; d < ss; d += 64) {
        const float f = __fadd_rn(1.0f, __fmul_rn(0.001f, (float)d));
        for (uint32_t c = 0; c < K; ++c)
            c_m[(size_t)c * ss + d] = c < chosen[m] ? T[(size_t)idx[(size_t)m * K + c] * D + (size_t)m * ss + d]
                                                    : __fmul_rn(c_m[(size_t)(c - 1) * ss + d], f);
    }
}

// One thread = one row, blockIdx.y = subspace m (its codebook staged in LDS when cb_lds).  best = the first c whose
// l2_squared_f32 is strictly below the best so far, starting from f32::MAX (NaN never wins; an all-NaN sub-vector keeps 0).
// Training: asg[m][i] updated, changed[m] |= 1 when it moved; encode: codes[i][m].
struct PqAssignArgs {
    const float* V;
    uint32_t ld;            // row pitch of V (floats)
    uint64_t n;
    uint32_t M, ss, K;
    const float* cb;        // [M][K][ss]
    int cb_lds;
    const uint32_t* active; // [M] training: subspaces still iterating; NULL = all
    uint32_t* asg;          // [M][n] or NULL
    uint32_t* changed;      // [M] or NULL
    uint8_t* codes;         // [n][M] or NULL
};

template <int SS>   // 0: the sub-vector is read from memory (ss > 128)
__global__ void __launch_bounds__(256) k_pq_assign(PqAssignArgs a) {
    extern __shared__ float cb_l[];
    const uint32_t m = blockIdx.y, tid = threadIdx.x;
    if (a.active && !a.active[m]) return;
    const float* cb = a.cb + (size_t)m * a.K * a.ss;
    if (a.cb_lds) {
        for (uint32_t i = tid; i < a.K * a.ss; i += 256) cb_l[i] = cb[i];
        __syncthreads();
        cb = cb_l;
    }
    const uint64_t i = (uint64_t)blockIdx.x * 256 + tid;
    if (i >= a.n) return;
    const float* v = a.V + i * a.ld + (size_t)m * a.ss;
    float best = __FLT_MAX__;
    uint32_t bc = 0;
    if constexpr (SS > 0) {
        float r[SS];
#pragma unroll
        for (int e = 0; e < SS; ++e) r[e] = (uint32_t)e < a.ss ? v[e] : 0.0f;
        for (uint32_t c = 0; c < a.K; ++c) {
            const float d = pq_pair_reg<SS, false>(r, cb + (size_t)c * a.ss, a.ss);
            if (d < best) { best = d; bc = c; }
        }
    } else {
        for (uint32_t c = 0; c < a.K; ++c) {
            const float d = pq_pair<false>(v, cb + (size_t)c * a.ss, a.ss);
            if (d < best) { best = d; bc = c; }
        }
    }
    if (a.codes) a.codes[i * a.M + m] = (uint8_t)bc;
    if (a.asg) {
        uint32_t* p = a.asg + (size_t)m * a.n + i;
        if (*p != bc) {
            *p = bc;
            atomicOr(a.changed + m, 1u);
        }
    }
}

// The centroid update of kmeans_subspace (pq_mmap.rs:615-652).  Block = (c, m), thread = column d.  The members of cluster c are
// visited in ascending row order (one sequential f32 sum per column, as the reference's row loop adds them), the assignment words
// read once per block (uniform loads).  raw[m][c] keeps the sums, cb[m][c] gets sum * fl(1 / count); count[m][c] for k_pq_empty.
__global__ void __launch_bounds__(64) k_pq_update(const float* __restrict__ T, uint32_t D, uint64_t n, uint32_t ss, uint32_t K,
                                                  const uint32_t* __restrict__ active, const uint32_t* __restrict__ asg,
                                                  float* __restrict__ raw, float* __restrict__ cb, uint32_t* __restrict__ count) {
    const uint32_t c = blockIdx.x, m = blockIdx.y;
    if (!active[m]) return;
    const uint32_t* as = asg + (size_t)m * n;
    for (uint32_t d0 = 0; d0 < ss; d0 += 64) {
        const uint32_t d = d0 + threadIdx.x;
        float s = 0.0f;
        uint32_t cnt = 0;
        for (uint64_t i = 0; i < n; ++i) {
            if (as[i] == c) {
                ++cnt;
                if (d < ss) s = __fadd_rn(s, T[i * D + (size_t)m * ss + d]);
            }
        }
        const size_t o = ((size_t)m * K + c) * ss + d;
        if (d < ss) {
            raw[o] = s;
            if (cnt > 0) cb[o] = __fmul_rn(s, __fdiv_rn(1.0f, (float)cnt));
        }
        if (d0 == 0 && threadIdx.x == 0) count[(size_t)m * K + c] = cnt;
    }
}

// Empty clusters (pq_mmap.rs:633-650): src = the LAST index of the largest count (max_by_key); an empty c becomes
// new[src] * (1 + 0.01 ((d % 2) - 0.5)), where new[src] is already divided when src < c and still the raw sum when src > c.
__global__ void __launch_bounds__(64) k_pq_empty(uint32_t ss, uint32_t K, const uint32_t* __restrict__ active,
                                                 const float* __restrict__ raw, float* __restrict__ cb, const uint32_t* __restrict__ count) {
    const uint32_t m = blockIdx.x;
    if (!active[m]) return;
    const uint32_t* cn = count + (size_t)m * K;
    uint32_t src = 0, best = 0;
    for (uint32_t c = 0; c < K; ++c)
        if (cn[c] >= best) { best = cn[c]; src = c; }
    for (uint32_t c = 0; c < K; ++c) {
        if (cn[c] != 0) continue;
        const float* from = (src < c ? cb : raw) + ((size_t)m * K + src) * ss;
        for (uint32_t d = threadIdx.x; d < ss; d += 64) {
            const float f = __fadd_rn(1.0f, __fmul_rn(0.01f, __fsub_rn((float)(d % 2), 0.5f)));
            cb[((size_t)m * K + c) * ss + d] = __fmul_rn(from[d], f);
        }
    }
}

// build_lut (pq_mmap.rs:548-570): lut[q][m][c] = inner_product_f32 (IP) or l2_squared_f32 (L2 and cosine) of the RAW query's
// sub-vector m and codeword c.  Thread = (q, m, c).
__global__ void __launch_bounds__(256) k_pq_lut(const float* __restrict__ Q, uint32_t nq, uint32_t D, uint32_t M, uint32_t ss, uint32_t K,
                                                const float* __restrict__ cb, int ip, float* __restrict__ lut) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (uint64_t)nq * M * K) return;
    const uint32_t c = (uint32_t)(t % K), m = (uint32_t)((t / K) % M), q = (uint32_t)(t / ((uint64_t)K * M));
    const float* qs = Q + (size_t)q * D + (size_t)m * ss;
    const float* b = cb + ((size_t)m * K + c) * ss;
    lut[t] = ip ? pq_pair<true>(qs, b, ss) : pq_pair<false>(qs, b, ss);
}

// The ADC scan.  Block = PQ_NT threads x PQ_R rows each, blockIdx.y = a group of QB queries whose tables sit in LDS as
// [QB][mc][K] f32 (mc subspaces per chunk: all M when they fit, else the table goes through LDS chunk by chunk and every thread
// keeps its running sums in registers across the chunks).  A row's score is 0.0f + lut[0][c0] + lut[1][c1] + ... added by one
// thread in ascending m, exactly the reference's scan order.  Output: the order-preserving 32-bit image of the score
// (score_ord: ascending = best first for the metric, NaN last, -0 == +0), S[q][row].
constexpr int PQ_NT = 512;
constexpr int PQ_R = 2;

__device__ __forceinline__ uint32_t score_ord(float s, bool asc) { return (uint32_t)(make_key(s, 0u, asc) >> 32); }

struct PqAdcArgs {
    const uint8_t* codes;   // [n][M]
    uint64_t n;
    uint32_t M, K, mc;
    const float* lut;       // [nq][M][K]
    uint32_t nq;
    int asc;
    uint32_t* S;            // [nq][n]
};

template <int QB>
__global__ void __launch_bounds__(PQ_NT) k_pq_adc(PqAdcArgs a) {
    extern __shared__ float lut_l[];
    const uint32_t tid = threadIdx.x, q0 = blockIdx.y * QB;
    const uint32_t nqb = a.nq - q0 < (uint32_t)QB ? a.nq - q0 : (uint32_t)QB;
    const uint64_t base = (uint64_t)blockIdx.x * PQ_NT * PQ_R;
    const uint32_t MK = a.M * a.K;
    float acc[QB][PQ_R];
#pragma unroll
    for (int j = 0; j < QB; ++j)
#pragma unroll
        for (int r = 0; r < PQ_R; ++r) acc[j][r] = 0.0f;
    const bool words = (a.M % 4) == 0 && (a.mc % 4) == 0;
    for (uint32_t m0 = 0; m0 < a.M; m0 += a.mc) {
        const uint32_t mcc = a.M - m0 < a.mc ? a.M - m0 : a.mc;
        if (m0) __syncthreads();
        for (uint32_t i = tid; i < (uint32_t)QB * mcc * a.K; i += PQ_NT) {
            const uint32_t j = i / (mcc * a.K), w = i % (mcc * a.K);
            lut_l[j * a.mc * a.K + w] = j < nqb ? a.lut[(size_t)(q0 + j) * MK + (size_t)m0 * a.K + w] : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < PQ_R; ++r) {
            const uint64_t row = base + (uint64_t)r * PQ_NT + tid;
            if (row >= a.n) continue;
            const uint8_t* cr = a.codes + row * a.M + m0;
            if (words) {
                for (uint32_t mm = 0; mm < mcc; mm += 4) {
                    const uint32_t w = *reinterpret_cast<const uint32_t*>(cr + mm);
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const uint32_t off = (mm + b) * a.K + ((w >> (8 * b)) & 0xffu);
#pragma unroll
                        for (int j = 0; j < QB; ++j) acc[j][r] = __fadd_rn(acc[j][r], lut_l[j * a.mc * a.K + off]);
                    }
                }
            } else {
                for (uint32_t mm = 0; mm < mcc; ++mm) {
                    const uint32_t off = mm * a.K + cr[mm];
#pragma unroll
                    for (int j = 0; j < QB; ++j) acc[j][r] = __fadd_rn(acc[j][r], lut_l[j * a.mc * a.K + off]);
                }
            }
        }
    }
    const bool asc = a.asc != 0;
#pragma unroll
    for (int r = 0; r < PQ_R; ++r) {
        const uint64_t row = base + (uint64_t)r * PQ_NT + tid;
        if (row >= a.n) continue;
#pragma unroll
        for (int j = 0; j < QB; ++j)
            if ((uint32_t)j < nqb) a.S[(size_t)(q0 + j) * a.n + row] = score_ord(acc[j][r], asc);
    }
}

// Radix selection of the N smallest 64-bit keys (score_ord << 32 | row) of each query — the canonical (ADC score, row) cut.  The
// keys are unique (rows are), so the N-th smallest is one key and "every key <= it" is exactly N rows.  Per query: the bits above
// `hi` are fixed to `prefix`, `need` is the rank still to find inside them; a pass histograms the next 11 bits (LDS, then global
// atomics), k_pq_find picks the bucket holding rank `need`.  A query is done once its bucket holds exactly `need` keys (all of
// them are taken) or the last bit is fixed.
struct PqSel {
    uint64_t prefix;
    uint32_t hi;            // 64: nothing fixed yet
    uint32_t need;
    uint32_t done;
    uint32_t emitted;
};
constexpr uint32_t PQ_DIGIT = 11;
constexpr uint32_t PQ_BINS = 1u << PQ_DIGIT;

__device__ __forceinline__ bool pq_sel_match(uint64_t key, const PqSel& s) { return s.hi >= 64 || (key >> s.hi) == s.prefix; }

__global__ void __launch_bounds__(256) k_pq_hist(const uint32_t* __restrict__ S, uint64_t n, const PqSel* __restrict__ sel,
                                                 uint32_t* __restrict__ hist, uint32_t rows_per_block) {
    __shared__ uint32_t h[PQ_BINS];
    const uint32_t q = blockIdx.y, tid = threadIdx.x;
    const PqSel s = sel[q];
    if (s.done) return;
    const uint32_t lo = s.hi > PQ_DIGIT ? s.hi - PQ_DIGIT : 0u, w = s.hi - lo;
    for (uint32_t i = tid; i < PQ_BINS; i += 256) h[i] = 0;
    __syncthreads();
    const uint64_t r0 = (uint64_t)blockIdx.x * rows_per_block, r1 = r0 + rows_per_block < n ? r0 + rows_per_block : n;
    const uint32_t* Sq = S + (size_t)q * n;
    for (uint64_t rb = r0 + tid; rb < r1; rb += 256 * 8) {   // 8 independent loads in flight per thread, then their updates
        uint32_t v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = rb + 256 * j < r1 ? Sq[rb + 256 * j] : 0u;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint64_t r = rb + 256 * j, key = ((uint64_t)v[j] << 32) | r;
            if (r < r1 && pq_sel_match(key, s)) atomicAdd(&h[(uint32_t)(key >> lo) & ((1u << w) - 1u)], 1u);
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < (1u << w); i += 256)
        if (h[i]) atomicAdd(&hist[(size_t)q * PQ_BINS + i], h[i]);
}

__global__ void __launch_bounds__(256) k_pq_find(PqSel* __restrict__ sel, uint32_t* __restrict__ hist) {
    __shared__ uint32_t part[256], own[2];
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    PqSel s = sel[q];
    if (s.done) return;
    const uint32_t lo = s.hi > PQ_DIGIT ? s.hi - PQ_DIGIT : 0u, w = s.hi - lo, nb = 1u << w;
    uint32_t* hq = hist + (size_t)q * PQ_BINS;
    const uint32_t per = (nb + 255) / 256;   // bins per thread, contiguous (at most PQ_BINS / 256 = 8: read once, kept in registers)
    uint32_t t = 0, mine[PQ_BINS / 256];
#pragma unroll
    for (uint32_t j = 0; j < PQ_BINS / 256; ++j) {
        const uint32_t b = tid * per + j;
        mine[j] = (j < per && b < nb) ? hq[b] : 0u;
        t += mine[j];
    }
    part[tid] = t;
    __syncthreads();
    // inclusive prefix sums of the 256 partial counts (one thread walking them in LDS took longer than the histogram pass);
    // the owner is the first thread whose bins reach rank `need`: before < need <= before + t, true for exactly one thread
    for (uint32_t d = 1; d < 256; d <<= 1) {
        const uint32_t add = tid >= d ? part[tid - d] : 0u;
        __syncthreads();
        part[tid] += add;
        __syncthreads();
    }
    const uint32_t before = part[tid] - t;
    if (tid == 0) own[0] = 256u;   // no owner (never: need <= the keys that match)
    __syncthreads();
    if (before < s.need && s.need <= before + t) {
        own[0] = tid;
        own[1] = before;
    }
    __syncthreads();
    const uint32_t owner = own[0];
    if (tid == owner) {
        uint32_t cum = own[1], b = tid * per, in_b = mine[0];
#pragma unroll
        for (uint32_t j = 0; j + 1 < PQ_BINS / 256; ++j) {   // the first bin of mine whose running count reaches `need`, else the last
            if (b == tid * per + j && b + 1 < (tid + 1) * per && b + 1 < nb && cum + mine[j] < s.need) {
                cum += mine[j];
                ++b;
                in_b = mine[j + 1];
            }
        }
        s.need -= cum;
        s.prefix = (s.hi >= 64 ? 0ull : (s.prefix << w)) | b;
        s.hi = lo;
        s.done = (in_b == s.need || lo == 0) ? 1u : 0u;
        sel[q] = s;
    }
    __syncthreads();
    for (uint32_t b = tid; b < nb; b += 256) hq[b] = 0;
}

// every row whose key is <= the selected one (the first s.hi bits <= prefix) goes to the pool, in no particular order.  A block
// collects the hits of a tile of PQ_EMIT_TILE rows in LDS and reserves their pool slots with ONE atomic on the query's counter (a
// pool of thousands of rows, one returning atomic each on the same address, cost more than reading the scores).
constexpr uint32_t PQ_EMIT_TILE = 2048;   // 256 threads x 8 independent loads

template <bool KEYS = false>   // KEYS: the whole key (image << 32 | row) goes out instead of the row (range search sorts them as they are)
__global__ void __launch_bounds__(256) k_pq_emit(const uint32_t* __restrict__ S, uint64_t n, PqSel* __restrict__ sel, uint32_t pool_ld,
                                                 uint64_t* __restrict__ pool_rows, uint32_t* __restrict__ pool_cnt) {
    __shared__ uint32_t hit[PQ_EMIT_TILE];
    __shared__ uint32_t n_hit, base;
    const uint32_t q = blockIdx.y, tid = threadIdx.x;
    const PqSel s = sel[q];
    const uint32_t* Sq = S + (size_t)q * n;
    for (uint64_t t0 = (uint64_t)blockIdx.x * PQ_EMIT_TILE; t0 < n; t0 += (uint64_t)gridDim.x * PQ_EMIT_TILE) {
        if (tid == 0) n_hit = 0;
        __syncthreads();
        const uint64_t t1 = t0 + PQ_EMIT_TILE < n ? t0 + PQ_EMIT_TILE : n;
        uint32_t v[PQ_EMIT_TILE / 256];
#pragma unroll
        for (uint32_t j = 0; j < PQ_EMIT_TILE / 256; ++j) v[j] = t0 + 256 * j + tid < t1 ? Sq[t0 + 256 * j + tid] : 0u;
#pragma unroll
        for (uint32_t j = 0; j < PQ_EMIT_TILE / 256; ++j) {
            const uint64_t r = t0 + 256 * j + tid, key = ((uint64_t)v[j] << 32) | r;
            if (r < t1 && (key >> s.hi) <= s.prefix) hit[atomicAdd(&n_hit, 1u)] = (uint32_t)(r - t0);
        }
        __syncthreads();
        if (tid == 0 && n_hit) base = atomicAdd(&pool_cnt[q], n_hit);
        __syncthreads();
        for (uint32_t i = tid; i < n_hit; i += 256)
            if (base + i < pool_ld)
                pool_rows[(size_t)q * pool_ld + base + i] = KEYS ? (((uint64_t)Sq[t0 + hit[i]] << 32) | (t0 + hit[i])) : t0 + hit[i];
        __syncthreads();
    }
}

// N == n_pq: the pool is every row
__global__ void __launch_bounds__(256) k_pq_pool_all(uint64_t n, uint32_t nq, uint32_t pool_ld, uint64_t* __restrict__ pool_rows,
                                                     uint32_t* __restrict__ pool_cnt) {
    const uint64_t total = (uint64_t)nq * n;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) {
        const uint64_t q = i / n, r = i % n;
        pool_rows[q * pool_ld + r] = r;
        if (r == 0) pool_cnt[q] = (uint32_t)n;
    }
}

}  // namespace lynse
