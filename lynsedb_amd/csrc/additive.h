// additive.h — the additive metrics (ids 7-10: Manhattan, Chebyshev, Canberra, Bray-Curtis) in the reference's AVX2 forms
// (manhattan_avx2 / chebyshev_avx2 / canberra_avx2 / bray_curtis_avx2, src/distance/simd.rs:2136-2158, :2717-2737, :2764-2793,
// :2826-2865).  The contract block next to the metric enum of include/lynse_hip.h states the four forms; DESIGN.md §17.
//   additive_score     the device function: one (query, row) pair by the 8 lanes of a group, the result on all 8 (as exact_score);
//                      k_range_scan (range.h) calls it for the range search
//   k_additive_scan    the top-k scan: S[q][row] = the score_ord image of every live row's distance, RANGE_FAIL for a masked-out
//                      row.  None of the four is bilinear (no MFMA form): a VALU loop fed from LDS, the tiles staged LANE-MAJOR
//                      so that one ds_read_b128 brings four consecutive steps of a lane, QB queries' accumulators per lane.
// The cut and the order behind it are those of the range search (ScoreCut::cut<true>, k_pool_select; additive_host.inc).
#pragma once

#include "range.h"

namespace lynse {

// f32::max(m, d) with m never NaN (the fold starts at 0.0): the non-NaN operand
__device__ __forceinline__ float additive_rmax(float m, float d) { return d != d ? m : (m > d ? m : d); }

// one step of a lane's accumulators (y: the denominator sum of Bray-Curtis)
template <int M>
__device__ __forceinline__ void additive_step(float a, float b, float& x, float& y) {
    const float d = __builtin_fabsf(__fsub_rn(a, b));
    if constexpr (M == M_L1) {
        x = __fadd_rn(x, d);
        asm("" : "+v"(x));   // (kept scalar: paired over two queries as v_pk_add_f32 the |.| is no free source modifier any more)
    } else if constexpr (M == M_CHEBYSHEV) {
        x = (x > d) ? x : d;   // _mm256_max_ps(acc, d): d when either is NaN (never fmaxf)
    } else if constexpr (M == M_CANBERRA) {
        const float den = __fadd_rn(__builtin_fabsf(a), __builtin_fabsf(b));
        const float q = __fdiv_rn(d, den);
        x = __fadd_rn(x, (den == den && den != 0.0f) ? q : 0.0f);   // _CMP_NEQ_OQ: false for a NaN den
    } else {
        x = __fadd_rn(x, d);
        y = __fadd_rn(y, __builtin_fabsf(__fadd_rn(a, b)));
        asm("" : "+v"(x), "+v"(y));   // (as above)
    }
}

// lane l's accumulators folded into the running reduction (lanes 0 .. 7 in order, from 0.0)
template <int M>
__device__ __forceinline__ void additive_fold(float lx, float ly, float& x, float& y) {
    if constexpr (M == M_CHEBYSHEV) x = additive_rmax(x, lx);
    else x = __fadd_rn(x, lx);
    if constexpr (M == M_BRAY_CURTIS) y = __fadd_rn(y, ly);
}

// one tail element (scalar Rust)
template <int M>
__device__ __forceinline__ void additive_tail(float a, float b, float& x, float& y) {
    const float d = __builtin_fabsf(__fsub_rn(a, b));
    if constexpr (M == M_L1) {
        x = __fadd_rn(x, d);
    } else if constexpr (M == M_CHEBYSHEV) {
        x = additive_rmax(x, d);
    } else if constexpr (M == M_CANBERRA) {
        const float den = __fadd_rn(__builtin_fabsf(a), __builtin_fabsf(b));
        if (den != 0.0f) x = __fadd_rn(x, __fdiv_rn(d, den));   // plain !=: a NaN den adds NaN
    } else {
        x = __fadd_rn(x, d);
        y = __fadd_rn(y, __builtin_fabsf(__fadd_rn(a, b)));
    }
}

template <int M>
__device__ __forceinline__ float additive_finish(float x, float y) {
    if constexpr (M == M_BRAY_CURTIS) return y == 0.0f ? (x == 0.0f ? 0.0f : LY_INF) : __fdiv_rn(x, y);
    return x;
}

template <int M, int UB>
__device__ __forceinline__ float additive_score_m(const float* __restrict__ q, const float* __restrict__ v, uint32_t D, int g) {
    const uint32_t chunks = D / 8, rem = D % 8, base = chunks * 8;
    float x = 0.0f, y = 0.0f;
    uint32_t i = 0;
    for (; i + UB <= chunks; i += UB) {   // (loads issued UB steps at a time; the chain keeps the reference's order)
        float a[UB], b[UB];
#pragma unroll
        for (int u = 0; u < UB; ++u) { a[u] = q[(i + u) * 8 + g]; b[u] = v[(i + u) * 8 + g]; }
#pragma unroll
        for (int u = 0; u < UB; ++u) additive_step<M>(a[u], b[u], x, y);
    }
    for (; i < chunks; ++i) additive_step<M>(q[i * 8 + g], v[i * 8 + g], x, y);
    float sx = 0.0f, sy = 0.0f;
#pragma unroll
    for (int l = 0; l < 8; ++l) additive_fold<M>(__shfl(x, l, 8), M == M_BRAY_CURTIS ? __shfl(y, l, 8) : 0.0f, sx, sy);
    for (uint32_t t = 0; t < rem; ++t) additive_tail<M>(q[base + t], v[base + t], sx, sy);
    return additive_finish<M>(sx, sy);
}

// The distance of ids 7-10 for one (query, row) pair: 8 lanes (g = lane & 7) share the pair, q and v are row-major, the result is
// the same on all 8 lanes.  The metric is uniform: callers branch on it at the call site (exact_score serves ids 0-2).
template <int UB>   // (declared in range.h, UB = 8 by default)
__device__ __forceinline__ float additive_score(int metric, const float* __restrict__ q, const float* __restrict__ v, uint32_t D, int g) {
    switch (metric) {
    case M_L1: return additive_score_m<M_L1, UB>(q, v, D, g);
    case M_CHEBYSHEV: return additive_score_m<M_CHEBYSHEV, UB>(q, v, D, g);
    case M_CANBERRA: return additive_score_m<M_CANBERRA, UB>(q, v, D, g);
    default: return additive_score_m<M_BRAY_CURTIS, UB>(q, v, D, g);
    }
}

// ---- the top-k scan ------------------------------------------------------------------------------------------------------------
// LDS image of a vector x of D floats, LANE-MAJOR: the body element 8 i + g at g * LP + i (lane g's steps contiguous: one
// ds_read_b128 = four steps), the D % 8 tail elements in a table of their own (8 floats per vector).  LP = 4 s with s odd and
// >= ceil(chunks / 4); a vector's body is 8 LP = 32 s floats.  Banks (MI355X_MICROARCH.md, LDS: ds_read_b128 is served in four
// groups of 16 lanes — half-rows of four different 8-lane groups — over the 16 16-B slots of a 256-B bank row): lane g of the
// r-th row group of a wave reads slot r * 8 s + g * s + i / 4; with s odd the 16 lanes of a group fall on 16 different slots
// (multiply by s^-1 mod 16: r * 8 + g over {0-3, 12-15, 20-27} or {4-11, 16-19, 28-31}).  The query reads are the same address
// for every row group (a broadcast), 8 slots apart by s.
constexpr int ADD_NT = 256;              // 32 groups of 8 lanes, one row per group and trip
constexpr uint32_t ADD_MAX_ROWS = 64;    // rows of an LDS tile
constexpr uint32_t ADD_MAX_Q = 32;       // queries of an LDS tile

__host__ __device__ inline uint32_t additive_lane_pitch(uint32_t D) {
    const uint32_t s = (D / 8 + 3) / 4;
    return 4u * (s | 1u);
}

struct AdditiveScanArgs {
    const float* V;         // n rows of f32, pitch ld floats (ld % 4 == 0, pad columns zero)
    uint32_t ld, D;
    uint64_t n;
    const float* Q;         // nq x D
    uint32_t nq;
    const uint64_t* mask;   // NULL = every row
    uint64_t mask_words;
    uint32_t R, TQ;         // rows / queries of an LDS tile
    uint32_t* S;            // [nq][n]
};

// lane g + K's value (the same row of 16 lanes; what lane 0 of an 8-lane group needs from its lanes 1 .. 7)
template <int K>
__device__ __forceinline__ float additive_lane_up(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x100 + K /* row_shl:K */, 0xf, 0xf, true));
}

// the sequential reduction of a group's lanes 0 .. 7, valid on the group's lane 0 (VALU only: no LDS permute per pair)
template <int M>
__device__ __forceinline__ void additive_reduce0(float x, float y, float& sx, float& sy) {
    sx = 0.0f;
    sy = 0.0f;
    additive_fold<M>(x, y, sx, sy);
    additive_fold<M>(additive_lane_up<1>(x), M == M_BRAY_CURTIS ? additive_lane_up<1>(y) : 0.0f, sx, sy);
    additive_fold<M>(additive_lane_up<2>(x), M == M_BRAY_CURTIS ? additive_lane_up<2>(y) : 0.0f, sx, sy);
    additive_fold<M>(additive_lane_up<3>(x), M == M_BRAY_CURTIS ? additive_lane_up<3>(y) : 0.0f, sx, sy);
    additive_fold<M>(additive_lane_up<4>(x), M == M_BRAY_CURTIS ? additive_lane_up<4>(y) : 0.0f, sx, sy);
    additive_fold<M>(additive_lane_up<5>(x), M == M_BRAY_CURTIS ? additive_lane_up<5>(y) : 0.0f, sx, sy);
    additive_fold<M>(additive_lane_up<6>(x), M == M_BRAY_CURTIS ? additive_lane_up<6>(y) : 0.0f, sx, sy);
    additive_fold<M>(additive_lane_up<7>(x), M == M_BRAY_CURTIS ? additive_lane_up<7>(y) : 0.0f, sx, sy);
}

// LDS: TQ query bodies of 8 LP floats | R row bodies | TQ query tails of 8 floats | R row tails
template <int M, int QB>
__global__ void __launch_bounds__(ADD_NT) k_additive_scan(AdditiveScanArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm_add[];
    const uint32_t tid = threadIdx.x, grp = tid >> 3, g = tid & 7u;
    const uint32_t D = a.D, chunks = D / 8, rem = D % 8, base = chunks * 8;
    const uint32_t LP = additive_lane_pitch(D), VS = 8u * LP;
    const uint32_t q0 = blockIdx.y * a.TQ;
    const uint32_t tq = a.nq - q0 < a.TQ ? a.nq - q0 : a.TQ;
    float* q_l = sm_add;
    float* rows_l = q_l + (size_t)a.TQ * VS;
    float* qt_l = rows_l + (size_t)a.R * VS;
    float* rt_l = qt_l + (size_t)a.TQ * 8u;
    for (uint32_t i = tid; i < tq * D; i += ADD_NT) {
        const uint32_t j = i / D, e = i - j * D;
        const float x = a.Q[(size_t)q0 * D + i];
        if (e < base) q_l[(size_t)j * VS + (e & 7u) * LP + (e >> 3)] = x;
        else qt_l[j * 8u + (e - base)] = x;
    }
    const uint32_t vpr = (D + 3u) / 4u;   // 16-B pieces of a row
    const uint64_t tiles = (a.n + a.R - 1) / a.R;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint64_t r0 = t * a.R;
        const uint32_t rn = a.n - r0 < a.R ? (uint32_t)(a.n - r0) : a.R;
        __syncthreads();   // the previous tile has been scored (first trip: nothing to wait for)
        for (uint32_t p = tid; p < rn * vpr; p += ADD_NT) {
            const uint32_t r = p / vpr, c = p - r * vpr;
            const f32x4 x = *reinterpret_cast<const f32x4*>(a.V + (r0 + r) * a.ld + (size_t)c * 4u);
#pragma unroll
            for (uint32_t u = 0; u < 4; ++u) {
                const uint32_t e = c * 4u + u;
                if (e < base) rows_l[(size_t)r * VS + (e & 7u) * LP + (e >> 3)] = x[u];
                else if (e < D) rt_l[r * 8u + (e - base)] = x[u];
            }
        }
        __syncthreads();   // the tile (first trip: and the queries) is staged
        for (uint32_t rr = grp; rr < rn; rr += 32u) {   // (the 8 lanes of a group share rr)
            const uint64_t row = r0 + rr;
            if (!range_live(a.mask, a.mask_words, row)) {
                if (g == 0)
                    for (uint32_t j = 0; j < tq; ++j) a.S[(size_t)(q0 + j) * a.n + row] = RANGE_FAIL;
                continue;
            }
            const float* vp = rows_l + (size_t)rr * VS + g * LP;
            for (uint32_t jb = 0; jb < tq; jb += QB) {
                const float* qp[QB];   // (a block past the tile's queries scores its last query again and drops it)
#pragma unroll
                for (int u = 0; u < QB; ++u) qp[u] = q_l + (size_t)(jb + u < tq ? jb + u : tq - 1u) * VS + g * LP;
                float x[QB], y[QB];
#pragma unroll
                for (int u = 0; u < QB; ++u) { x[u] = 0.0f; y[u] = 0.0f; }
                // four steps per ds_read_b128; two register sets take turns, so that the reads of the next four steps are issued
                // before the arithmetic of these four (two workgroups of four waves per CU: a wave keeps its own reads in flight)
                const uint32_t full = chunks & ~3u;
                auto load = [&](uint32_t at, f32x4& v4, f32x4 (&q4)[QB]) {
                    v4 = *reinterpret_cast<const f32x4*>(vp + at);
#pragma unroll
                    for (int u = 0; u < QB; ++u) q4[u] = *reinterpret_cast<const f32x4*>(qp[u] + at);
                };
                auto steps = [&](const f32x4& v4, const f32x4 (&q4)[QB]) {
                    asm volatile("" ::: "memory");   // (the reads issued so far stay above the arithmetic)
#pragma unroll
                    for (int u = 0; u < QB; ++u) {
                        additive_step<M>(q4[u][0], v4[0], x[u], y[u]);
                        additive_step<M>(q4[u][1], v4[1], x[u], y[u]);
                        additive_step<M>(q4[u][2], v4[2], x[u], y[u]);
                        additive_step<M>(q4[u][3], v4[3], x[u], y[u]);
                    }
                };
                // (a read of the four steps past the last full group stays inside the allocation: the tail tables follow the bodies)
                f32x4 va, vb, qa[QB], qb[QB];
                uint32_t i = 0;
                if (full) load(0, va, qa);
                for (; i + 8 <= full; i += 8) {
                    load(i + 4, vb, qb);
                    steps(va, qa);
                    load(i + 8, va, qa);
                    steps(vb, qb);
                }
                if (i < full) {
                    steps(va, qa);
                    i += 4;
                }
                if (i < chunks) {   // the last 1 .. 3 steps (the read stays inside the lane's LP floats)
                    const uint32_t left = chunks - i;
                    const f32x4 v4 = *reinterpret_cast<const f32x4*>(vp + i);
#pragma unroll
                    for (int u = 0; u < QB; ++u) {
                        const f32x4 q4 = *reinterpret_cast<const f32x4*>(qp[u] + i);
                        additive_step<M>(q4[0], v4[0], x[u], y[u]);
                        if (left > 1) additive_step<M>(q4[1], v4[1], x[u], y[u]);
                        if (left > 2) additive_step<M>(q4[2], v4[2], x[u], y[u]);
                    }
                }
#pragma unroll
                for (int u = 0; u < QB; ++u) {
                    float sx, sy;
                    additive_reduce0<M>(x[u], y[u], sx, sy);
                    const uint32_t j = jb + u < tq ? jb + u : tq - 1u;
                    for (uint32_t e = 0; e < rem; ++e) additive_tail<M>(qt_l[j * 8u + e], rt_l[rr * 8u + e], sx, sy);
                    const float d = additive_finish<M>(sx, sy);
                    if (g == 0 && jb + u < tq) a.S[(size_t)(q0 + j) * a.n + row] = score_ord(d, true);   // (a NaN goes in as +inf)
                }
            }
        }
    }
}

}  // namespace lynse
