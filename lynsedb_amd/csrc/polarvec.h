// polarvec.h — FLAT-{IP,L2,COS}-POLARVEC<b> (PolarVecIndex, src/storage/polarvec_mmap.rs): b-bit codes (b = 1..8) of the randomised
// Hadamard rotation on a per-dimension min / scale grid, the per-dimension tables of the rotated query and the scan that scores every
// code.  The rotation is RaBitQ's (rbq_signed / rbq_fwht, rabitq.h) and so is the device layout of the codes (rbq_word_index); the
// selection of the N best scores is ScoreCut and the exact rescore of those rows PoolRerank (rerank_host.inc).  DESIGN.md §23.
//   k_plv_minmax    sample rows through LDS, per-dimension min / max of each block's rows in row order (the earliest row wins a tie)
//   k_plv_fit       the per-block partials merged in block order, then dim_min / dim_scale
//   k_plv_encode    rows through LDS, the codes packed one 32-bit word per thread, one thread per row for the two correction chains
//   k_plv_query     the rotation of a query (cosine: scaled by 1 / norm first) and its table lut[d][c]
//   k_plv_scan      THE HOT KERNEL: the codes streamed once per query group as dwordx4 loads, the tables of QB queries in LDS,
//                   the lookups of a row added in one of the reference's four accumulation orders
// Every sum here is a chain of separate f32 operations in the reference's order (__fadd_rn / __fmul_rn: nothing contracts).
#pragma once

#include "rabitq.h"

namespace lynse {

// code = round-half-away((val - min) / scale) clamped to [0, levels - 1]; max / min return the operand that is not a NaN, so a NaN is 0
__device__ __forceinline__ uint32_t plv_code(float val, float mn, float sc, float lm1) {
    const float raw = __fdiv_rn(__fsub_rn(val, mn), sc);
    return (uint32_t)fminf(fmaxf(roundf(raw), 0.0f), lm1);
}
__device__ __forceinline__ float plv_dequant(float mn, float sc, uint32_t code) { return __fadd_rn(mn, __fmul_rn((float)code, sc)); }

// `rb` rows from r0 on (rows past `rows` as zeros), padded to P, signed, rotated; row r of the block lies at buf[r * P].  `step`: the
// distance between two of the block's rows in V (the sampling stride of the fit).  Ends with a barrier.
template <int NT>
__device__ __forceinline__ void plv_rotate_rows(float* buf, const float* __restrict__ V, uint32_t ld, uint32_t D, uint32_t P, uint64_t r0,
                                                uint64_t step, uint32_t rows, uint32_t rb, const uint64_t* __restrict__ sign, uint32_t tid) {
    const uint32_t total = rb * P;
    for (uint32_t e = tid; e < total; e += NT) {
        const uint32_t r = e / P, d = e % P;
        const float x = (r < rows && d < D) ? V[(r0 + (uint64_t)r * step) * ld + d] : 0.0f;
        buf[e] = rbq_signed(x, sign, d);
    }
    __syncthreads();
    rbq_fwht<NT>(buf, P, rb, tid);
}

// ---- the fit (polarvec_mmap.rs:137-208) ----
// Block b takes the sample rows [b * per, (b + 1) * per) in groups of rb; sample row si is row si * stride of V.  Thread t owns the
// dimensions t, t + NT, ...: after each rotation it runs its dimensions' strict < / > over the group's rows in row order, the running
// pair kept in the block's slot of pmin / pmax (written by no other thread).  A NaN never compares, and of two equal values (+0, -0)
// the earlier row's stays.
constexpr int PLV_FIT_NT = 256;

struct PlvMinmaxArgs {
    const float* V;
    uint32_t ld, D, P;
    uint64_t n_sample, stride, per;   // per: sample rows of one block, a multiple of rb
    uint32_t rb;
    const uint64_t* sign;
    float *pmin, *pmax;               // [blocks][P]
};

__global__ void __launch_bounds__(PLV_FIT_NT) k_plv_minmax(PlvMinmaxArgs a) {
    extern __shared__ float rbq_buf[];
    const uint32_t tid = threadIdx.x, P = a.P;
    float* pmin = a.pmin + (size_t)blockIdx.x * P;
    float* pmax = a.pmax + (size_t)blockIdx.x * P;
    const uint64_t s0 = (uint64_t)blockIdx.x * a.per;
    const uint64_t s1 = a.n_sample - s0 < a.per ? a.n_sample : s0 + a.per;
    for (uint64_t s = s0; s < s1; s += a.rb) {
        const uint32_t rows = s1 - s < a.rb ? (uint32_t)(s1 - s) : a.rb;
        if (s != s0) __syncthreads();   // (the last group's reads of the buffer)
        plv_rotate_rows<PLV_FIT_NT>(rbq_buf, a.V, a.ld, a.D, P, s * a.stride, a.stride, rows, a.rb, a.sign, tid);
        for (uint32_t d = tid; d < P; d += PLV_FIT_NT) {
            float mn = s == s0 ? INFINITY : pmin[d], mx = s == s0 ? -INFINITY : pmax[d];
            for (uint32_t r = 0; r < rows; ++r) {
                const float v = rbq_buf[(size_t)r * P + d];
                if (v < mn) mn = v;
                if (v > mx) mx = v;
            }
            pmin[d] = mn;
            pmax[d] = mx;
        }
    }
}

__global__ void __launch_bounds__(PLV_FIT_NT) k_plv_fit(const float* __restrict__ pmin, const float* __restrict__ pmax, uint32_t blocks,
                                                        uint32_t P, float lm1, float* __restrict__ dim_mins, float* __restrict__ dim_scales) {
    const uint32_t d = blockIdx.x * PLV_FIT_NT + threadIdx.x;
    if (d >= P) return;
    float mn = INFINITY, mx = -INFINITY;
    for (uint32_t b = 0; b < blocks; ++b) {
        const float lo = pmin[(size_t)b * P + d], hi = pmax[(size_t)b * P + d];
        if (lo < mn) mn = lo;
        if (hi > mx) mx = hi;
    }
    const float range = __fsub_rn(mx, mn);
    if (range > 1e-8f) {
        dim_mins[d] = __fsub_rn(mn, __fmul_rn(0.05f, range));
        dim_scales[d] = __fdiv_rn(__fmul_rn(range, __fadd_rn(1.0f, __fmul_rn(2.0f, 0.05f))), lm1);
    } else {
        dim_mins[d] = mn;
        dim_scales[d] = 1.0f;
    }
}

// ---- encode (polarvec_mmap.rs:703-777, :787-834) ----
// Block = RBQ_ENC_NT threads and `rb` rows.  The code stream of a row is LSB-first, dimension d at bits [d * bits, (d + 1) * bits):
// a thread builds one 32-bit word of one row from the dimensions that touch it (a code that spans two words is computed by both) and
// stores it whole, so the code buffer needs no zeroing and no atomics.  Thread r < rows then runs row r's two d-ascending chains.
struct PlvEncodeArgs {
    const float* V;
    uint32_t ld, D, P, bits;
    uint64_t n;
    uint32_t rb, ng;                // rows per block, 16-byte column groups of a row's code
    const uint64_t* sign;
    const float *dim_mins, *dim_scales;
    uint32_t* codes;                // device layout (rbq_word_index)
    float *residual_sq, *inv_norms; // [n] or NULL
};

__global__ void __launch_bounds__(RBQ_ENC_NT) k_plv_encode(PlvEncodeArgs a) {
    extern __shared__ float rbq_buf[];
    const uint32_t tid = threadIdx.x, P = a.P, bits = a.bits;
    const uint64_t r0 = (uint64_t)blockIdx.x * a.rb;
    const uint32_t rows = a.n - r0 < a.rb ? (uint32_t)(a.n - r0) : a.rb;
    const float lm1 = (float)((1u << bits) - 1u);
    plv_rotate_rows<RBQ_ENC_NT>(rbq_buf, a.V, a.ld, a.D, P, r0, 1, rows, a.rb, a.sign, tid);
    const uint32_t wtot = 4 * a.ng;   // every word of the row's column groups is written: zeros past the code
    for (uint32_t e = tid; e < rows * wtot; e += RBQ_ENC_NT) {
        const uint32_t r = e / wtot, w = e % wtot;
        const float* x = rbq_buf + (size_t)r * P;
        uint32_t word = 0;
        const uint32_t d0 = (32u * w) / bits;
        for (uint32_t d = d0; d < P && d * bits < 32u * w + 32u; ++d) {
            const uint32_t c = plv_code(x[d], a.dim_mins[d], a.dim_scales[d], lm1);
            const int sh = (int)(d * bits) - (int)(32u * w);
            word |= sh >= 0 ? c << sh : c >> -sh;
        }
        a.codes[rbq_word_index(r0 + r, w, a.ng)] = word;
    }
    if (tid < rows && (a.residual_sq || a.inv_norms)) {
        const float* x = rbq_buf + (size_t)tid * P;
        float res = 0.0f, vh = 0.0f;
        for (uint32_t d = 0; d < P; ++d) {
            const float mn = a.dim_mins[d], sc = a.dim_scales[d], val = x[d];
            const float v_hat = plv_dequant(mn, sc, plv_code(val, mn, sc, lm1));
            const float diff = __fsub_rn(val, v_hat);
            res = __fadd_rn(res, __fmul_rn(diff, diff));
            vh = __fadd_rn(vh, __fmul_rn(v_hat, v_hat));
        }
        if (a.residual_sq) a.residual_sq[r0 + tid] = res;
        if (a.inv_norms) a.inv_norms[r0 + tid] = __fdiv_rn(1.0f, fmaxf(__fsqrt_rn(vh), 1e-12f));
    }
}

// ---- query transform (polarvec_mmap.rs:310-332, :926-972) ----
// blockIdx.x = the query; each of its gridDim.y workgroups rotates the query into LDS and writes the table entries e = y * NT + tid,
// + gridDim.y * NT, ...: lut[q][d * levels + c] from v = dim_min[d] + (float)c * dim_scale[d] — IP q * v, L2 (q - v)^2, cosine -(q * v).
// For cosine the query is divided by max(sqrt(sum x^2), 1e-12) first; the sum is one thread's chain.
__device__ __forceinline__ float plv_lut_entry(float q, float mn, float sc, uint32_t c, int metric) {
    const float v = plv_dequant(mn, sc, c);
    if (metric == M_L2) {
        const float diff = __fsub_rn(q, v);
        return __fmul_rn(diff, diff);
    }
    const float p = __fmul_rn(q, v);
    return metric == M_COS ? -p : p;
}

__global__ void __launch_bounds__(RBQ_Q_NT) k_plv_query(const float* __restrict__ Q, uint32_t D, uint32_t P, uint32_t bits, int metric,
                                                        const uint64_t* __restrict__ sign, const float* __restrict__ dim_mins,
                                                        const float* __restrict__ dim_scales, float* __restrict__ lut) {
    extern __shared__ float rbq_buf[];
    const uint32_t tid = threadIdx.x, q = blockIdx.x;
    const float* x = Q + (size_t)q * D;
    float qn = 1.0f;
    if (metric == M_COS) {   // (the norm passes through the first word of the buffer: no static LDS beside a 160 KiB dynamic request)
        if (tid == 0) {
            float s = 0.0f;
            for (uint32_t d = 0; d < D; ++d) s = __fadd_rn(s, __fmul_rn(x[d], x[d]));
            rbq_buf[0] = fmaxf(__fsqrt_rn(s), 1e-12f);
        }
        __syncthreads();
        qn = rbq_buf[0];
        __syncthreads();
    }
    for (uint32_t d = tid; d < P; d += RBQ_Q_NT) {
        float v = d < D ? x[d] : 0.0f;
        if (metric == M_COS && d < D) v = __fdiv_rn(v, qn);
        rbq_buf[d] = rbq_signed(v, sign, d);
    }
    __syncthreads();
    rbq_fwht<RBQ_Q_NT>(rbq_buf, P, 1, tid);
    const uint32_t E = P << bits;
    float* lq = lut + (size_t)q * E;
    for (uint32_t e = blockIdx.y * RBQ_Q_NT + tid; e < E; e += gridDim.y * RBQ_Q_NT) {
        const uint32_t d = e >> bits, c = e & ((1u << bits) - 1u);
        lq[e] = plv_lut_entry(rbq_buf[d], dim_mins[d], dim_scales[d], c, metric);
    }
}

// ---- the scan (compute_lut_score_row + scan_topn's epilogue, polarvec_mmap.rs:1010-1135, :1202-1207) ----
// Block = PLV_NT threads x PLV_R rows each, blockIdx.y = a group of QB queries.  The tables go through LDS in chunks of `cu` units,
// entry-major with the QB queries of an entry side by side (QB = 4: one ds_read_b128 fetches an entry of all four); the running sums
// of every (query, row) stay in registers across the chunks.  A unit is a whole number of 16-byte column groups AND of dimensions:
//   PLV_BYTE   bits 8: 16 bytes = 16 dimensions of 256 entries.  Byte b adds lut[b][code_b] to s[b % 4].
//   PLV_B4     bits 4: 16 bytes = 32 dimensions of 16 entries.  Byte b adds lut[2b][low nibble] + lut[2b + 1][high nibble] (the second
//              only if 2b + 1 < P) to s[b % 4]: one f32 add of the operands of the reference's byte table bl[b][v], so the same bits.
//              In both, a code of fewer than 4 bytes goes to s0 alone ("leftover bytes").
//   PLV_B3     bits 3: 48 bytes = 128 dimensions of 8 entries, in groups of 8 dimensions = 3 bytes; dimension j of a group adds to
//              s[j % 4]; P / 8 groups, none below P = 8 (every table sum is then 0.0f).
//   PLV_GEN    bits 1, 2, 5, 6, 7: 16 * bits bytes = 128 dimensions of 2^bits entries; one chain over d.
// The score is ((s0 + s1) + s2) + s3 (PLV_GEN: s), + corr[row] when corr, * mult[row] when mult.  Output: the score_ord image S[q][row].
constexpr int PLV_NT = 512;
constexpr int PLV_R = 4;
enum { PLV_BYTE = 0, PLV_B4 = 1, PLV_B3 = 2, PLV_GEN = 3 };

struct PlvScanArgs {
    const uint4* codes;     // device layout
    uint64_t n;
    uint32_t P, bits, cb, ng;
    uint32_t cu, ub, ue;    // units per LDS chunk; bytes and table entries of a unit
    const float* lut;       // [nq][P << bits]
    uint32_t nq;
    int asc;
    const float *corr, *mult;   // [n] or NULL
    uint32_t* S;            // [nq][n]
};

template <int QB> struct PlvVec;
template <> struct PlvVec<1> {
    float v;
    __device__ __forceinline__ void zero() { v = 0.0f; }
    __device__ __forceinline__ void add(const PlvVec& o) { v = __fadd_rn(v, o.v); }
    __device__ __forceinline__ float at(int) const { return v; }
};
template <> struct __attribute__((aligned(16))) PlvVec<4> {
    float x, y, z, w;
    __device__ __forceinline__ void zero() { x = y = z = w = 0.0f; }
    __device__ __forceinline__ void add(const PlvVec& o) {
        x = __fadd_rn(x, o.x); y = __fadd_rn(y, o.y); z = __fadd_rn(z, o.z); w = __fadd_rn(w, o.w);
    }
    __device__ __forceinline__ float at(int j) const { return j == 0 ? x : (j == 1 ? y : (j == 2 ? z : w)); }
};

template <int CLS, int QB>
__global__ void __launch_bounds__(PLV_NT) k_plv_scan(PlvScanArgs a) {
    extern __shared__ __attribute__((aligned(16))) float plv_lut[];
    using Vec = PlvVec<QB>;
    constexpr int NACC = CLS == PLV_GEN ? 1 : 4;
    Vec* tab = reinterpret_cast<Vec*>(plv_lut);
    const uint32_t tid = threadIdx.x, q0 = blockIdx.y * QB;
    const uint32_t nqb = a.nq - q0 < (uint32_t)QB ? a.nq - q0 : (uint32_t)QB;
    const uint64_t base = (uint64_t)blockIdx.x * PLV_NT * PLV_R;
    const uint32_t E = a.P << a.bits;
    const uint32_t mc = a.cu * a.ub, ce = a.cu * a.ue;   // bytes and entries of a chunk
    const bool one = a.cb < 4;                           // no full group of four bytes: every byte goes to s0
    Vec acc[PLV_R][NACC];
#pragma unroll
    for (int r = 0; r < PLV_R; ++r)
#pragma unroll
        for (int s = 0; s < NACC; ++s) acc[r][s].zero();
    for (uint32_t b0 = 0, e0 = 0; b0 < a.cb; b0 += mc, e0 += ce) {
        const uint32_t mcc = a.cb - b0 < mc ? a.cb - b0 : mc;   // code bytes of this chunk
        const uint32_t nent = E - e0 < ce ? E - e0 : ce;        // its table entries
        if (b0) __syncthreads();
        for (uint32_t w = tid; w < nent; w += PLV_NT) {
            Vec v;
            if constexpr (QB == 1) {
                v.v = a.lut[(size_t)q0 * E + e0 + w];
            } else {
                v.x = a.lut[(size_t)q0 * E + e0 + w];
                v.y = 1 < nqb ? a.lut[(size_t)(q0 + 1) * E + e0 + w] : 0.0f;
                v.z = 2 < nqb ? a.lut[(size_t)(q0 + 2) * E + e0 + w] : 0.0f;
                v.w = 3 < nqb ? a.lut[(size_t)(q0 + 3) * E + e0 + w] : 0.0f;
            }
            tab[w] = v;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < PLV_R; ++r) {
            const uint64_t row = base + (uint64_t)r * PLV_NT + tid;   // rows past n are not stored
            if (row >= a.n) continue;
            const uint4* cr = a.codes + ((size_t)(row >> 6) * a.ng << 6) + (row & 63u) + ((size_t)(b0 >> 4) << 6);
            if constexpr (CLS == PLV_BYTE || CLS == PLV_B4) {
                const bool odd = a.P > 1;   // (PLV_B4: dimension 2b + 1 exists)
                for (uint32_t bb = 0; bb < mcc; bb += 16) {
                    const uint4 c = cr[(size_t)(bb >> 4) << 6];
                    const uint32_t w4[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        if (bb + i < mcc) {
                            const uint32_t code = (w4[i >> 2] >> (8 * (i & 3))) & 0xffu;
                            Vec t;
                            if constexpr (CLS == PLV_BYTE) {
                                t = tab[(bb + i) * 256 + code];
                            } else {
                                t = tab[(bb + i) * 32 + (code & 15u)];
                                if (odd) t.add(tab[(bb + i) * 32 + 16 + (code >> 4)]);
                            }
                            if (one) acc[r][0].add(t);
                            else acc[r][i & 3].add(t);
                        }
                    }
                }
            } else if constexpr (CLS == PLV_B3) {
                const uint32_t groups = (a.P >> 3) - (e0 >> 6);   // groups of 8 dimensions from this chunk's first on (64 entries each)
                for (uint32_t u = 0; u < a.cu && u * 16 < groups; ++u) {
                    uint32_t w12[12];
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        const uint4 c = (uint32_t)(u * 3 + k) * 16 < mcc ? cr[(size_t)(u * 3 + k) << 6] : make_uint4(0, 0, 0, 0);
                        w12[4 * k] = c.x; w12[4 * k + 1] = c.y; w12[4 * k + 2] = c.z; w12[4 * k + 3] = c.w;
                    }
#pragma unroll
                    for (int g = 0; g < 16; ++g) {
                        if (u * 16 + g < groups) {
                            const int wi = (24 * g) >> 5, sh = (24 * g) & 31;
                            uint32_t w = w12[wi] >> sh;
                            if (sh > 8) w |= w12[wi + 1] << (32 - sh);
#pragma unroll
                            for (int j = 0; j < 8; ++j)
                                acc[r][j & 3].add(tab[((u * 16 + g) * 8 + j) * 8 + ((w >> (3 * j)) & 7u)]);
                        }
                    }
                }
            } else {
                const uint32_t bits = a.bits, mask = (1u << bits) - 1u;
                const uint32_t d0 = e0 >> bits;
                const uint32_t dend = a.P - d0 < a.cu * 128 ? a.P - d0 : a.cu * 128;   // dimensions of this chunk
                const uint32_t g16 = (mcc + 15) >> 4;                                   // its 16-byte groups
                uint64_t buf = 0;
                uint32_t have = 0, d = 0;
                for (uint32_t g = 0; g < g16 && d < dend; ++g) {
                    const uint4 c = cr[(size_t)g << 6];
                    const uint32_t w4[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        buf |= (uint64_t)w4[k] << have;
                        have += 32;
                        while (have >= bits && d < dend) {
                            acc[r][0].add(tab[(d << bits) + ((uint32_t)buf & mask)]);
                            buf >>= bits;
                            have -= bits;
                            ++d;
                        }
                    }
                }
            }
        }
    }
    const bool asc = a.asc != 0;
#pragma unroll
    for (int r = 0; r < PLV_R; ++r) {
        const uint64_t row = base + (uint64_t)r * PLV_NT + tid;
        if (row >= a.n) continue;
        if constexpr (NACC == 4) {
            acc[r][0].add(acc[r][1]);
            acc[r][0].add(acc[r][2]);
            acc[r][0].add(acc[r][3]);
        }
        const float corr = a.corr ? a.corr[row] : 0.0f, mult = a.mult ? a.mult[row] : 0.0f;
#pragma unroll
        for (int j = 0; j < QB; ++j) {
            if ((uint32_t)j < nqb) {
                float s = acc[r][0].at(j);
                if (a.corr) s = __fadd_rn(s, corr);
                if (a.mult) s = __fmul_rn(s, mult);
                a.S[(size_t)(q0 + j) * a.n + row] = score_ord(s, asc);
            }
        }
    }
}

}  // namespace lynse
