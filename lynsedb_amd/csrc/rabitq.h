// rabitq.h — FLAT-{IP,L2,COS}-RABITQ (RaBitQIndex, src/storage/rabitq_mmap.rs): 1-bit codes of the randomised Hadamard rotation,
// the per-byte tables of the rotated query and the scan that scores every code.  The selection of the N best scores is
// k_pq_hist / k_pq_find / k_pq_emit (pq.h), the exact rescore of those rows k_pool_rerank (kernels.h).  DESIGN.md §15.
//   k_rbq_encode    rows through LDS: signs, FWHT (stages separated by barriers), bits packed by wave ballot, the row norm
//   k_rbq_query     the same rotation of a query, total_q and the byte tables lut[q][b][v]
//   k_rbq_scan      THE HOT KERNEL: the codes streamed once per query group as dwordx4 loads, the tables of QB queries in LDS,
//                   one thread adds a row's byte lookups in ascending byte order and finishes the score
// Every sum here is a chain of separate f32 operations in the reference's order (__fadd_rn / __fmul_rn: nothing contracts).
#pragma once

#include "pq.h"

namespace lynse {

// The device layout of the codes.  A row's code is wpr = ceil(code_bytes / 4) 32-bit words (zero bits past code_bytes), grouped into
// ng = ceil(wpr / 4) column groups of 16 bytes; rows go in tiles of 64.  Group g of tile t is 64 consecutive uint4, one per row
// of the tile: a wave that holds one row per lane loads a group with ONE contiguous 1 KiB dwordx4 access.
//   word w of row r  ->  dev32[(((r / 64) * ng + w / 4) * 64 + r % 64) * 4 + w % 4]
// [n][code_bytes] is only the export and file layout.
__host__ __device__ inline size_t rbq_word_index(uint64_t row, uint32_t w, uint32_t ng) {
    return ((((size_t)(row >> 6) * ng + (w >> 2)) << 6) + (size_t)(row & 63u)) * 4 + (w & 3u);
}

// x[i] = -x[i] where bit i % 64 of sign word i / 64 is set, then the in-place unnormalised FWHT (rabitq_mmap.rs:345-377) of
// `rows` vectors of P floats that lie back to back in LDS.  P is a power of two, so the butterflies of a stage h < P never cross
// a vector: the stage runs over the whole array.  Each butterfly is (x + y, x - y) with x the lower index; the butterflies of a
// stage are independent, so the result carries the bits of the sequential loop.  Ends with a barrier.
template <int NT>
__device__ __forceinline__ void rbq_fwht(float* buf, uint32_t P, uint32_t rows, uint32_t tid) {
    const uint32_t half = rows * P / 2;
    for (uint32_t h = 1, sh = 0; h < P; h <<= 1, ++sh) {
        for (uint32_t t = tid; t < half; t += NT) {
            const uint32_t i = ((t >> sh) << (sh + 1)) + (t & (h - 1u));
            const float x = buf[i], y = buf[i + h];
            buf[i] = __fadd_rn(x, y);
            buf[i + h] = __fsub_rn(x, y);
        }
        __syncthreads();
    }
}

__device__ __forceinline__ float rbq_signed(float x, const uint64_t* __restrict__ sign, uint32_t i) {
    return ((sign[i >> 6] >> (i & 63u)) & 1ull) ? -x : x;
}

// Encode (rabitq_mmap.rs:101-132).  Block = RBQ_ENC_NT threads and `rb` rows (rb * P floats of LDS).  norm = sqrt of the f32 sum of
// x * x in ascending index order from 0.0f: thread r < rb runs the chain of row r from LDS, the signs taken off again.
// Bit d % 8 of byte d / 8 is buf[d] >= 0.0f (-0.0 sets it, NaN does not): a wave's ballot over 64 consecutive elements is two
// code words of one row (P >= 64) or the whole codes of 64 / P rows (P < 64).  The code buffer is zeroed beforehand.
constexpr int RBQ_ENC_NT = 256;

struct RbqEncodeArgs {
    const float* V;         // [n] rows, pitch ld
    uint32_t ld, D, P;
    uint64_t n;
    uint32_t rb;            // rows per block
    uint32_t ng;
    const uint64_t* sign;   // [ceil(P / 64)]
    uint32_t* codes;        // device layout (rbq_word_index)
    float* norms;           // [n]
};

__global__ void __launch_bounds__(RBQ_ENC_NT) k_rbq_encode(RbqEncodeArgs a) {
    extern __shared__ float rbq_buf[];
    const uint32_t tid = threadIdx.x, P = a.P;
    const uint64_t r0 = (uint64_t)blockIdx.x * a.rb;
    const uint32_t rows = a.n - r0 < a.rb ? (uint32_t)(a.n - r0) : a.rb;
    const uint32_t total = a.rb * P;
    for (uint32_t e = tid; e < total; e += RBQ_ENC_NT) {
        const uint32_t r = e / P, d = e % P;
        const float x = (r < rows && d < a.D) ? a.V[(r0 + r) * a.ld + d] : 0.0f;
        rbq_buf[e] = rbq_signed(x, a.sign, d);
    }
    __syncthreads();
    if (tid < rows) {
        const float* x = rbq_buf + (size_t)tid * P;
        float s = 0.0f;
        for (uint32_t d = 0; d < a.D; ++d) {
            const float v = rbq_signed(x[d], a.sign, d);
            s = __fadd_rn(s, __fmul_rn(v, v));
        }
        a.norms[r0 + tid] = __fsqrt_rn(s);
    }
    __syncthreads();
    rbq_fwht<RBQ_ENC_NT>(rbq_buf, P, a.rb, tid);
    const uint32_t lane = tid & 63u;
    for (uint32_t e0 = tid - lane; e0 < total; e0 += RBQ_ENC_NT) {   // e0: the wave's first element, uniform in the wave
        const uint32_t e = e0 + lane;
        const uint64_t m = __ballot(e < total && rbq_buf[e] >= 0.0f);
        if (P >= 64) {
            const uint32_t r = e0 / P, w = (e0 % P) >> 5;
            if (lane < 2 && r < rows) a.codes[rbq_word_index(r0 + r, w + lane, a.ng)] = (uint32_t)(m >> (32 * lane));
        } else {
            const uint32_t r = e0 / P + lane;
            if (lane < 64 / P && r < rows) a.codes[rbq_word_index(r0 + r, 0, a.ng)] = (uint32_t)((m >> (lane * P)) & ((1ull << P) - 1ull));
        }
    }
}

// Query transform (rabitq_mmap.rs:202-213, :387-407).  blockIdx.x = the query; its blockIdx.y < gridDim.y - 1 workgroups each rotate
// the query into LDS (the rotation is cheap next to the tables) and write the tables of the bytes b = y, y + (gridDim.y - 1), ...:
// thread v adds lut[b][v] = the f32 sum from 0.0f of q_rot[8 b + bit] over the set bits of v in ascending bit order (a clear bit
// adds +0.0f, which leaves a sum that started at +0.0f unchanged bit for bit).  The last workgroup's thread 0 runs total_q = the f32
// sum of all P rotated values in ascending order, one dependent chain.
constexpr int RBQ_Q_NT = 256;

__global__ void __launch_bounds__(RBQ_Q_NT) k_rbq_query(const float* __restrict__ Q, uint32_t D, uint32_t P, uint32_t cb,
                                                        const uint64_t* __restrict__ sign, float* __restrict__ lut,
                                                        float* __restrict__ total) {
    extern __shared__ float rbq_buf[];
    const uint32_t tid = threadIdx.x, q = blockIdx.x, parts = gridDim.y - 1;
    for (uint32_t d = tid; d < P; d += RBQ_Q_NT) rbq_buf[d] = rbq_signed(d < D ? Q[(size_t)q * D + d] : 0.0f, sign, d);
    __syncthreads();
    rbq_fwht<RBQ_Q_NT>(rbq_buf, P, 1, tid);
    if (blockIdx.y == parts) {
        if (tid == 0) {
            float s = 0.0f;
            if (P >= 4) {
                const float4* b4 = reinterpret_cast<const float4*>(rbq_buf);
#pragma unroll 8
                for (uint32_t i = 0; i < P / 4; ++i) {
                    const float4 v = b4[i];
                    s = __fadd_rn(__fadd_rn(__fadd_rn(__fadd_rn(s, v.x), v.y), v.z), v.w);
                }
            } else {
                for (uint32_t d = 0; d < P; ++d) s = __fadd_rn(s, rbq_buf[d]);
            }
            total[q] = s;
        }
        return;
    }
    float* lq = lut + (size_t)q * cb * 256;
    for (uint32_t b = blockIdx.y; b < cb; b += parts) {
        float s = 0.0f;
#pragma unroll
        for (uint32_t bit = 0; bit < 8; ++bit) {
            const float x = b * 8 + bit < P ? rbq_buf[b * 8 + bit] : 0.0f;   // (the same address in every lane: a broadcast)
            s = __fadd_rn(s, ((tid >> bit) & 1u) ? x : 0.0f);
        }
        lq[(size_t)b * 256 + tid] = s;
    }
}

// The scan (compute_binary_score, rabitq_mmap.rs:560-585).  Block = RBQ_NT threads x RBQ_R rows each, blockIdx.y = a group of QB
// queries.  The tables go through LDS as [QB][mc][256] f32, mc bytes of the code per chunk (a multiple of 16 unless the whole code
// is shorter), the running sums of every (query, row) stay in registers across the chunks.  A thread loads 16 bytes of its row
// per column group (the wave: one contiguous KiB) and adds lut[b][code[b]] in ascending b:
//   sum_set = 0.0f + lut[0][c0] + lut[1][c1] + ...;  ip_raw = 2 sum_set - total_q
//   IP: ip_raw * norm (largest first);  L2 / cosine: norm * norm - ((2 ip_raw) * norm) / (float)P (smallest first)
// Output: the score_ord image, S[q][row].
constexpr int RBQ_NT = 512;
constexpr int RBQ_R = 4;

struct RbqScanArgs {
    const uint4* codes;     // device layout
    const float* norms;     // [n]
    uint64_t n;
    uint32_t cb, ng, mc;    // code bytes, column groups, bytes per LDS chunk
    float fP;               // (float)padded_dim
    const float* lut;       // [nq][cb][256]
    const float* total;     // [nq]
    uint32_t nq;
    int asc;
    uint32_t* S;            // [nq][n]
};

template <int QB>
__global__ void __launch_bounds__(RBQ_NT) k_rbq_scan(RbqScanArgs a) {
    extern __shared__ float rbq_lut[];
    const uint32_t tid = threadIdx.x, q0 = blockIdx.y * QB;
    const uint32_t nqb = a.nq - q0 < (uint32_t)QB ? a.nq - q0 : (uint32_t)QB;
    const uint64_t base = (uint64_t)blockIdx.x * RBQ_NT * RBQ_R;
    float acc[QB][RBQ_R];
#pragma unroll
    for (int j = 0; j < QB; ++j)
#pragma unroll
        for (int r = 0; r < RBQ_R; ++r) acc[j][r] = 0.0f;
    for (uint32_t b0 = 0; b0 < a.cb; b0 += a.mc) {
        const uint32_t mcc = a.cb - b0 < a.mc ? a.cb - b0 : a.mc;
        if (b0) __syncthreads();
        for (uint32_t i = tid; i < (uint32_t)QB * mcc * 256; i += RBQ_NT) {
            const uint32_t j = i / (mcc * 256), w = i % (mcc * 256);
            rbq_lut[j * a.mc * 256 + w] = j < nqb ? a.lut[((size_t)(q0 + j) * a.cb + b0) * 256 + w] : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < RBQ_R; ++r) {
            const uint64_t row = base + (uint64_t)r * RBQ_NT + tid;   // rows past n are zero codes of the padded last tile: not stored
            if (row >= a.n) continue;
            const uint4* cr = a.codes + ((size_t)(row >> 6) * a.ng << 6) + (row & 63u);
            for (uint32_t bb = 0; bb < mcc; bb += 16) {
                const uint4 c = cr[(size_t)((b0 + bb) >> 4) << 6];
                const uint32_t w4[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    if (bb + i < mcc) {
                        const uint32_t off = (bb + i) * 256 + ((w4[i >> 2] >> (8 * (i & 3))) & 0xffu);
#pragma unroll
                        for (int j = 0; j < QB; ++j) acc[j][r] = __fadd_rn(acc[j][r], rbq_lut[j * a.mc * 256 + off]);
                    }
                }
            }
        }
    }
    const bool asc = a.asc != 0;
#pragma unroll
    for (int r = 0; r < RBQ_R; ++r) {
        const uint64_t row = base + (uint64_t)r * RBQ_NT + tid;
        if (row >= a.n) continue;
        const float norm = a.norms[row];
#pragma unroll
        for (int j = 0; j < QB; ++j) {
            if ((uint32_t)j < nqb) {
                const float ip_raw = __fsub_rn(__fmul_rn(2.0f, acc[j][r]), a.total[q0 + j]);
                const float s = asc ? __fsub_rn(__fmul_rn(norm, norm), __fdiv_rn(__fmul_rn(__fmul_rn(2.0f, ip_raw), norm), a.fP))
                                    : __fmul_rn(ip_raw, norm);
                a.S[(size_t)(q0 + j) * a.n + row] = score_ord(s, asc);
            }
        }
    }
}

}  // namespace lynse
