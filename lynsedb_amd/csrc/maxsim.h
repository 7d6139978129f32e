// maxsim.h — multi-vector (late interaction) search: score(Q, P) = sum_i max_j <q_i, p_j> over the query tokens q_i and the tokens
// p_j of a record.  The cut and the order are the shared ones (ScoreCut, k_pool_select / select_pool_keys).  DESIGN.md §28.
//   k_maxsim_scan   one WAVE owns one range of whole records (the host's table, ~2,048 tokens each) and walks its token stream in
//                   blocks of 32 consecutive token rows, whatever records they belong to.  The query's tokens are the A operand,
//                   stationary in LDS for the workgroup; a block is the B operand, double-buffered in the wave's own LDS; the 32 x 32
//                   score block is accumulated over the columns with v_mfma_f32_32x32x2_f32.  In the accumulator a lane holds ONE
//                   token column and 16 of the 32 query rows, so the max over a record's tokens is a segmented max across the 32
//                   column lanes (ds_bpermute steps keyed by the record boundaries), a record that runs on into the next block
//                   carries its row maxima in registers, and when a record ends its row maxima are added in query-token order.
// It writes S[q][c] = the score_ord image (descending) of the score of the c-th record THAT HAS TOKENS, RANGE_FAIL when the mask
// leaves that record out.  No two waves touch one record: no atomics, no second pass.
#pragma once

#include "range.h"

namespace lynse {

constexpr uint32_t MAXSIM_BLOCK = 32;        // token rows of a block = columns of the MFMA tile
constexpr uint32_t MAXSIM_KC = 32;           // columns of a k chunk: 4 k-steps of 8 columns, 16 MFMAs; the row pitch is a multiple of it
constexpr uint32_t MAXSIM_RANGE = 2048;      // tokens of a wave range (the host's target)
constexpr uint32_t MAXSIM_MAX_TQ = 256;      // query tokens: 8 tiles of 32 rows, their carried maxima are 128 registers
constexpr uint32_t MAXSIM_MAX_DIM = 1024;
constexpr uint32_t MAXSIM_MAX_WAVES = 4;     // waves of a workgroup (one per SIMD: the LDS of a CU holds no more blocks at 128 columns)

// the row pitch of the token array in HBM and of the padded queries: the dimension rounded up to whole k chunks, zero filled
__host__ __device__ inline uint32_t maxsim_ld(uint32_t dim) { return (dim + MAXSIM_KC - 1u) / MAXSIM_KC * MAXSIM_KC; }
// LDS row pitch in floats, for the query rows and the block rows alike: ld + 4 = 4 s with s odd (ld / 4 is even).  Banks
// (MI355X_MICROARCH.md, LDS: a ds_read_b128 is served in four groups of 16 lanes over the 16 16-B slots of a 256-B bank row): the
// lanes of a group read the same 16-B column piece of 16 consecutive rows, slots r * s + c; with s odd these are 16 different slots
// mod 16, so the A and the B fragment reads are conflict-free.  (The staging stores put 8 consecutive pieces of two rows into a
// group: rows one slot apart mod 8, a 2-way conflict on a sixteenth of the LDS traffic.)
__host__ __device__ inline uint32_t maxsim_pitch(uint32_t ld) { return ld + 4u; }
// LDS floats: the query tiles | per wave: two blocks and the 32 boundary flags
__host__ __device__ inline size_t maxsim_lds_bytes(uint32_t ld, uint32_t tiles, uint32_t waves) {
    const size_t blk = (size_t)MAXSIM_BLOCK * maxsim_pitch(ld);
    return ((size_t)tiles * blk + (size_t)waves * (2u * blk + MAXSIM_BLOCK)) * 4u;
}

struct MaxSimArgs {
    const float* tokens;      // [total tokens][ld], columns dim .. ld - 1 are zero
    uint32_t ld;
    const uint64_t* cptr;     // m + 1 token offsets of the records that have tokens
    const uint32_t* crec;     // m: their record rows (the mask is over record rows)
    uint64_t m;
    const uint32_t* ranges;   // n_ranges + 1: range r holds the records ranges[r] .. ranges[r + 1] - 1 (indices into cptr)
    uint32_t n_ranges;
    const float* Q;           // the chunk's queries, each [round_up(tq, 32)][ld] and zero padded
    const uint64_t* qdesc;    // per query: its offset into Q in floats, its token count tq
    const uint64_t* mask;     // NULL = every record
    uint64_t mask_words;
    uint32_t* S;              // [nq][m]
};

// no packed f32 arithmetic in the scan: rule 4 adds one row maximum at a time (the host pass does not know the feature)
#if defined(__HIP_DEVICE_COMPILE__)
#define LY_MAXSIM_FN __attribute__((target("no-packed-fp32-ops")))
#else
#define LY_MAXSIM_FN
#endif

__device__ __forceinline__ uint32_t maxsim_uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint64_t maxsim_uniform(uint64_t v) {
    return ((uint64_t)maxsim_uniform((uint32_t)(v >> 32)) << 32) | maxsim_uniform((uint32_t)v);
}
__device__ __forceinline__ float maxsim_from_lane(float v, uint32_t src_lane) {
    return __int_as_float(__builtin_amdgcn_ds_bpermute((int)(src_lane << 2), __float_as_int(v)));
}
// the wave's own LDS buffers need no workgroup barrier: the stores of this wave are ordered before its later reads
__device__ __forceinline__ void maxsim_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One k chunk of a block: the 256 16-B pieces [32 rows][8 pieces], four per lane — 8 lanes read 128 contiguous bytes of a row.
// Rows at or past `t_end` (the end of the wave's range) are zero: nothing outside the range is read.
__device__ __forceinline__ void maxsim_load_chunk(const MaxSimArgs& a, uint64_t t_first, uint64_t t_end, uint32_t kc, uint32_t lane, f32x4 (&pre)[4]) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const uint32_t p = (uint32_t)u * 64u + lane, row = p >> 3, c4 = p & 7u;
        pre[u] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        if (t_first + row < t_end) pre[u] = *reinterpret_cast<const f32x4*>(a.tokens + (size_t)(t_first + row) * a.ld + kc + c4 * 4u);
    }
}
__device__ __forceinline__ void maxsim_store_chunk(float* blk, uint32_t P, uint32_t kc, uint32_t lane, const f32x4 (&pre)[4]) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const uint32_t p = (uint32_t)u * 64u + lane, row = p >> 3, c4 = p & 7u;
        *reinterpret_cast<f32x4*>(blk + (size_t)row * P + kc + c4 * 4u) = pre[u];
    }
}

// NT = query tiles of 32 rows the LDS holds (1, 2, 4 or 8); a query of fewer tiles skips the rest.  grid.x strides over the ranges,
// grid.y is the query; blockDim.x / 64 waves.
template <int NT>
__global__ void LY_MAXSIM_FN __launch_bounds__(MAXSIM_MAX_WAVES * 64) k_maxsim_scan(MaxSimArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm_maxsim[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, col = lane & 31u, half = lane >> 5;
    const uint32_t wave = maxsim_uniform(tid >> 6), waves = blockDim.x >> 6;
    const uint32_t K = a.ld, P = maxsim_pitch(K), BLK = MAXSIM_BLOCK * P;
    const uint32_t q = blockIdx.y;
    const uint64_t q_off = a.qdesc[2u * q];
    const uint32_t tq = (uint32_t)a.qdesc[2u * q + 1u], tq_rows = (tq + 31u) / 32u * 32u;
    float* q_l = sm_maxsim;
    float* buf = q_l + (size_t)NT * BLK + (size_t)wave * (2u * BLK + MAXSIM_BLOCK);
    uint32_t* flag_l = reinterpret_cast<uint32_t*>(buf + 2u * BLK);
    // the query tiles, zero rows past the query's own
    const uint32_t c4n = K / 4u;
    for (uint32_t p = tid; p < (uint32_t)NT * 32u * c4n; p += blockDim.x) {
        const uint32_t r = p / c4n, c = p - r * c4n;
        f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
        if (r < tq_rows) v = *reinterpret_cast<const f32x4*>(a.Q + q_off + (size_t)r * K + c * 4u);
        *reinterpret_cast<f32x4*>(q_l + (size_t)r * P + c * 4u) = v;
    }
    __syncthreads();   // the only workgroup barrier: from here on the waves run their own ranges
    const float NINF = -__builtin_huge_valf();
    for (uint32_t r = blockIdx.x * waves + wave; r < a.n_ranges; r += gridDim.x * waves) {
        const uint32_t ca = maxsim_uniform(a.ranges[r]), cb = maxsim_uniform(a.ranges[r + 1u]);
        const uint64_t t0 = maxsim_uniform(a.cptr[ca]), t1 = maxsim_uniform(a.cptr[cb]);
        const uint32_t nb = (uint32_t)((t1 - t0 + MAXSIM_BLOCK - 1u) / MAXSIM_BLOCK);
        for (uint32_t kc = 0; kc < K; kc += MAXSIM_KC) {   // the first block of the range, not overlapped
            f32x4 pre[4];
            maxsim_load_chunk(a, t0, t1, kc, lane, pre);
            maxsim_store_chunk(buf, P, kc, lane, pre);
        }
        maxsim_wave_sync();
        uint32_t rc0 = ca;       // the record of the block's first token
        float carry[NT][16];     // the row maxima of the record that runs on from the previous block (read at column 0 only)
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int v = 0; v < 16; ++v) carry[t][v] = NINF;
        for (uint32_t b = 0; b < nb; ++b) {
            const uint64_t tb = t0 + (uint64_t)b * MAXSIM_BLOCK;
            const float* cur = buf + (size_t)(b & 1u) * BLK;
            float* nxt = buf + (size_t)((b + 1u) & 1u) * BLK;
            const bool more = b + 1u < nb;
            // the ends of the records from rc0 on: at most 32 of them fall into (tb, tb + 32]; the load lands under the MFMAs
            uint64_t rec_end = ~0ull;
            if (lane < 32u && (uint64_t)rc0 + 1u + lane <= cb) rec_end = a.cptr[rc0 + 1u + lane];
            uint32_t starts = 0u, endmask = 0u, n_adv = 0u;   // wave-uniform once tile 0 has set them
            bool open_next = false;
            uint32_t ok_d = 0u;   // bit i: the lane 2^i columns down is in the same record
            float s = 0.0f;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                if (t != 0 && (uint32_t)t * 32u >= tq) continue;
                f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
                const float* qa = q_l + (size_t)((uint32_t)t * 32u + col) * P + half * 4u;
                const float* pb = cur + (size_t)col * P + half * 4u;
                for (uint32_t kc = 0; kc < K; kc += MAXSIM_KC) {
                    f32x4 pre[4];
                    if (t == 0 && more) maxsim_load_chunk(a, tb + MAXSIM_BLOCK, t1, kc, lane, pre);   // the next block, under this chunk's MFMAs
#pragma unroll
                    for (uint32_t ks = 0; ks < MAXSIM_KC; ks += 8u) {
                        // a k-step of 8 columns: lane (row or column, half) holds columns 4 half .. 4 half + 3 of it, so MFMA e multiplies
                        // the column pair (e, 4 + e) — the same pairing on both operands, and the order of a sum is not part of the contract
                        const f32x4 av = *reinterpret_cast<const f32x4*>(qa + kc + ks);
                        const f32x4 bv = *reinterpret_cast<const f32x4*>(pb + kc + ks);
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[e], bv[e], acc, 0, 0, 0);
                    }
                    if (t == 0 && more) maxsim_store_chunk(nxt, P, kc, lane, pre);
                }
                if (t == 0) {
                    // the record boundaries of the block as a bit mask: bit j = a record begins at column j (1 <= j <= 31)
                    const uint64_t rel64 = rec_end - tb;   // >= 1; ~0 - tb stays huge
                    const uint32_t rel = rel64 > 64u ? 64u : (uint32_t)rel64;
                    if (lane < 32u) flag_l[lane] = 0u;
                    maxsim_wave_sync();
                    if (lane < 32u && rel < 32u) flag_l[rel] = 1u;   // (the ends ascend strictly: one lane per flag)
                    maxsim_wave_sync();
                    starts = (uint32_t)__ballot(flag_l[col] != 0u);
                    const bool end32 = __ballot(lane < 32u && rel == 32u) != 0ull;   // a record ends with the block's last column
                    n_adv = (uint32_t)__popcll(__ballot(lane < 32u && rel <= 32u));
                    endmask = (starts >> 1) | (end32 ? 0x80000000u : 0u);          // bit j = a record ends at column j
                    open_next = more && !end32;
#pragma unroll
                    for (int i = 0; i < 5; ++i) {
                        const uint32_t d = 1u << i;
                        if (col >= d && ((starts >> (col - d + 1u)) & ((1u << d) - 1u)) == 0u) ok_d |= 1u << i;
                    }
                }
                // columns past the end of the range score -inf; the running record's maxima join at column 0
                float x[16], o[16];
                const bool col_in = tb + col < t1;
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    x[v] = col_in ? acc[v] : NINF;
                    if (col == 0u) x[v] = fmaxf(x[v], carry[t][v]);
                }
                // segmented inclusive max over the 32 column lanes of each half; fmaxf skips a NaN (rule 3), so only a record whose
                // every s_ij is NaN still holds one at its last column: the fold below makes it -inf
#pragma unroll
                for (int i = 0; i < 5; ++i) {
                    const bool ok = (ok_d >> i) & 1u;
#pragma unroll
                    for (int v = 0; v < 16; ++v) {
                        const float y = maxsim_from_lane(x[v], lane - (1u << i));
                        x[v] = ok ? fmaxf(x[v], y) : x[v];
                    }
                }
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    x[v] = x[v] != x[v] ? NINF : x[v];
                    const float c = maxsim_from_lane(x[v], half * 32u + 31u);
                    carry[t][v] = open_next ? c : NINF;
                    o[v] = maxsim_from_lane(x[v], lane ^ 32u);
                }
                // rule 4 in the lanes of half 0: accumulator register v of half h is row 8 (v / 4) + 4 h + v % 4 of the tile
#pragma unroll
                for (int g = 0; g < 8; ++g)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const uint32_t row = (uint32_t)t * 32u + 4u * g + e;
                        const int v = (g >> 1) * 4 + e;
                        const float mv = (g & 1) ? o[v] : x[v];
                        if (row == 0u) s = mv;
                        else if (row < tq) s = s + mv;
                    }
            }
            if (half == 0u && ((endmask >> col) & 1u)) {
                const uint32_t c = rc0 + (uint32_t)__popc(starts & ((2u << col) - 1u));
                const bool live = range_live(a.mask, a.mask_words, a.crec[c]);
                a.S[(size_t)q * a.m + c] = live ? score_ord(s, false) : RANGE_FAIL;
            }
            rc0 += n_adv;
            maxsim_wave_sync();   // the next block is stored; this one may be overwritten by the block after it
        }
    }
}

}  // namespace lynse
