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

template <typename T>
struct MaxSimArgsT {
    const T* tokens;          // [total tokens][ld], columns dim .. ld - 1 are zero
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
using MaxSimArgs = MaxSimArgsT<float>;          // k_maxsim_scan
using MaxSimH16Args = MaxSimArgsT<_Float16>;    // k_maxsim_h16: the token rows are halves, the queries still f32 (converted as they are staged)

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

// ---- f16 token storage (include/lynse_hip.h, MULTI-VECTOR SEARCH, f16 addendum) ------------------------------------
//   k_maxsim_h16    the same split (one wave, one range of whole records, blocks of 32 token rows) and the same epilogue on
//                   v_mfma_f32_32x32x16_f16.  The 16 bytes a lane gives that instruction for B are 8 consecutive halves of ONE token
//                   row, so lane (j = lane % 32, h = lane / 32) loads its fragments of row j from HBM straight into the operand
//                   registers: the token stream never sees the LDS, which holds the query tiles (halves, converted as they are
//                   staged) and 32 boundary flags per wave.  Of each 32 columns of a row half h owns the 16 at 16 h: k-steps 2 p and
//                   2 p + 1 take its halves 0..7 and 8..15, so a lane reads 32 contiguous bytes and a row 64 per pair of steps; the
//                   query fragments follow the same assignment (the order of a sum is not part of the contract).  A chunk of 128
//                   columns (64 at 8 query tiles) is 8 fragments = 32 VGPRs; the chunks of the stream (block after block) go through a ring of RING such
//                   buffers, loaded RING - 1 chunks ahead of the MFMAs that read them.

// LDS row pitch of a query tile in BYTES: 2 ld + 16 = 16 s with s = ld / 8 + 1 odd (ld / 8 is a multiple of 4), so by the argument at
// maxsim_pitch the ds_read_b128 fragment reads (16 lanes: one 16-B piece of 16 consecutive rows) are conflict-free.
__host__ __device__ inline uint32_t maxsim_h16_pitch(uint32_t ld) { return 2u * ld + 16u; }
// LDS bytes: the query tiles | the 32 boundary flags of each of the (always 4) waves
__host__ __device__ inline size_t maxsim_h16_lds_bytes(uint32_t ld, uint32_t tiles) {
    return (size_t)tiles * MAXSIM_BLOCK * maxsim_h16_pitch(ld) + (size_t)MAXSIM_MAX_WAVES * MAXSIM_BLOCK * 4u;
}

// Rule 1 of the addendum: round to nearest even to binary16, then a subnormal result becomes a zero of its sign.
__host__ __device__ inline uint16_t maxsim_h16_flush(uint16_t b) { return (b & 0x7c00u) ? b : (uint16_t)(b & 0x8000u); }
__device__ __forceinline__ uint32_t maxsim_h16_of(float x) { return maxsim_h16_flush(__builtin_bit_cast(uint16_t, (_Float16)x)); }

// The store's rows at the device pitch from what `append` was given: SRC = float (converted) or uint16_t (raw halves), [rows][dim]
// -> [rows][ld] with rule 1 applied and zero columns past the dimension.  One thread per stored half.
template <typename SRC>
__global__ void __launch_bounds__(256) k_maxsim_store_h16(const SRC* __restrict__ src, uint16_t* __restrict__ dst, uint64_t rows, uint32_t dim, uint32_t ld) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= rows * ld) return;
    const uint64_t r = i / ld;
    const uint32_t c = (uint32_t)(i - r * ld);
    uint16_t v = 0;
    if (c < dim) {
        if constexpr (sizeof(SRC) == 4) v = (uint16_t)maxsim_h16_of(src[r * dim + c]);
        else v = maxsim_h16_flush(src[r * dim + c]);
    }
    dst[i] = v;
}

// One chunk of a block into a ring buffer: lane (col, half) takes, of each of the chunk's NP column groups of 32 that exist, the 32
// bytes at halves 16 half .. 16 half + 15 of token row t_first + col.  Rows at or past `t_end` (the end of the wave's range, or a
// block past its last) are zero, as are the groups past the row pitch: nothing outside the range is read.
template <int NP>
__device__ __forceinline__ void maxsim_h16_load(const MaxSimH16Args& a, uint64_t t_first, uint64_t t_end, uint32_t kc, uint32_t col, uint32_t half, half8 (&f)[2 * NP]) {
    const bool in = t_first + col < t_end;
    const _Float16* src = a.tokens + (size_t)(t_first + col) * a.ld + kc + half * 16u;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        f[2 * p] = half8{0, 0, 0, 0, 0, 0, 0, 0};
        f[2 * p + 1] = half8{0, 0, 0, 0, 0, 0, 0, 0};
        if (in && kc + (uint32_t)p * 32u < a.ld) {
            f[2 * p] = *reinterpret_cast<const half8*>(src + p * 32);
            f[2 * p + 1] = *reinterpret_cast<const half8*>(src + p * 32 + 8);
        }
    }
}

// the record boundaries of a block, wave-uniform
struct MaxSimBounds {
    uint32_t starts;     // bit j = a record begins at column j (1 <= j <= 31)
    uint32_t endmask;    // bit j = a record ends at column j
    uint32_t n_adv;      // records that end in the block
    bool open_next;      // the last record runs on into the next block
};
// rec_end: lane l < 32 holds the end of record rc0 + l (~0 past the range); at most 32 of them fall into (tb, tb + 32]
__device__ __forceinline__ MaxSimBounds maxsim_h16_bounds(uint64_t rec_end, uint64_t tb, bool more, uint32_t lane, uint32_t col, uint32_t* flag_l) {
    const uint64_t rel64 = rec_end - tb;   // >= 1; ~0 - tb stays huge
    const uint32_t rel = rel64 > 64u ? 64u : (uint32_t)rel64;
    if (lane < 32u) flag_l[lane] = 0u;
    maxsim_wave_sync();
    if (lane < 32u && rel < 32u) flag_l[rel] = 1u;   // (the ends ascend strictly: one lane per flag)
    maxsim_wave_sync();
    MaxSimBounds bd;
    bd.starts = (uint32_t)__ballot(flag_l[col] != 0u);
    const bool end32 = __ballot(lane < 32u && rel == 32u) != 0ull;   // a record ends with the block's last column
    bd.n_adv = (uint32_t)__popcll(__ballot(lane < 32u && rel <= 32u));
    bd.endmask = (bd.starts >> 1) | (end32 ? 0x80000000u : 0u);
    bd.open_next = more && !end32;
    maxsim_wave_sync();   // (the flags are read: the next block may clear them)
    return bd;
}

// Rules 3 and 4 for one query tile of a block, as in k_maxsim_scan (the 32 x 32 accumulator of v_mfma_f32_32x32x16_f16 has the lane
// and register layout of v_mfma_f32_32x32x2_f32): columns past the range score -inf, the running record's maxima join at column 0,
// a segmented inclusive max over the 32 column lanes of each half, the carry out of column 31, and in the lanes of half 0 the sum of
// the row maxima in query-token order, `s` running on from tile to tile.
__device__ __forceinline__ LY_MAXSIM_FN void maxsim_h16_fold(const f32x16& acc, float (&carry)[16], const MaxSimBounds& bd, uint32_t ok_d, bool col_in,
                                                             uint32_t lane, uint32_t col, uint32_t half, uint32_t t, uint32_t tq, float& s) {
    const float NINF = -__builtin_huge_valf();
    float x[16], o[16];
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        x[v] = col_in ? acc[v] : NINF;
        if (col == 0u) x[v] = fmaxf(x[v], carry[v]);
    }
    // fmaxf skips a NaN (rule 3), so only a record whose every s_ij is NaN still holds one at its last column: the fold makes it -inf
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
        carry[v] = bd.open_next ? c : NINF;
        o[v] = maxsim_from_lane(x[v], lane ^ 32u);
    }
    // accumulator register v of half h is row 8 (v / 4) + 4 h + v % 4 of the tile
#pragma unroll
    for (int g = 0; g < 8; ++g)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t row = t * 32u + 4u * g + e;
            const int v = (g >> 1) * 4 + e;
            const float mv = (g & 1) ? o[v] : x[v];
            if (row == 0u) s = mv;
            else if (row < tq) s = s + mv;
        }
}

// The query tiles of a workgroup into LDS as halves (rule 1 on the way), `rows` rows at pitch PB, zero rows past the query's own:
// 16-B pieces of 8 columns.  Shared by k_maxsim_h16 and k_maxsim_cand_h16.
__device__ __forceinline__ void maxsim_h16_stage(const float* Q, uint32_t tq_rows, uint32_t rows, uint32_t K, uint32_t PB, unsigned char* q_l, uint32_t tid) {
    const uint32_t c8n = K / 8u;
    for (uint32_t p = tid; p < rows * c8n; p += blockDim.x) {
        const uint32_t r = p / c8n, c = p - r * c8n;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (r < tq_rows) {
            const float* src = Q + (size_t)r * K + c * 8u;
            const f32x4 lo = *reinterpret_cast<const f32x4*>(src), hi = *reinterpret_cast<const f32x4*>(src + 4);
            v = u32x4{maxsim_h16_of(lo[0]) | (maxsim_h16_of(lo[1]) << 16), maxsim_h16_of(lo[2]) | (maxsim_h16_of(lo[3]) << 16),
                      maxsim_h16_of(hi[0]) | (maxsim_h16_of(hi[1]) << 16), maxsim_h16_of(hi[2]) | (maxsim_h16_of(hi[3]) << 16)};
        }
        *reinterpret_cast<u32x4*>(q_l + (size_t)r * PB + c * 16u) = v;
    }
}

// NT = query tiles of 32 rows the LDS holds (1, 2, 4 or 8); a query of fewer tiles skips the rest.  grid.x strides over the ranges,
// grid.y is the query; blockDim.x / 64 waves.  RING - 1 = the chunks a load runs ahead: two while the accumulators and carried maxima
// of the tiles leave the registers for a third buffer, one from 4 tiles on.
template <int NT>
__global__ void LY_MAXSIM_FN __launch_bounds__(MAXSIM_MAX_WAVES * 64) k_maxsim_h16(MaxSimH16Args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sm_maxsim_h16[];
    constexpr int RING = NT <= 2 ? 3 : 2;
    constexpr int NP = NT == 8 ? 2 : 4;   // column groups of 32 in a chunk: 128 columns, 64 where 8 tiles' accumulators and maxima fill the registers
    constexpr uint32_t KC = 32u * NP;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, col = lane & 31u, half = lane >> 5;
    const uint32_t wave = maxsim_uniform(tid >> 6), waves = blockDim.x >> 6;
    const uint32_t K = a.ld, PB = maxsim_h16_pitch(K), nch = (K + KC - 1u) / KC;
    const uint32_t q = blockIdx.y;
    const uint64_t q_off = a.qdesc[2u * q];
    const uint32_t tq = (uint32_t)a.qdesc[2u * q + 1u], tq_rows = (tq + 31u) / 32u * 32u;
    unsigned char* q_l = sm_maxsim_h16;
    uint32_t* flag_l = reinterpret_cast<uint32_t*>(q_l + (size_t)NT * MAXSIM_BLOCK * PB) + wave * MAXSIM_BLOCK;
    maxsim_h16_stage(a.Q + q_off, tq_rows, (uint32_t)NT * 32u, K, PB, q_l, tid);
    __syncthreads();   // the only workgroup barrier: from here on the waves run their own ranges
    // this lane's query fragments: row `col` of a tile, the bytes of its halves 16 half .. of each column group
    const unsigned char* qa = q_l + (size_t)col * PB + half * 32u;
    // one tile: the fragments of the first chunk stay in registers for the whole kernel — up to 128 columns the loop reads no LDS
    half8 qreg[8];
    if constexpr (NT == 1) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            qreg[2 * p] = half8{0, 0, 0, 0, 0, 0, 0, 0};
            qreg[2 * p + 1] = half8{0, 0, 0, 0, 0, 0, 0, 0};
            if ((uint32_t)p * 32u < K) {
                qreg[2 * p] = *reinterpret_cast<const half8*>(qa + p * 64);
                qreg[2 * p + 1] = *reinterpret_cast<const half8*>(qa + p * 64 + 16);
            }
        }
    }
    const float NINF = -__builtin_huge_valf();
    for (uint32_t r = blockIdx.x * waves + wave; r < a.n_ranges; r += gridDim.x * waves) {
        const uint32_t ca = maxsim_uniform(a.ranges[r]), cb = maxsim_uniform(a.ranges[r + 1u]);
        const uint64_t t0 = maxsim_uniform(a.cptr[ca]), t1 = maxsim_uniform(a.cptr[cb]);
        const uint32_t nb = (uint32_t)((t1 - t0 + MAXSIM_BLOCK - 1u) / MAXSIM_BLOCK);
        half8 buf[RING][2 * NP];
        uint32_t lb = 0, lc = 0;   // the load cursor: block and chunk, RING - 1 chunks ahead of (b, c)
#pragma unroll
        for (int i = 0; i < RING - 1; ++i) {
            maxsim_h16_load<NP>(a, t0 + (uint64_t)lb * MAXSIM_BLOCK, lb < nb ? t1 : 0ull, lc * KC, col, half, buf[i]);
            if (++lc == nch) lc = 0, ++lb;
        }
        uint32_t rc0 = ca;       // the record of the block's first token
        float carry[NT][16];     // the row maxima of the record that runs on from the previous block (read at column 0 only)
        f32x16 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int v = 0; v < 16; ++v) carry[t][v] = NINF;
        uint64_t rec_end = ~0ull;
        uint32_t b = 0, c = 0;
        while (b < nb) {
#pragma unroll
            for (int i = 0; i < RING; ++i) {
                if (b < nb) {
                    const uint64_t tb = t0 + (uint64_t)b * MAXSIM_BLOCK;
                    if (c == 0u) {
                        // the ends of the records from rc0 on, asked for BEFORE the chunk ahead: the epilogue's wait then leaves that one in flight
                        rec_end = ~0ull;
                        if (lane < 32u && (uint64_t)rc0 + 1u + lane <= cb) rec_end = a.cptr[rc0 + 1u + lane];
#pragma unroll
                        for (int t = 0; t < NT; ++t) acc[t] = f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
                    }
                    maxsim_h16_load<NP>(a, t0 + (uint64_t)lb * MAXSIM_BLOCK, lb < nb ? t1 : 0ull, lc * KC, col, half, buf[(i + RING - 1) % RING]);
                    if (++lc == nch) lc = 0, ++lb;
                    const uint32_t kc = c * KC;
#pragma unroll
                    for (int p = 0; p < NP; ++p) {
                        if (kc + (uint32_t)p * 32u >= K) continue;
#pragma unroll
                        for (int e = 0; e < 2; ++e) {
#pragma unroll
                            for (int t = 0; t < NT; ++t) {
                                if (t != 0 && (uint32_t)t * 32u >= tq) continue;
                                half8 av;
                                if (NT == 1 && c == 0u) av = qreg[2 * p + e];
                                else av = *reinterpret_cast<const half8*>(qa + (size_t)t * 32u * PB + (kc + (uint32_t)p * 32u) * 2u + e * 16);
                                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(av, buf[i][2 * p + e], acc[t], 0, 0, 0);
                            }
                        }
                    }
                    if (c + 1u == nch) {   // the block's last chunk: rules 3 and 4, the scores of the records that end in it
                        const MaxSimBounds bd = maxsim_h16_bounds(rec_end, tb, b + 1u < nb, lane, col, flag_l);
                        uint32_t ok_d = 0u;   // bit i: the lane 2^i columns down is in the same record
#pragma unroll
                        for (int j = 0; j < 5; ++j) {
                            const uint32_t d = 1u << j;
                            if (col >= d && ((bd.starts >> (col - d + 1u)) & ((1u << d) - 1u)) == 0u) ok_d |= 1u << j;
                        }
                        float s = 0.0f;
#pragma unroll
                        for (int t = 0; t < NT; ++t) {
                            if (t != 0 && (uint32_t)t * 32u >= tq) continue;
                            maxsim_h16_fold(acc[t], carry[t], bd, ok_d, tb + col < t1, lane, col, half, (uint32_t)t, tq, s);
                        }
                        if (half == 0u && ((bd.endmask >> col) & 1u)) {
                            const uint32_t cr = rc0 + (uint32_t)__popc(bd.starts & ((2u << col) - 1u));
                            const bool live = !a.mask || range_live(a.mask, a.mask_words, a.crec[cr]);
                            a.S[(size_t)q * a.m + cr] = live ? score_ord(s, false) : RANGE_FAIL;
                        }
                        rc0 += bd.n_adv;
                        c = 0u;
                        ++b;
                    } else {
                        ++c;
                    }
                }
            }
        }
    }
}

// ---- int8 token storage (include/lynse_hip.h, MULTI-VECTOR SEARCH, INT8 TOKEN STORAGE) ---------------------------
//   k_maxsim_i8     the same split (one wave, one range of whole records, blocks of 32 token rows) with the operand roles SWAPPED:
//                   the block's tokens are the A operand of v_mfma_i32_32x32x32_i8 and the query tile the B operand, so in the
//                   32 x 32 accumulator a lane holds ONE query column and 16 of the 32 token rows.  The max over a record's tokens
//                   then walks down the lane's own registers (v_max_f32, no cross-lane traffic inside 4 rows) and crosses to the
//                   other half of the wave once per 4 rows (v_permlane32_swap); only where a record ENDS do the 32 column lanes
//                   meet, in the 5-step pairwise tree of rule 4".  The 16 bytes a lane gives the instruction for A are 16 codes of
//                   ONE token row: lane (j = lane % 32, h = lane / 32) loads them from HBM straight into the operand registers.
//                   Of each 64 columns of a row half h owns the 32 at 32 h: k-steps 2 p and 2 p + 1 take its bytes 0..15 and
//                   16..31, so a lane reads 32 contiguous bytes per pair of steps; the query fragments follow the same assignment
//                   (the integer sum is exact, its order free).  A chunk of 128 columns is 4 fragments = 16 VGPRs; the chunks of
//                   the stream go through a ring of RING such buffers, loaded RING - 1 chunks ahead of the MFMAs that read them.
//   k_maxsim_store_i8  rule 1": f32 rows [rows][dim] -> codes [rows][ld] and scales[rows], 16 lanes a row.
typedef int maxsim_i32x4 __attribute__((ext_vector_type(4)));
typedef int maxsim_i32x16 __attribute__((ext_vector_type(16)));
typedef float maxsim_f32x4_u __attribute__((ext_vector_type(4), aligned(4)));   // the scales of 4 rows: a token offset is any multiple of 4 B

constexpr uint32_t MAXSIM_I8_KC = 128;   // columns of a chunk: 2 pairs of k-steps

// LDS row pitch of a query tile in BYTES: ld + 16 = 16 s with s = ld / 16 + 1 odd (ld / 16 is even), so by the argument at
// maxsim_pitch the ds_read_b128 fragment reads (16 lanes: one 16-B piece of 16 consecutive rows) are conflict-free.
__host__ __device__ inline uint32_t maxsim_i8_pitch(uint32_t ld) { return ld + 16u; }
// LDS bytes: the query tiles as codes | their scales | the 32 boundary flags of each of the (always 4) waves
__host__ __device__ inline size_t maxsim_i8_lds_bytes(uint32_t ld, uint32_t tiles) {
    return (size_t)tiles * MAXSIM_BLOCK * (maxsim_i8_pitch(ld) + 4u) + (size_t)MAXSIM_MAX_WAVES * MAXSIM_BLOCK * 4u;
}

struct MaxSimI8Args {
    MaxSimArgsT<int8_t> a;    // the token rows are codes, ld BYTES a row; the queries still f32 (quantised as they are staged)
    const float* scales;      // [total tokens]
};

// Rule 1": the scale pair of a row from its amax (fmaxf over |p_k|: a NaN element is skipped), and the code of an element
__device__ __forceinline__ void maxsim_i8_scale(float amax, float& inv, float& s) {
    const bool none = amax == 0.0f || amax == __builtin_huge_valf();
    inv = none ? 0.0f : 127.0f / amax;
    s = none ? 0.0f : amax / 127.0f;
}
__device__ __forceinline__ uint32_t maxsim_i8_code(float p, float inv) {
    float r = rintf(p * inv);
    r = r != r ? 0.0f : fminf(fmaxf(r, -127.0f), 127.0f);   // (inv = 0 where the row has no scale: 0, or NaN from an inf element)
    return (uint32_t)(int)r & 0xffu;
}
__device__ __forceinline__ uint32_t maxsim_i8_pack(f32x4 v, float inv) {
    return maxsim_i8_code(v[0], inv) | (maxsim_i8_code(v[1], inv) << 8) | (maxsim_i8_code(v[2], inv) << 16) | (maxsim_i8_code(v[3], inv) << 24);
}

// 16 lanes a row: the amax over the lanes' columns (order-free), then 4 codes a lane and trip as one 32-bit store.
__global__ void __launch_bounds__(256) k_maxsim_store_i8(const float* __restrict__ src, uint32_t* __restrict__ codes, float* __restrict__ scales,
                                                         uint64_t rows, uint32_t dim, uint32_t ld) {
    const uint32_t lane = threadIdx.x & 63u, l = threadIdx.x & 15u;
    const uint64_t r = (uint64_t)blockIdx.x * 16u + (threadIdx.x >> 4);
    const bool in = r < rows;   // (no early return: the lanes of a wave exchange below)
    const float* p = src + (in ? r : 0) * dim;
    float amax = 0.0f;
    if (in)
        for (uint32_t c = l; c < dim; c += 16u) amax = fmaxf(amax, fabsf(p[c]));
#pragma unroll
    for (uint32_t d = 1; d < 16u; d <<= 1) amax = fmaxf(amax, maxsim_from_lane(amax, lane ^ d));
    if (!in) return;
    float inv, s;
    maxsim_i8_scale(amax, inv, s);
    if (l == 0u) scales[r] = s;
    for (uint32_t c4 = l; c4 < ld / 4u; c4 += 16u) {
        f32x4 v;
#pragma unroll
        for (uint32_t e = 0; e < 4u; ++e) v[e] = c4 * 4u + e < dim ? p[c4 * 4u + e] : 0.0f;
        codes[r * (ld / 4u) + c4] = maxsim_i8_pack(v, inv);
    }
}

// One chunk of a block into a ring buffer: lane (col, half) takes, of each of the chunk's 2 column groups of 64, the 32 bytes at
// 32 half of token row t_first + col.  Rows at or past `t_end` (the end of the wave's range, or a block past its last) are zero,
// as are the bytes past the row pitch (ld may end in the middle of a group): nothing outside the range is read.
__device__ __forceinline__ void maxsim_i8_load(const MaxSimI8Args& x, uint64_t t_first, uint64_t t_end, uint32_t kc, uint32_t col, uint32_t half, maxsim_i32x4 (&f)[4]) {
    const bool in = t_first + col < t_end;
    const int8_t* src = x.a.tokens + (size_t)(t_first + col) * x.a.ld + kc + half * 32u;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        f[2 * p] = maxsim_i32x4{0, 0, 0, 0};
        f[2 * p + 1] = maxsim_i32x4{0, 0, 0, 0};
        if (in && kc + (uint32_t)p * 64u + half * 32u < x.a.ld) {
            f[2 * p] = *reinterpret_cast<const maxsim_i32x4*>(src + p * 64);
            f[2 * p + 1] = *reinterpret_cast<const maxsim_i32x4*>(src + p * 64 + 16);
        }
    }
}
// the matching query fragment: 16 codes of the lane's query row at byte `off` of it, zero past the pitch
__device__ __forceinline__ maxsim_i32x4 maxsim_i8_qfrag(const unsigned char* qrow, uint32_t off, uint32_t K) {
    maxsim_i32x4 v = {0, 0, 0, 0};
    if (off < K) v = *reinterpret_cast<const maxsim_i32x4*>(qrow + off);
    return v;
}

// v of this lane and of the lane 32 away: v_permlane32_swap of a register with itself leaves (own | lower half's) and (upper half's | own)
__device__ __forceinline__ void maxsim_i8_halves(float v, float& from_lo, float& from_hi) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    from_lo = __uint_as_float(r[0]);   // lanes 32..63: the value of lane - 32; lanes 0..31: their own
    from_hi = __uint_as_float(r[1]);   // lanes 0..31: the value of lane + 32; lanes 32..63: their own
}
// Rule 4" within a tile: the balanced pairwise tree over the 32 column lanes of a half, as a butterfly — an f32 add commutes, so
// every lane ends with the bits of the tree's root.  Lanes 1, 2 apart by quad_perm, 4 and 8 apart by the mirrors (the lanes of a
// finished level agree, so the mirror's partner holds the partner group's sum), 16 apart by ds_swizzle.
__device__ __forceinline__ LY_MAXSIM_FN float maxsim_i8_tree(float m) {
    m = m + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(m), 0xB1, 0xf, 0xf, false));    // quad_perm [1, 0, 3, 2]
    m = m + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(m), 0x4E, 0xf, 0xf, false));    // quad_perm [2, 3, 0, 1]
    m = m + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(m), 0x141, 0xf, 0xf, false));   // row_half_mirror
    m = m + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(m), 0x140, 0xf, 0xf, false));   // row_mirror
    return m + __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(m), 0x401F));                    // lane ^ 16
}

// The query tiles of a workgroup into LDS by rule 1", 8 lanes a row and 32 rows of the workgroup a trip: the row's amax over its 16-B
// pieces, then the codes of those pieces (the row comes from the cache the second time) and the scale; rows past the query's own
// tiles are never read.  Shared by k_maxsim_i8 and k_maxsim_cand_i8.
__device__ __forceinline__ void maxsim_i8_stage(const float* Q, uint32_t tq_rows, uint32_t K, uint32_t PB, unsigned char* q_l, float* sq_l, uint32_t tid, uint32_t lane) {
    const uint32_t g = tid & 7u, c16n = K / 16u;
    for (uint32_t r = tid >> 3; r < tq_rows; r += blockDim.x >> 3) {   // (uniform over a wave's groups of 8: tq_rows is a multiple of 32)
        const float* src = Q + (size_t)r * K;
        float amax = 0.0f;
        for (uint32_t c = g; c < c16n; c += 8u)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(src + c * 16u + e * 4);
                amax = fmaxf(fmaxf(amax, fmaxf(fabsf(v[0]), fabsf(v[1]))), fmaxf(fabsf(v[2]), fabsf(v[3])));
            }
#pragma unroll
        for (uint32_t d = 1; d < 8u; d <<= 1) amax = fmaxf(amax, maxsim_from_lane(amax, lane ^ d));
        float inv, s;
        maxsim_i8_scale(amax, inv, s);
        if (g == 0u) sq_l[r] = s;
        for (uint32_t c = g; c < c16n; c += 8u) {
            u32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = maxsim_i8_pack(*reinterpret_cast<const f32x4*>(src + c * 16u + e * 4), inv);
            *reinterpret_cast<u32x4*>(q_l + (size_t)r * PB + c * 16u) = o;
        }
    }
}

// NT = query tiles of 32 rows the LDS holds (1, 2, 4 or 8); a query of fewer tiles skips the rest.  grid.x strides over the ranges,
// grid.y is the query; 4 waves.  RING - 1 = the chunks a load runs ahead (DESIGN.md §30 has the register report behind the choice).
template <int NT>
__global__ void LY_MAXSIM_FN __launch_bounds__(MAXSIM_MAX_WAVES * 64) k_maxsim_i8(MaxSimI8Args x) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sm_maxsim_i8[];
    constexpr int RING = NT <= 2 ? 4 : 3;
    constexpr uint32_t KC = MAXSIM_I8_KC;
    const MaxSimArgsT<int8_t>& a = x.a;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, col = lane & 31u, half = lane >> 5;
    const uint32_t wave = maxsim_uniform(tid >> 6), waves = blockDim.x >> 6;
    const uint32_t K = a.ld, PB = maxsim_i8_pitch(K), nch = (K + KC - 1u) / KC;
    const uint32_t q = blockIdx.y;
    const uint64_t q_off = a.qdesc[2u * q];
    const uint32_t tq = (uint32_t)a.qdesc[2u * q + 1u], tq_rows = (tq + 31u) / 32u * 32u;
    unsigned char* q_l = sm_maxsim_i8;
    float* sq_l = reinterpret_cast<float*>(q_l + (size_t)NT * MAXSIM_BLOCK * PB);
    uint32_t* flag_l = reinterpret_cast<uint32_t*>(sq_l + NT * MAXSIM_BLOCK) + wave * MAXSIM_BLOCK;
    maxsim_i8_stage(a.Q + q_off, tq_rows, K, PB, q_l, sq_l, tid, lane);
    __syncthreads();   // the only workgroup barrier: from here on the waves run their own ranges
    // this lane's query column: row `col` of each tile, its scale (+0 and never used past the query's tokens) and its fragment bytes
    const unsigned char* qa = q_l + (size_t)col * PB;
    float sq[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) sq[t] = (uint32_t)t * 32u + col < tq ? sq_l[(uint32_t)t * 32u + col] : 0.0f;
    // one tile: the fragments of the first chunk stay in registers for the whole kernel — up to 128 columns the loop reads no LDS
    maxsim_i32x4 qreg[4];
    if constexpr (NT == 1) {
#pragma unroll
        for (int f = 0; f < 4; ++f) qreg[f] = maxsim_i8_qfrag(qa, (uint32_t)(f >> 1) * 64u + half * 32u + (uint32_t)(f & 1) * 16u, K);
    }
    const float NINF = -__builtin_huge_valf();
    for (uint32_t r = blockIdx.x * waves + wave; r < a.n_ranges; r += gridDim.x * waves) {
        const uint32_t ca = maxsim_uniform(a.ranges[r]), cb = maxsim_uniform(a.ranges[r + 1u]);
        const uint64_t t0 = maxsim_uniform(a.cptr[ca]), t1 = maxsim_uniform(a.cptr[cb]);
        const uint32_t nb = (uint32_t)((t1 - t0 + MAXSIM_BLOCK - 1u) / MAXSIM_BLOCK);
        maxsim_i32x4 buf[RING][4];
        uint32_t lb = 0, lc = 0;   // the load cursor: block and chunk, RING - 1 chunks ahead of (b, c)
#pragma unroll
        for (int i = 0; i < RING - 1; ++i) {
            maxsim_i8_load(x, t0 + (uint64_t)lb * MAXSIM_BLOCK, lb < nb ? t1 : 0ull, lc * KC, col, half, buf[i]);
            if (++lc == nch) lc = 0, ++lb;
        }
        uint32_t rc0 = ca;   // the record of the block's first token
        float run[NT];       // the maximum so far of the record that is open, ONE register a tile: it runs on from block to block
        maxsim_i32x16 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) run[t] = NINF;
        uint64_t rec_end = ~0ull;
        uint32_t b = 0, c = 0;
        while (b < nb) {
#pragma unroll
            for (int i = 0; i < RING; ++i) {
                if (b < nb) {
                    const uint64_t tb = t0 + (uint64_t)b * MAXSIM_BLOCK;
                    const uint32_t nrows = t1 - tb < MAXSIM_BLOCK ? (uint32_t)(t1 - tb) : MAXSIM_BLOCK;   // rows of the block inside the range
                    const bool last = c + 1u == nch;
                    if (c == 0u) {
                        // the ends of the records from rc0 on, asked for BEFORE the chunk ahead: the epilogue's wait then leaves that one in flight
                        rec_end = ~0ull;
                        if (lane < 32u && (uint64_t)rc0 + 1u + lane <= cb) rec_end = a.cptr[rc0 + 1u + lane];
#pragma unroll
                        for (int t = 0; t < NT; ++t) acc[t] = maxsim_i32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
                    }
                    // the scales of this half's 16 rows (register v is row 8 (v / 4) + 4 half + v % 4), ahead of the block's last MFMAs;
                    // rows past the range are not read
                    f32x4 sc[4];
                    if (last) {
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            const uint32_t r0 = 8u * g + 4u * half;
                            if (r0 + 4u <= nrows) {
                                sc[g] = *reinterpret_cast<const maxsim_f32x4_u*>(x.scales + tb + r0);
                            } else {
#pragma unroll
                                for (uint32_t e = 0; e < 4u; ++e) sc[g][e] = r0 + e < nrows ? x.scales[tb + r0 + e] : 0.0f;
                            }
                        }
                    }
                    maxsim_i8_load(x, t0 + (uint64_t)lb * MAXSIM_BLOCK, lb < nb ? t1 : 0ull, lc * KC, col, half, buf[(i + RING - 1) % RING]);
                    if (++lc == nch) lc = 0, ++lb;
                    const uint32_t kc = c * KC;
#pragma unroll
                    for (int f = 0; f < 4; ++f) {
                        const uint32_t off = kc + (uint32_t)(f >> 1) * 64u;   // the column group of 64; half h of it, bytes 16 (f & 1) ..
                        if (off >= K) continue;
#pragma unroll
                        for (int t = 0; t < NT; ++t) {
                            if (t != 0 && (uint32_t)t * 32u >= tq) continue;
                            maxsim_i32x4 bv;
                            if (NT == 1 && c == 0u) bv = qreg[f];
                            else bv = maxsim_i8_qfrag(qa + (size_t)t * 32u * PB, off + half * 32u + (uint32_t)(f & 1) * 16u, K);
                            acc[t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(buf[i][f], bv, acc[t], 0, 0, 0);
                        }
                    }
                    if (last) {   // the block's last chunk: rules 2" - 4", the scores of the records that end in it
                        const MaxSimBounds bd = maxsim_h16_bounds(rec_end, tb, b + 1u < nb, lane, col, flag_l);
                        // v_ij = f32(d_ij) * s_j in place of the sums
                        float v[NT][16];
#pragma unroll
                        for (int t = 0; t < NT; ++t) {
                            if (t != 0 && (uint32_t)t * 32u >= tq) continue;
#pragma unroll
                            for (int k = 0; k < 16; ++k) v[t][k] = (float)acc[t][k] * sc[k >> 2][k & 3];
                        }
                        // down the 32 rows in groups of 8: rows 8 g .. 8 g + 3 are registers 4 g .. of half 0, the next four of half 1
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            if (8u * g >= nrows) continue;
                            if (8u * g + 8u <= nrows && ((bd.endmask >> (8 * g)) & 0xffu) == 0u) {
                                // no record ends in these 8 rows: each half folds its own four, one exchange joins them in both halves
#pragma unroll
                                for (int t = 0; t < NT; ++t) {
                                    if (t != 0 && (uint32_t)t * 32u >= tq) continue;
                                    const float m4 = fmaxf(fmaxf(v[t][4 * g], v[t][4 * g + 1]), fmaxf(v[t][4 * g + 2], v[t][4 * g + 3]));
                                    float lo, hi;
                                    maxsim_i8_halves(m4, lo, hi);
                                    run[t] = fmaxf(run[t], fmaxf(lo, hi));
                                }
                                continue;
                            }
#pragma unroll
                            for (int o = 0; o < 2; ++o) {   // the owning half of rows 8 g + 4 o ..: its lanes hold the record's maximum so far
#pragma unroll
                                for (int e = 0; e < 4; ++e) {
                                    const uint32_t row = 8u * g + 4u * o + e;
                                    if (row >= nrows) continue;
#pragma unroll
                                    for (int t = 0; t < NT; ++t) {
                                        if (t != 0 && (uint32_t)t * 32u >= tq) continue;
                                        run[t] = fmaxf(run[t], v[t][4 * g + e]);
                                    }
                                    if ((bd.endmask >> row) & 1u) {   // a record ends here: rules 3" and 4" in the owning half
                                        float s = 0.0f;
#pragma unroll
                                        for (int t = 0; t < NT; ++t) {
                                            if (t != 0 && (uint32_t)t * 32u >= tq) continue;
                                            const float tile = maxsim_i8_tree((uint32_t)t * 32u + col < tq ? sq[t] * run[t] : 0.0f);
                                            s = t == 0 ? tile : s + tile;
                                            run[t] = NINF;
                                        }
                                        if (lane == 32u * o) {
                                            const uint32_t cr = rc0 + (uint32_t)__popc(bd.endmask & ((1u << row) - 1u));
                                            const bool live = !a.mask || range_live(a.mask, a.mask_words, a.crec[cr]);
                                            a.S[(size_t)q * a.m + cr] = live ? score_ord(s, false) : RANGE_FAIL;
                                        }
                                    }
                                }
                                // hand the maximum so far to the other half, which owns the next four rows (both halves agree after it)
#pragma unroll
                                for (int t = 0; t < NT; ++t) {
                                    if (t != 0 && (uint32_t)t * 32u >= tq) continue;
                                    float lo, hi;
                                    maxsim_i8_halves(run[t], lo, hi);
                                    run[t] = o == 0 ? lo : hi;
                                }
                            }
                        }
                        rc0 += bd.n_adv;
                        c = 0u;
                        ++b;
                    } else {
                        ++c;
                    }
                }
            }
        }
    }
}

// ---- MXFP4 token storage (include/lynse_hip.h, MULTI-VECTOR SEARCH, MXFP4 TOKEN STORAGE) -------------------------
//   k_maxsim_mx4    k_maxsim_i8's split and swapped roles on v_mfma_scale_f32_32x32x64_f8f6f4: the block's token rows are the A
//                   operand as E2M1 nibbles, the query tile the B operand as E4M3 bytes, and the E8M0 block scales of both go into
//                   the instruction, so the accumulator IS s_ij.  A k-step is 64 columns; lane (j = lane % 32, h = lane / 32) gives it
//                   the 32 columns at 32 h of token row j — exactly MX block 2 s + h of that row: 16 bytes (one global_load_dwordx4
//                   into four of the operand's eight registers, the others zero) — and ONE scale byte, that block's.  The query
//                   operand is 32 bytes a lane (two ds_read_b128) in the 8-bit layout, 16 columns of each of the step's two blocks
//                   (maxsim_mx4_qfrag), with the scale byte of block 2 s + h.  A chunk of 128 columns is 2 k-steps = 4 MX blocks: 8 VGPRs of codes and
//                   one dword of scale bytes a lane (shifted by 8 h as it arrives, so step p reads byte 2 p by the instruction's
//                   byte select).  The chunks of the stream go through a ring of RING such buffers, loaded RING - 1 chunks ahead.
//   k_maxsim_store_mx4  rule 1''': f32 rows [rows][dim] -> codes [rows][ld / 2] and scale bytes [rows][scale pitch], 4 lanes a block.
typedef int maxsim_i32x8 __attribute__((ext_vector_type(8)));
typedef uint32_t maxsim_u32x2 __attribute__((ext_vector_type(2)));

constexpr uint32_t MAXSIM_MX_KC = 128;             // columns of a chunk: 2 k-steps of 64
constexpr uint32_t MAXSIM_MX_UNIT = 0x7f7f7f7fu;   // four E8M0 bytes 127 = 2^0: the scale next to an operand that is zero

// LDS row pitch of a query tile in BYTES (one E4M3 byte an element): ld + 16 = 16 s with s odd, as maxsim_i8_pitch.
__host__ __device__ inline uint32_t maxsim_mx4_pitch(uint32_t ld) { return ld + 16u; }
// HBM: the scale bytes of a token row, ld / 32 of them padded with 127 to whole dwords — a lane's load of a chunk's four is aligned
__host__ __device__ inline uint32_t maxsim_mx4_scale_pitch(uint32_t ld) { return (ld / 32u + 3u) / 4u * 4u; }
// LDS bytes: the query tiles as E4M3 bytes | their ld / 32 scale bytes a row | the 32 boundary flags of each of the (always 4) waves
__host__ __device__ inline size_t maxsim_mx4_lds_bytes(uint32_t ld, uint32_t tiles) {
    return (size_t)tiles * MAXSIM_BLOCK * (maxsim_mx4_pitch(ld) + ld / 32u) + (size_t)MAXSIM_MAX_WAVES * MAXSIM_BLOCK * 4u;
}

struct MaxSimMx4Args {
    MaxSimArgsT<uint8_t> a;   // the token rows are E2M1 codes, two a byte (low nibble the even element): ld / 2 BYTES a row
    const uint8_t* scales;    // [total tokens][maxsim_mx4_scale_pitch(ld)]
};

// Rules 1''' (SHIFT 2: amax lands in [4, 8), E2M1 tops at 6) and 1'''' (SHIFT 8: [256, 512), E4M3 tops at 448): the scale byte
// E + 127 = max(biased exponent of amax - SHIFT, 0) — a subnormal amax clamps to E = -127 whatever its log2 — and inv = 2^-E.
// amax 0 (every element 0 or NaN: fmaxf skipped them) or +inf: byte 127 and inv 0, which codes every element as 0.
template <int SHIFT>
__device__ __forceinline__ void maxsim_mx_scale(float amax, uint32_t& byte, float& inv) {
    const bool none = amax == 0.0f || amax == __builtin_huge_valf();
    const int e = (int)(__float_as_uint(amax) >> 23) - SHIFT;
    byte = none ? 127u : (uint32_t)(e < 0 ? 0 : e);
    inv = none ? 0.0f : __uint_as_float((254u - byte) << 23);
}
// the E2M1 code nearest v, ties to the code whose low bit is 0, saturating at 6; NaN -> 0
__device__ __forceinline__ uint32_t maxsim_e2m1(float v) {
    const float m = fabsf(v);
    const uint32_t c = (uint32_t)(m > 0.25f) + (uint32_t)(m >= 0.75f) + (uint32_t)(m > 1.25f) + (uint32_t)(m >= 1.75f) + (uint32_t)(m > 2.5f) +
                       (uint32_t)(m >= 3.5f) + (uint32_t)(m > 5.0f);
    return c ? c | ((__float_as_uint(v) >> 28) & 8u) : 0u;
}
// the E4M3 (e4m3fn) code nearest v, ties to even, subnormals at 2^-9, saturating at 448 = 0x7e; NaN -> 0
__device__ __forceinline__ uint32_t maxsim_e4m3(float v) {
    const float m = fabsf(v);
    uint32_t b = __float_as_uint(m);
    b += 0x7ffffu + ((b >> 20) & 1u);   // nearest even at 3 mantissa bits
    uint32_t c = (b >> 20) - 960u;      // (exponent, mantissa) at e4m3's bias: 2^-6 = 121 << 3 -> 8
    c = c > 0x7eu ? 0x7eu : c;
    if (m < 0.015625f) c = (uint32_t)rintf(m * 512.0f);   // below the least normal: whole steps of 2^-9 (8 of them are that normal)
    c = m == m ? c : 0u;
    return c ? c | ((__float_as_uint(v) >> 24) & 0x80u) : 0u;
}

// 4 lanes a block of 32 elements: its amax over them (order-free), then 8 codes a lane as one 32-bit store and the block's scale byte.
__global__ void __launch_bounds__(256) k_maxsim_store_mx4(const float* __restrict__ src, uint32_t* __restrict__ codes, uint8_t* __restrict__ scales,
                                                          uint64_t rows, uint32_t dim, uint32_t ld) {
    const uint32_t lane = threadIdx.x & 63u, sub = threadIdx.x & 3u, nsb = ld / 32u, sp = maxsim_mx4_scale_pitch(ld);
    const uint64_t blk = (uint64_t)blockIdx.x * 64u + (threadIdx.x >> 2);
    const bool in = blk < rows * nsb;   // (no early return: the lanes of a wave exchange below)
    const uint64_t r = in ? blk / nsb : 0;
    const uint32_t bk = in ? (uint32_t)(blk - r * nsb) : 0u, c0 = bk * 32u + sub * 8u;
    float v[8], amax = 0.0f;
#pragma unroll
    for (uint32_t e = 0; e < 8u; ++e) {
        v[e] = in && c0 + e < dim ? src[r * dim + c0 + e] : 0.0f;
        amax = fmaxf(amax, fabsf(v[e]));
    }
    amax = fmaxf(amax, maxsim_from_lane(amax, lane ^ 1u));
    amax = fmaxf(amax, maxsim_from_lane(amax, lane ^ 2u));
    if (!in) return;
    uint32_t byte, w = 0u;
    float inv;
    maxsim_mx_scale<2>(amax, byte, inv);
#pragma unroll
    for (uint32_t e = 0; e < 8u; ++e) w |= maxsim_e2m1(v[e] * inv) << (4u * e);
    codes[blk * 4u + sub] = w;   // (a row is ld / 8 = 4 nsb dwords)
    if (sub == 0u) {
        scales[r * sp + bk] = (uint8_t)byte;
        if (bk + 1u == nsb)
            for (uint32_t b = nsb; b < sp; ++b) scales[r * sp + b] = 127u;
    }
}

// The query tiles of a workgroup into LDS by rule 1'''', 4 lanes a block of 32 columns: the block's amax, then 8 E4M3 bytes a lane and
// the block's scale byte; rows past the query's own tiles are never read (nor written: the scan skips those tiles).
__device__ __forceinline__ void maxsim_mx4_stage(const float* Q, uint32_t tq_rows, uint32_t K, uint32_t PB, unsigned char* q_l, unsigned char* sq_l,
                                                 uint32_t tid, uint32_t lane) {
    const uint32_t sub = tid & 3u, nsb = K / 32u;
    for (uint32_t p = tid >> 2; p < tq_rows * nsb; p += blockDim.x >> 2) {   // (uniform over a group of 4 lanes)
        const uint32_t r = p / nsb, bk = p - r * nsb;
        const float* src = Q + (size_t)r * K + bk * 32u + sub * 8u;
        const f32x4 lo = *reinterpret_cast<const f32x4*>(src), hi = *reinterpret_cast<const f32x4*>(src + 4);
        float amax = 0.0f;
#pragma unroll
        for (int e = 0; e < 4; ++e) amax = fmaxf(fmaxf(amax, fabsf(lo[e])), fabsf(hi[e]));
        amax = fmaxf(amax, maxsim_from_lane(amax, lane ^ 1u));
        amax = fmaxf(amax, maxsim_from_lane(amax, lane ^ 2u));
        uint32_t byte;
        float inv;
        maxsim_mx_scale<8>(amax, byte, inv);
        maxsim_u32x2 o = {0u, 0u};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            o[0] |= maxsim_e4m3(lo[e] * inv) << (8 * e);
            o[1] |= maxsim_e4m3(hi[e] * inv) << (8 * e);
        }
        *reinterpret_cast<maxsim_u32x2*>(q_l + (size_t)r * PB + bk * 32u + sub * 8u) = o;
        if (sub == 0u) sq_l[r * nsb + bk] = (unsigned char)byte;
    }
}

// One chunk of a block in the ring: the two 16-B code fragments of lane (col, half) and the chunk's four scale bytes of its row,
// shifted so that byte 2 p is the block of k-step p and this half.
struct MaxSimMx4Chunk {
    maxsim_i32x4 f[2];
    uint32_t sc;
};
// Lane (col, half) takes, of each of chunk c's 2 column groups of 64, the 16 bytes (32 codes) at 32 half of token row t_first + col,
// and the dword of the row's scale bytes 4 c ...  Rows at or past `t_end` (the end of the wave's range, or a block past its last) and
// the half-step past the row pitch are zero codes under a unit scale: nothing outside the range is read.
__device__ __forceinline__ void maxsim_mx4_load(const MaxSimMx4Args& x, uint64_t t_first, uint64_t t_end, uint32_t c, uint32_t col, uint32_t half, MaxSimMx4Chunk& o) {
    const bool in = t_first + col < t_end;
    const uint32_t K = x.a.ld;
    const uint64_t row = t_first + col;
    o.sc = MAXSIM_MX_UNIT;
    if (in) o.sc = *reinterpret_cast<const uint32_t*>(x.scales + (size_t)row * maxsim_mx4_scale_pitch(K) + c * 4u) >> (8u * half);
#pragma unroll
    for (uint32_t p = 0; p < 2u; ++p) {
        o.f[p] = maxsim_i32x4{0, 0, 0, 0};
        if (in && c * MAXSIM_MX_KC + p * 64u + half * 32u < K)
            o.f[p] = *reinterpret_cast<const maxsim_i32x4*>(x.a.tokens + (size_t)row * (K / 2u) + c * (MAXSIM_MX_KC / 2u) + p * 32u + half * 16u);
    }
}
// The matching query operand of one tile for the k-step at column k0 = 64 s.  An 8-bit operand is laid out differently from a 4-bit
// one: registers 0 .. 3 of lane half h are columns k0 + 16 h .. + 15 (the step's first MX block), registers 4 .. 7 columns k0 + 32 +
// 16 h .. (its second block) — while the SCALE of block h is still the one lanes of half h supply.  So the lane reads two 16-B pieces
// 32 bytes apart and the scale byte of block 2 s + h.  Past the row pitch: zero under a unit scale (the pad of a row is never
// written: an E4M3 NaN there would poison the sum).
struct MaxSimMx4Q {
    maxsim_i32x8 v;
    uint32_t sc;
};
__device__ __forceinline__ MaxSimMx4Q maxsim_mx4_qfrag(const unsigned char* qrow, const unsigned char* srow, uint32_t k0, uint32_t half, uint32_t K) {
    const maxsim_i32x4 lo = *reinterpret_cast<const maxsim_i32x4*>(qrow + k0 + half * 16u);   // (k0 < K, a multiple of 32: the first block exists)
    maxsim_i32x4 hi = {0, 0, 0, 0};
    if (k0 + 32u < K) hi = *reinterpret_cast<const maxsim_i32x4*>(qrow + k0 + 32u + half * 16u);
    return MaxSimMx4Q{maxsim_i32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]}, k0 + half * 32u < K ? (uint32_t)srow[k0 / 32u + half] : 127u};
}
// k-step P of a chunk: A = 32 E2M1 codes (cbsz 4; four of the eight registers: the lane's own MX block, columns in order), its scale
// byte 2 P of the shifted dword; B = 32 E4M3 bytes (blgp 0) in the 8-bit layout above, its scale in byte 0.
template <int P>
__device__ __forceinline__ f32x16 maxsim_mx4_mfma(const MaxSimMx4Chunk& ch, const MaxSimMx4Q& qf, f32x16 acc) {
    const maxsim_i32x8 av = {ch.f[P][0], ch.f[P][1], ch.f[P][2], ch.f[P][3], 0, 0, 0, 0};
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, qf.v, acc, 4, 0, 2 * P, (int)ch.sc, 0, (int)qf.sc);
#else
    (void)av;
    return acc;
#endif
}

// Rules 3''' and 4''' for the finished block, k_maxsim_i8's walk with the accumulator already s_ij: down the 32 token rows in groups
// of 8 (rows 8 g .. 8 g + 3 are registers 4 g .. of half 0, the next four of half 1), run[t] the maximum so far of the open record.
template <int NT>
__device__ __forceinline__ LY_MAXSIM_FN void maxsim_mx4_fold(const MaxSimArgsT<uint8_t>& a, const f32x16 (&acc)[NT], float (&run)[NT], const MaxSimBounds& bd,
                                                             uint32_t nrows, uint32_t tq, uint32_t q, uint32_t rc0, uint32_t lane, uint32_t col) {
    const float NINF = -__builtin_huge_valf();
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        if (8u * g >= nrows) continue;
        if (8u * g + 8u <= nrows && ((bd.endmask >> (8 * g)) & 0xffu) == 0u) {
            // no record ends in these 8 rows: each half folds its own four, one exchange joins them in both halves
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                if (t != 0 && (uint32_t)t * 32u >= tq) continue;
                const float m4 = fmaxf(fmaxf(acc[t][4 * g], acc[t][4 * g + 1]), fmaxf(acc[t][4 * g + 2], acc[t][4 * g + 3]));
                float lo, hi;
                maxsim_i8_halves(m4, lo, hi);
                run[t] = fmaxf(run[t], fmaxf(lo, hi));
            }
            continue;
        }
#pragma unroll
        for (int o = 0; o < 2; ++o) {   // the owning half of rows 8 g + 4 o ..: its lanes hold the record's maximum so far
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint32_t row = 8u * g + 4u * o + e;
                if (row >= nrows) continue;
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    if (t != 0 && (uint32_t)t * 32u >= tq) continue;
                    run[t] = fmaxf(run[t], acc[t][4 * g + e]);   // (fmaxf skips a NaN s_ij: all NaN leaves -inf)
                }
                if ((bd.endmask >> row) & 1u) {   // a record ends here: rule 4''' in the owning half
                    float s = 0.0f;
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        if (t != 0 && (uint32_t)t * 32u >= tq) continue;
                        const float tile = maxsim_i8_tree((uint32_t)t * 32u + col < tq ? run[t] : 0.0f);
                        s = t == 0 ? tile : s + tile;
                        run[t] = NINF;
                    }
                    if (lane == 32u * o) {
                        const uint32_t cr = rc0 + (uint32_t)__popc(bd.endmask & ((1u << row) - 1u));
                        const bool live = !a.mask || range_live(a.mask, a.mask_words, a.crec[cr]);
                        a.S[(size_t)q * a.m + cr] = live ? score_ord(s, false) : RANGE_FAIL;
                    }
                }
            }
            // hand the maximum so far to the other half, which owns the next four rows (both halves agree after it)
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                if (t != 0 && (uint32_t)t * 32u >= tq) continue;
                float lo, hi;
                maxsim_i8_halves(run[t], lo, hi);
                run[t] = o == 0 ? lo : hi;
            }
        }
    }
}

// NT = query tiles of 32 rows the LDS holds (1, 2, 4 or 8); a query of fewer tiles skips the rest.  grid.x strides over the ranges,
// grid.y is the query; 4 waves.  RING - 1 = the chunks a load runs ahead: a chunk is 9 registers, about half of k_maxsim_i8's 16, and
// the difference goes into depth (DESIGN.md §33 has the register report behind the choice).
template <int NT>
__global__ void LY_MAXSIM_FN __launch_bounds__(MAXSIM_MAX_WAVES * 64) k_maxsim_mx4(MaxSimMx4Args x) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sm_maxsim_mx4[];
    constexpr int RING = NT <= 2 ? 6 : 4;
    const MaxSimArgsT<uint8_t>& a = x.a;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, col = lane & 31u, half = lane >> 5;
    const uint32_t wave = maxsim_uniform(tid >> 6), waves = blockDim.x >> 6;
    const uint32_t K = a.ld, NSB = K / 32u, PB = maxsim_mx4_pitch(K), nch = (K + MAXSIM_MX_KC - 1u) / MAXSIM_MX_KC;
    const uint32_t q = blockIdx.y;
    const uint64_t q_off = a.qdesc[2u * q];
    const uint32_t tq = (uint32_t)a.qdesc[2u * q + 1u], tq_rows = (tq + 31u) / 32u * 32u;
    unsigned char* q_l = sm_maxsim_mx4;
    unsigned char* sq_l = q_l + (size_t)NT * MAXSIM_BLOCK * PB;
    uint32_t* flag_l = reinterpret_cast<uint32_t*>(sq_l + (size_t)NT * MAXSIM_BLOCK * NSB) + wave * MAXSIM_BLOCK;
    maxsim_mx4_stage(a.Q + q_off, tq_rows, K, PB, q_l, sq_l, tid, lane);
    __syncthreads();   // the only workgroup barrier: from here on the waves run their own ranges
    // this lane's query column: row `col` of each tile, its E4M3 bytes and its scale bytes
    const unsigned char* qa = q_l + (size_t)col * PB;
    const unsigned char* qs = sq_l + (size_t)col * NSB;
    // one tile: the operands of the first chunk stay in registers for the whole kernel — up to 128 columns the loop reads no LDS
    MaxSimMx4Q qreg[2];
    if constexpr (NT == 1) {
        qreg[0] = maxsim_mx4_qfrag(qa, qs, 0u, half, K);
        if (64u < K) qreg[1] = maxsim_mx4_qfrag(qa, qs, 64u, half, K);
    }
    const float NINF = -__builtin_huge_valf();
    for (uint32_t r = blockIdx.x * waves + wave; r < a.n_ranges; r += gridDim.x * waves) {
        const uint32_t ca = maxsim_uniform(a.ranges[r]), cb = maxsim_uniform(a.ranges[r + 1u]);
        const uint64_t t0 = maxsim_uniform(a.cptr[ca]), t1 = maxsim_uniform(a.cptr[cb]);
        const uint32_t nb = (uint32_t)((t1 - t0 + MAXSIM_BLOCK - 1u) / MAXSIM_BLOCK);
        MaxSimMx4Chunk buf[RING];
        uint32_t lb = 0, lc = 0;   // the load cursor: block and chunk, RING - 1 chunks ahead of (b, c)
#pragma unroll
        for (int i = 0; i < RING - 1; ++i) {
            maxsim_mx4_load(x, t0 + (uint64_t)lb * MAXSIM_BLOCK, lb < nb ? t1 : 0ull, lc, col, half, buf[i]);
            if (++lc == nch) lc = 0, ++lb;
        }
        uint32_t rc0 = ca;   // the record of the block's first token
        float run[NT];       // the maximum so far of the record that is open, ONE register a tile: it runs on from block to block
        f32x16 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) run[t] = NINF;
        uint64_t rec_end = ~0ull;
        uint32_t b = 0, c = 0;
        while (b < nb) {
#pragma unroll
            for (int i = 0; i < RING; ++i) {
                if (b < nb) {
                    const uint64_t tb = t0 + (uint64_t)b * MAXSIM_BLOCK;
                    if (c == 0u) {
                        // the ends of the records from rc0 on, asked for BEFORE the chunk ahead: the epilogue's wait then leaves that one in flight
                        rec_end = ~0ull;
                        if (lane < 32u && (uint64_t)rc0 + 1u + lane <= cb) rec_end = a.cptr[rc0 + 1u + lane];
#pragma unroll
                        for (int t = 0; t < NT; ++t) acc[t] = f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
                    }
                    maxsim_mx4_load(x, t0 + (uint64_t)lb * MAXSIM_BLOCK, lb < nb ? t1 : 0ull, lc, col, half, buf[(i + RING - 1) % RING]);
                    if (++lc == nch) lc = 0, ++lb;
                    const uint32_t kc = c * MAXSIM_MX_KC;
                    // a token fragment meets every tile before the next one: consecutive MFMAs write different accumulators
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        if (t != 0 && (uint32_t)t * 32u >= tq) continue;
                        const MaxSimMx4Q qf = NT == 1 && c == 0u ? qreg[0] : maxsim_mx4_qfrag(qa + (size_t)t * 32u * PB, qs + (size_t)t * 32u * NSB, kc, half, K);
                        acc[t] = maxsim_mx4_mfma<0>(buf[i], qf, acc[t]);
                    }
                    if (kc + 64u < K) {
#pragma unroll
                        for (int t = 0; t < NT; ++t) {
                            if (t != 0 && (uint32_t)t * 32u >= tq) continue;
                            const MaxSimMx4Q qf = NT == 1 && c == 0u ? qreg[1] : maxsim_mx4_qfrag(qa + (size_t)t * 32u * PB, qs + (size_t)t * 32u * NSB, kc + 64u, half, K);
                            acc[t] = maxsim_mx4_mfma<1>(buf[i], qf, acc[t]);
                        }
                    }
                    if (c + 1u == nch) {   // the block's last chunk: rules 3''' and 4''', the scores of the records that end in it
                        const uint32_t nrows = t1 - tb < MAXSIM_BLOCK ? (uint32_t)(t1 - tb) : MAXSIM_BLOCK;   // rows of the block inside the range
                        const MaxSimBounds bd = maxsim_h16_bounds(rec_end, tb, b + 1u < nb, lane, col, flag_l);
                        maxsim_mx4_fold<NT>(a, acc, run, bd, nrows, tq, q, rc0, lane, col);
                        rc0 += bd.n_adv;
                        c = 0u;
                        ++b;
                    } else {
                        ++c;
                    }
                }
            }
        }
    }
}

// ---- candidate lists (include/lynse_hip.h, MULTI-VECTOR RERANK) ----------------------------------------------------
//   k_maxsim_cand_h16 / k_maxsim_cand_i8   MaxSim over per-query candidate lists: a gather, not the scan with an indirection.  A
//                   work item is one (query, candidate record) pair and ONE WAVE owns it; the workgroups of a query (grid.y) take
//                   its candidates grid-stride over grid.x.  A wave walks its record's token rows in blocks of 32; every block
//                   belongs to one record, so nothing of the scans' boundary machinery exists here: rows past the record's end are
//                   not read and are masked by the wave-uniform row count.  Operand roles for BOTH dtypes are §30's — the token rows
//                   are A, the query tile B, a lane holds one query column and 16 token rows — so the max over a record's tokens is
//                   v_max_f32 down the lane's own registers into one running register a tile, block after block, and ONE
//                   v_permlane32_swap a tile and record joins the halves.  In bytes the two stores look alike: of each 64 bytes of a
//                   row half h owns the 32 at 32 h, two 16-B fragments — so one body serves both, fragment f of a chunk in the
//                   scan's k-step order.  The chunks of the wave's whole item stream go through one statically indexed ring, loaded
//                   RING - 1 chunks ahead: the first loads of the next candidate are in flight before this record's epilogue.  The
//                   extents of up to 64 items sit one per lane (loaded together), read by v_readlane as the two cursors cross records.
//   S[q][slot] = the score_ord image of the slot-th candidate of query q, RANGE_FAIL in the slots past the query's list.
struct MaxSimCandArgs {
    const unsigned char* tokens;   // [total tokens][row bytes]: halves (2 ld) or codes (ld)
    const float* scales;           // i8: [total tokens]
    uint32_t ld;
    const uint64_t* cptr;          // m + 1 token offsets of the records that have tokens
    const uint32_t* cand;          // compact record numbers (indices into cptr), strictly ascending within a query's list
    const uint64_t* cand_ptr;      // nq + 1 offsets into cand; NULL: cand[0 .. n_shared) is every query's list
    uint32_t n_shared;
    uint32_t pitch;                // slots of a query in S: the longest list
    const float* Q;                // as for the scans
    const uint64_t* qdesc;
    uint32_t* S;                   // [nq][pitch]
};

template <bool I8> struct MaxSimCandAcc { using T = f32x16; };
template <> struct MaxSimCandAcc<true> { using T = maxsim_i32x16; };

__device__ __forceinline__ uint64_t maxsim_lane64(uint64_t v, uint32_t l) {
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)l) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)l);
}

// A position in the wave's item stream, wave-uniform: item j of the batch, the first token row of its current block, the record's
// end, the chunk of the block.  step() moves on one chunk; true when that left the record (and entered the next, if there is one).
struct MaxSimCursor {
    uint32_t j, c;
    uint64_t t, t_end;
    __device__ __forceinline__ void enter(uint64_t e0, uint64_t e1) { t = maxsim_lane64(e0, j), t_end = maxsim_lane64(e1, j), c = 0u; }
    __device__ __forceinline__ bool step(uint32_t nch, uint32_t nit, uint64_t e0, uint64_t e1) {
        if (++c < nch) return false;
        c = 0u, t += MAXSIM_BLOCK;
        if (t < t_end) return false;
        if (++j < nit) enter(e0, e1);
        return true;
    }
};

// One chunk of the cursor's block into a ring buffer: lane (col, half) takes, of each of the chunk's F / 2 groups of 64 row bytes,
// the 32 at 32 half of token row cu.t + col.  Rows at or past the record's end and bytes past the row are zero and NOT read.
template <int F>
__device__ __forceinline__ void maxsim_cand_load(const unsigned char* tokens, uint32_t RB, const MaxSimCursor& cu, uint32_t col, uint32_t half, maxsim_i32x4 (&f)[F]) {
    const bool in = cu.t + col < cu.t_end;
    const uint32_t kcb = cu.c * (uint32_t)F * 32u + half * 32u;
    const unsigned char* src = tokens + (size_t)(cu.t + col) * RB + kcb;
#pragma unroll
    for (int p = 0; p < F / 2; ++p) {
        f[2 * p] = maxsim_i32x4{0, 0, 0, 0};
        f[2 * p + 1] = maxsim_i32x4{0, 0, 0, 0};
        if (in && kcb + (uint32_t)p * 64u < RB) {
            f[2 * p] = *reinterpret_cast<const maxsim_i32x4*>(src + p * 64);
            f[2 * p + 1] = *reinterpret_cast<const maxsim_i32x4*>(src + p * 64 + 16);
        }
    }
}

// NT = query tiles of 32 rows the LDS holds; I8: codes + scales and rules 2" - 4", else halves and rules 3, 4.  RING and the chunk
// (F fragments of 16 B a lane) are those of the scan of the dtype.
template <int NT, bool I8>
__device__ __forceinline__ LY_MAXSIM_FN void maxsim_cand(const MaxSimCandArgs& a, unsigned char* q_l) {
    constexpr int RING = I8 ? (NT <= 2 ? 4 : 3) : (NT <= 2 ? 3 : 2);
    constexpr int F = I8 ? 4 : (NT == 8 ? 4 : 8);
    constexpr uint32_t KCB = (uint32_t)F * 32u;   // row bytes of a chunk
    using Acc = typename MaxSimCandAcc<I8>::T;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, col = lane & 31u, half = lane >> 5;
    const uint32_t wave = maxsim_uniform(tid >> 6), waves = blockDim.x >> 6;
    const uint32_t K = a.ld, RB = I8 ? K : 2u * K, PB = RB + 16u, nch = (RB + KCB - 1u) / KCB;   // (PB: maxsim_i8_pitch / maxsim_h16_pitch)
    const uint32_t q = blockIdx.y;
    const uint64_t q_off = a.qdesc[2u * q];
    const uint32_t tq = (uint32_t)a.qdesc[2u * q + 1u], tq_rows = (tq + 31u) / 32u * 32u;
    float* sq_l = reinterpret_cast<float*>(q_l + (size_t)NT * MAXSIM_BLOCK * PB);
    if constexpr (I8) maxsim_i8_stage(a.Q + q_off, tq_rows, K, PB, q_l, sq_l, tid, lane);
    else maxsim_h16_stage(a.Q + q_off, tq_rows, (uint32_t)NT * 32u, K, PB, q_l, tid);
    __syncthreads();   // the only barrier
    // this lane's query column: row `col` of each tile, its bytes at 32 half of each group of 64; i8: its scale
    const unsigned char* qa = q_l + (size_t)col * PB + half * 32u;
    float sq[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) sq[t] = I8 && (uint32_t)t * 32u + col < tq ? sq_l[(uint32_t)t * 32u + col] : 0.0f;
    maxsim_i32x4 qreg[F];   // one tile: the fragments of the first chunk stay in registers
    if constexpr (NT == 1) {
#pragma unroll
        for (int f = 0; f < F; ++f) {
            qreg[f] = maxsim_i32x4{0, 0, 0, 0};
            if ((uint32_t)(f >> 1) * 64u + half * 32u < RB) qreg[f] = *reinterpret_cast<const maxsim_i32x4*>(qa + (f >> 1) * 64 + (f & 1) * 16);
        }
    }
    uint64_t c0 = 0;
    uint32_t len = a.n_shared;
    if (a.cand_ptr) {
        c0 = a.cand_ptr[q];
        len = (uint32_t)(a.cand_ptr[q + 1u] - c0);
    }
    uint32_t* Sq = a.S + (size_t)q * a.pitch;
    for (uint32_t s = len + blockIdx.x * blockDim.x + tid; s < a.pitch; s += gridDim.x * blockDim.x) Sq[s] = RANGE_FAIL;
    const uint32_t w = blockIdx.x * waves + wave, W = gridDim.x * waves;
    if (w >= len) return;
    const uint32_t mine = (len - w + W - 1u) / W;   // the wave's items: slots w, w + W, ...
    const float NINF = -__builtin_huge_valf();
    for (uint32_t jb = 0; jb < mine; jb += 64u) {
        const uint32_t nit = mine - jb < 64u ? mine - jb : 64u;
        uint64_t e0 = 0, e1 = 0;   // lane l: the token rows [e0, e1) of item jb + l
        if (lane < nit) {
            const uint32_t rec = a.cand[c0 + w + (uint64_t)(jb + lane) * W];
            e0 = a.cptr[rec], e1 = a.cptr[rec + 1u];
        }
        MaxSimCursor lc, cc;   // the load cursor runs RING - 1 chunks ahead of the compute cursor, across records
        lc.j = 0u, lc.enter(e0, e1);
        cc = lc;
        maxsim_i32x4 buf[RING][F];
#pragma unroll
        for (int i = 0; i < RING - 1; ++i)
            if (lc.j < nit) {
                maxsim_cand_load<F>(a.tokens, RB, lc, col, half, buf[i]);
                lc.step(nch, nit, e0, e1);
            }
        float run[NT];   // the maximum so far of the record, one register a tile
        Acc acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) run[t] = NINF;
        while (cc.j < nit) {
#pragma unroll
            for (int i = 0; i < RING; ++i) {
                if (cc.j < nit) {
                    const bool last = cc.c + 1u == nch;
                    const uint32_t nrows = cc.t_end - cc.t < MAXSIM_BLOCK ? (uint32_t)(cc.t_end - cc.t) : MAXSIM_BLOCK;
                    if (cc.c == 0u) {
#pragma unroll
                        for (int t = 0; t < NT; ++t) acc[t] = Acc{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
                    }
                    // i8: the scales of this half's 16 rows (register v is row 8 (v / 4) + 4 half + v % 4), ahead of the block's last
                    // MFMAs; rows past the record are not read
                    f32x4 sc[4];
                    if (I8 && last) {
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            const uint32_t r0 = 8u * g + 4u * half;
                            if (r0 + 4u <= nrows) {
                                sc[g] = *reinterpret_cast<const maxsim_f32x4_u*>(a.scales + cc.t + r0);
                            } else {
#pragma unroll
                                for (uint32_t e = 0; e < 4u; ++e) sc[g][e] = r0 + e < nrows ? a.scales[cc.t + r0 + e] : 0.0f;
                            }
                        }
                    }
                    if (lc.j < nit) {
                        maxsim_cand_load<F>(a.tokens, RB, lc, col, half, buf[(i + RING - 1) % RING]);
                        lc.step(nch, nit, e0, e1);
                    }
                    const uint32_t kcb = cc.c * KCB;
#pragma unroll
                    for (int f = 0; f < F; ++f) {
                        const uint32_t off = kcb + (uint32_t)(f >> 1) * 64u;   // the group of 64 row bytes; half h of it, bytes 16 (f & 1) ..
                        if (off >= RB) continue;
#pragma unroll
                        for (int t = 0; t < NT; ++t) {
                            if (t != 0 && (uint32_t)t * 32u >= tq) continue;
                            maxsim_i32x4 bv = {0, 0, 0, 0};
                            if (NT == 1 && cc.c == 0u) bv = qreg[f];
                            else if (!I8 || off + half * 32u < RB) bv = *reinterpret_cast<const maxsim_i32x4*>(qa + (size_t)t * 32u * PB + off + (uint32_t)(f & 1) * 16u);
                            if constexpr (I8) acc[t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(buf[i][f], bv, acc[t], 0, 0, 0);
                            else acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(half8, buf[i][f]), __builtin_bit_cast(half8, bv), acc[t], 0, 0, 0);
                        }
                    }
                    if (!last) {
                        ++cc.c;
                        continue;
                    }
                    // the block is complete: down the lane's 16 rows into the running maximum (fmaxf skips a NaN: rule 3)
                    const int lim = (int)nrows - 4 * (int)half;   // register v holds a row of the record iff 8 (v / 4) + v % 4 < lim
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        if (t != 0 && (uint32_t)t * 32u >= tq) continue;
                        float v[16];
#pragma unroll
                        for (int k = 0; k < 16; ++k) v[k] = I8 ? (float)acc[t][k] * sc[k >> 2][k & 3] : (float)acc[t][k];
                        if (nrows < MAXSIM_BLOCK) {
#pragma unroll
                            for (int k = 0; k < 16; ++k) v[k] = 8 * (k >> 2) + (k & 3) < lim ? v[k] : NINF;
                        }
#pragma unroll
                        for (int k = 0; k < 16; ++k) run[t] = fmaxf(run[t], v[k]);
                    }
                    const uint32_t slot = w + (jb + cc.j) * W;
                    if (!cc.step(nch, nit, e0, e1)) continue;
                    // the record is complete: one exchange a tile joins the halves, then the sum over the query's tokens
                    float s = 0.0f;
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        if (t != 0 && (uint32_t)t * 32u >= tq) continue;
                        float lo, hi;
                        maxsim_i8_halves(run[t], lo, hi);
                        const float m = fmaxf(lo, hi);
                        run[t] = NINF;
                        if constexpr (I8) {   // rules 3" and 4": the scaled maxima through the pairwise tree, the tiles in order
                            const float tile = maxsim_i8_tree((uint32_t)t * 32u + col < tq ? sq[t] * m : 0.0f);
                            s = t == 0 ? tile : s + tile;
                        } else {   // rule 4: m_i sits in lane i; ((m_0 + m_1) + m_2) + ... one v_readlane and one add a query token
                            const uint32_t nv = tq - (uint32_t)t * 32u < 32u ? tq - (uint32_t)t * 32u : 32u;
                            for (uint32_t i2 = 0; i2 < nv; ++i2) {
                                const float mi = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(m), (int)i2));
                                s = t == 0 && i2 == 0u ? mi : s + mi;
                            }
                        }
                    }
                    if (lane == 0u) Sq[slot] = score_ord(s, false);
                }
            }
        }
    }
}

// grid.x strides over a query's candidates, grid.y is the query; blockDim.x / 64 waves (up to 4).  The LDS is the scan's plan.
template <int NT>
__global__ void LY_MAXSIM_FN __launch_bounds__(MAXSIM_MAX_WAVES * 64) k_maxsim_cand_h16(MaxSimCandArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sm_maxsim_cand_h16[];
    maxsim_cand<NT, false>(a, sm_maxsim_cand_h16);
}
template <int NT>
__global__ void LY_MAXSIM_FN __launch_bounds__(MAXSIM_MAX_WAVES * 64) k_maxsim_cand_i8(MaxSimCandArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sm_maxsim_cand_i8[];
    maxsim_cand<NT, true>(a, sm_maxsim_cand_i8);
}

}  // namespace lynse
