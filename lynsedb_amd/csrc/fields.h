// fields.h — field filters (FieldStore::query_from_index, src/storage/field_store.rs:1527-1590): the compiled predicate of a `where`
// string evaluated for every row over typed field columns in HBM.  include/lynse_hip.h FIELD FILTERS, DESIGN.md §25.
//   k_field_filter   one lane per row, grid-stride in whole waves.  A column is a one-byte tag and an 8-byte payload per row (array
//                    fields add a CSR of (tag, payload) elements); a leaf is evaluated from the two, the leaves are combined as AND or
//                    OR, and the wave64 ballot of 64 consecutive rows IS the u64 word of the reference's BitSet (k_pack_bits uses the
//                    same property).  Bits at and beyond n are zero; the matches are counted by a popcount per wave and one vector
//                    atomic per wave.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lynse {

constexpr int FIELD_NT = 256;
constexpr uint32_t FIELD_MAX_LEAVES = 32;
constexpr uint64_t FIELD_MAX_KEYS = 65536;
// the tag of a row's value (IndexKey / insert_value, field_store.rs:165-191, :469-517)
enum : uint32_t { FTAG_MISSING = 0, FTAG_NULL = 1, FTAG_BOOL = 2, FTAG_INT = 3, FTAG_FLOAT = 4, FTAG_STR = 5, FTAG_ARRAY = 6, FTAG_OBJECT = 7, FTAG_COUNT = 8 };
enum : uint32_t { FLEAF_EQ = 0, FLEAF_NUM_RANGE = 1, FLEAF_KEYSET = 2, FLEAF_STRTABLE = 3, FLEAF_CONTAINS = 4 };
enum : uint32_t { FOP_LT = 0, FOP_LE = 1, FOP_GT = 2, FOP_GE = 3 };
constexpr uint32_t FIELD_KEYSET_HEAD = FTAG_COUNT + 1;   // words of segment starts in front of a key list

// A leaf with its column resolved to device pointers (the host builds these from lynse_hip_field_leaf).
struct FieldLeafDev {
    const uint8_t* tags;         // [n]; NULL = a field no row carries: the leaf matches nothing
    const uint64_t* payloads;    // [n]
    const uint64_t* arr_ptr;     // [n_arrays + 1]; the payload of an FTAG_ARRAY row is its index here
    const uint8_t* etags;        // elements
    const uint64_t* epayloads;
    uint64_t n_arrays;
    const uint64_t* aux;         // KEYSET: FIELD_KEYSET_HEAD segment starts, then the payloads ascending within a tag; STRTABLE: bit table over codes
    uint64_t aux_len;            // KEYSET: keys; STRTABLE: codes covered
    uint64_t key;                // EQ / CONTAINS: payload; NUM_RANGE: the normalised bits of the literal
    uint32_t kind, op, flags, key_tag;
};

struct FieldFilterArgs {
    const FieldLeafDev* leaves;
    uint32_t n_leaves;
    uint32_t any;                // 0 = AND of the leaves, 1 = OR
    uint64_t n;
    uint64_t* words;             // [(n + 63) / 64]
    unsigned long long* count;   // zeroed by the caller
};

// normalize_f64_bits (field_store.rs:223-230): unsigned order of the result = numeric order, -0.0 before +0.0
__device__ __forceinline__ uint64_t field_norm_bits(double f) {
    const uint64_t b = (uint64_t)__double_as_longlong(f);
    return (b >> 63) == 0 ? (b | (1ull << 63)) : ~b;
}

__device__ __forceinline__ bool field_leaf_eval(const FieldLeafDev& L, uint64_t r) {
    if (!L.tags) return false;
    const uint32_t t = L.tags[r];
    const uint64_t p = L.payloads[r];
    switch (L.kind) {
    case FLEAF_EQ:
        return t == L.key_tag && p == L.key;
    case FLEAF_NUM_RANGE: {
        if (t == FTAG_STR) return L.op >= FOP_GT;   // RangeKey's derived order: every Text after every Number
        if (t != FTAG_INT && t != FTAG_FLOAT) return false;
        const uint64_t b = t == FTAG_FLOAT ? p : field_norm_bits((double)(long long)p);   // an Int compares as `as f64` rounds it
        return L.op == FOP_LT ? b < L.key : L.op == FOP_LE ? b <= L.key : L.op == FOP_GT ? b > L.key : b >= L.key;
    }
    case FLEAF_KEYSET: {
        if (t >= FTAG_COUNT) return false;
        uint64_t lo = L.aux[t], hi = L.aux[t + 1];   // the keys of this tag (the host has checked the starts against aux_len)
        const uint64_t* keys = L.aux + FIELD_KEYSET_HEAD;
        while (lo < hi) {
            const uint64_t mid = lo + ((hi - lo) >> 1);
            const uint64_t v = keys[mid];
            if (v == p) return true;
            if (v < p) lo = mid + 1;
            else hi = mid;
        }
        return false;
    }
    case FLEAF_STRTABLE:
        if (t == FTAG_INT || t == FTAG_FLOAT) return (L.flags & 1u) != 0u;   // a Text literal under < / <=: every Number is before it
        return t == FTAG_STR && p < L.aux_len && ((L.aux[p >> 6] >> (p & 63ull)) & 1ull) != 0ull;
    case FLEAF_CONTAINS: {
        if (t != FTAG_ARRAY || p >= L.n_arrays) return false;
        const uint64_t e1 = L.arr_ptr[p + 1];
        for (uint64_t e = L.arr_ptr[p]; e < e1; ++e)
            if (L.etags[e] == L.key_tag && L.epayloads[e] == L.key) return true;
        return false;
    }
    default:
        return false;
    }
}

__global__ void __launch_bounds__(FIELD_NT) k_field_filter(FieldFilterArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t n64 = (a.n + 63ull) & ~63ull;   // a wave's 64 rows begin at a multiple of 64: whole waves make every trip
    const uint64_t step = (uint64_t)gridDim.x * FIELD_NT;
    uint32_t mine = 0;
    for (uint64_t r = (uint64_t)blockIdx.x * FIELD_NT + threadIdx.x; r < n64; r += step) {
        bool pass = false;
        if (r < a.n) {
            pass = a.any == 0u;
            for (uint32_t l = 0; l < a.n_leaves; ++l) {
                const bool m = field_leaf_eval(a.leaves[l], r);
                pass = a.any ? (pass || m) : (pass && m);
            }
        }
        const uint64_t b = __ballot(pass);
        if (lane == 0) {
            a.words[r >> 6] = b;
            mine += (uint32_t)__popcll(b);
        }
    }
    if (lane == 0 && mine) atomicAdd(a.count, (unsigned long long)mine);
}

// Named vector fields (include/lynse_hip.h NAMED VECTOR FIELDS): a field's rows are a subset of the collection's rows in
// another order, so the BitSet words of a filter over collection rows are rewritten into field-row space.
//   k_bitset_remap   one lane per field row, grid-stride in whole waves.  A coalesced load of row_of[r], a gather of the 8-byte source
//                    word that holds bit row_of[r] (from `src` below n_src, from `tail` at row_of[r] - n_src above it) and a bit test;
//                    ROWMAP_NONE gives 0.  The wave64 ballot of 64 consecutive field rows IS the output word, as in k_field_filter:
//                    ceil(n_out / 64) words are written, bits at and beyond n_out are zero, the count is a popcount per wave and one
//                    vector atomic per wave.  The host has checked every row_of[r] against n_src + n_tail before the launch.
constexpr uint32_t ROWMAP_NONE = 0xFFFFFFFFu;

struct BitsetRemapArgs {
    const uint32_t* row_of;      // [n_out]
    uint64_t n_out;
    const uint64_t* src;         // [(n_src + 63) / 64]
    uint64_t n_src;
    const uint64_t* tail;        // [(n_tail + 63) / 64]; NULL when n_tail == 0
    uint64_t n_tail;
    uint64_t* words;             // [(n_out + 63) / 64]
    unsigned long long* count;   // zeroed by the caller
};

__global__ void __launch_bounds__(FIELD_NT) k_bitset_remap(BitsetRemapArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t n64 = (a.n_out + 63ull) & ~63ull;
    const uint64_t step = (uint64_t)gridDim.x * FIELD_NT;
    uint32_t mine = 0;
    for (uint64_t r = (uint64_t)blockIdx.x * FIELD_NT + threadIdx.x; r < n64; r += step) {
        bool pass = false;
        if (r < a.n_out) {
            const uint32_t j = a.row_of[r];
            if (j != ROWMAP_NONE) {
                if (j < a.n_src) {
                    pass = ((a.src[j >> 6] >> (j & 63u)) & 1ull) != 0ull;
                } else {
                    const uint64_t t = (uint64_t)j - a.n_src;
                    if (t < a.n_tail) pass = ((a.tail[t >> 6] >> (t & 63ull)) & 1ull) != 0ull;
                }
            }
        }
        const uint64_t b = __ballot(pass);
        if (lane == 0) {
            a.words[r >> 6] = b;
            mine += (uint32_t)__popcll(b);
        }
    }
    if (lane == 0 && mine) atomicAdd(a.count, (unsigned long long)mine);
}

}  // namespace lynse
