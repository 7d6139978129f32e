// graph.h — the device code the graph indexes share (hnsw.h: HNSW-*, diskann.h: DISKANN-*): the graph distance and the wave helpers,
// the LDS layout of a search kernel, the two-heap beam over one level of lists (search_layer, hnsw.rs:625-699) and the rank sort of
// its result.  DESIGN.md §19 and §21 hold the reasoning.  A search kernel seeds R and C in its own way (k_hnsw_search: the node its
// greedy descent ends at; k_vamana_search: the entry and the anchors), runs graph_beam and writes R out through graph_emit_ranked.
// Every order is the total order (distance, node): a key is make_key(d, node, ascending) (common.h), so which array slot an entry
// sits in never matters — pops, evictions and the final sort are decided by the keys alone.  The two comparisons on the distance alone
// (c.dist > worst.dist, d < worst.dist) are taken on the high words of the keys, the order-preserving images of the distances: the same
// predicate (no NaN, -0 == +0 by make_key), and the form hipcc 7.2 builds — comparing the decoded floats crashed its instruction selection.
#pragma once

#include "kernels.h"

namespace lynse {

constexpr uint32_t GRAPH_PAD = 0xffffffffu;

// the graph distance: compute_distance_f32 in the single-row form, negated for IP (hnsw.rs:536-543); NaN -> +inf at once
__device__ __forceinline__ float graph_dist(int metric, const float* q, const float* __restrict__ v, uint32_t D, int g) {
    float s = exact_score<32>(metric, LYNSE_IPFORM_SINGLE, q, v, D, g);
    if (metric == M_IP) s = -s;
    return s != s ? LY_INF : s;
}

__device__ __forceinline__ uint32_t graph_rank(uint64_t mask, int lane) { return (uint32_t)__popcll(mask & ((1ull << lane) - 1ull)); }

// lane l's value as a wave-uniform (scalar) one: l must be uniform.  The admission loops branch on these, so their control flow is scalar.
__device__ __forceinline__ float graph_lane(float v, uint32_t l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), (int)l)); }
__device__ __forceinline__ uint32_t graph_lane(uint32_t v, uint32_t l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)l); }
__device__ __forceinline__ uint64_t graph_uniform(uint64_t v) {
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
}

// The slot of the largest key of R (keys are distinct: one per node).  Out of line, like graph_compact: the admission loop stays small.
__device__ __noinline__ uint32_t graph_argmax(const uint64_t* Rk, uint32_t Rn, int lane) {
    uint64_t mx = 0ull;
    uint32_t mp = 0;
    for (uint32_t i = lane; i < Rn; i += 64) {
        const uint64_t kx = Rk[i];
        if (kx > mx) { mx = kx; mp = i; }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t ok = __shfl_xor(mx, o);
        const uint32_t op = __shfl_xor(mp, o);
        if (ok > mx) { mx = ok; mp = op; }
    }
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)mp);
}

// Drops the entries of C beyond worst.dist (wd = the order-preserving image of it: the high word of a key) in place; the new count.
__device__ __noinline__ uint32_t graph_compact(uint64_t* Ck, uint32_t Cn, uint32_t wd, int lane) {
    uint32_t w = 0;
    for (uint32_t base = 0; base < Cn; base += 64) {
        const uint32_t i = base + lane;
        const uint64_t kx = i < Cn ? Ck[i] : 0ull;
        const bool keep = i < Cn && (uint32_t)(kx >> 32) <= wd;
        const uint64_t km = __ballot(keep);
        __syncthreads();
        if (keep) Ck[w + graph_rank(km, lane)] = kx;
        w += (uint32_t)__popcll(km);
        __syncthreads();
    }
    return w;
}

// The dynamic LDS of a search kernel (one wave per query), stated once for the kernel that carves it and the host that sizes it.
struct GraphSearchLds {
    uint64_t* Rk;    // ef result keys, unordered
    uint64_t* Ck;    // c_cap candidate keys, unordered
    uint32_t* lst;   // 64 node slots: the unvisited neighbours of one expansion (and a kernel's start nodes), stored order
    float* qv;       // the query, D floats

    __host__ __device__ static constexpr size_t bytes(uint32_t ef, uint32_t c_cap, uint32_t D) {
        return ((size_t)ef + c_cap) * 8 + 64 * 4 + (size_t)D * 4;
    }
    __device__ __forceinline__ GraphSearchLds(unsigned char* smem, uint32_t ef, uint32_t c_cap)
        : Rk(reinterpret_cast<uint64_t*>(smem)), Ck(Rk + ef), lst(reinterpret_cast<uint32_t*>(Ck + c_cap)), qv(reinterpret_cast<float*>(lst + 64)) {}
};

// The beam's registers.  A kernel seeds them with R and C (both non-empty, worst = R[worst_pos] the largest key of R, the nodes of C
// marked visited) and reads Rn, scored and broken afterwards.
struct GraphBeamState {
    uint32_t Rn, Cn, worst_pos;
    uint64_t worst;
    uint32_t scored;   // distances scored so far
    bool broken;       // C outgrew c_cap: *status = 1, no result
};

// The beam over the lists adj[n][width] (GRAPH_PAD after the last neighbour, no neighbour twice): pop the closest candidate, mark and
// gather its unvisited neighbours, score them 8 at a time (8 groups of 8 lanes, the single-row kernels), admit them in stored order.
// vis: this query's visited bits.  c_cap bounds C: 2 ef + 8 for HNSW, 2 ef + 8 + VAMANA_STARTS for DiskANN.
__device__ __forceinline__ void graph_beam(const float* V, uint32_t ld, uint32_t D, int metric, const uint32_t* adj, uint32_t width,
                                           const GraphSearchLds& lds, uint32_t ef, uint32_t c_cap, uint32_t* vis, uint32_t* status, GraphBeamState& state) {
    uint64_t* const Rk = lds.Rk;
    uint64_t* const Ck = lds.Ck;
    uint32_t* const lst = lds.lst;
    const float* const qv = lds.qv;
    const int lane = threadIdx.x, g = lane & 7, grp = lane >> 3;
    uint32_t Rn = state.Rn, Cn = state.Cn, worst_pos = state.worst_pos, scored = state.scored;
    uint64_t worst = state.worst;
    bool broken = state.broken;
    while (Cn && !broken) {
        // pop the closest candidate
        uint64_t best = KEY_SENTINEL;
        uint32_t bpos = 0;
        for (uint32_t i = lane; i < Cn; i += 64) {
            const uint64_t kx = Ck[i];
            if (kx < best) { best = kx; bpos = i; }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const uint64_t ok = __shfl_xor(best, o);
            const uint32_t op = __shfl_xor(bpos, o);
            if (ok < best) { best = ok; bpos = op; }
        }
        best = graph_uniform(best);
        bpos = (uint32_t)__builtin_amdgcn_readfirstlane((int)bpos);
        __syncthreads();
        if (lane == 0) Ck[bpos] = Ck[Cn - 1];
        --Cn;
        __syncthreads();
        if (Rn >= ef && (uint32_t)(best >> 32) > (uint32_t)(worst >> 32)) break;   // c.dist > worst.dist, on the order-preserving images
        const uint32_t c = key_row(best);
        // its unvisited neighbours, in stored order
        const uint32_t nb = (uint32_t)lane < width ? adj[(size_t)c * width + lane] : GRAPH_PAD;
        bool fresh = false;
        if (nb != GRAPH_PAD) fresh = ((atomicOr(&vis[nb >> 5], 1u << (nb & 31u)) >> (nb & 31u)) & 1u) == 0u;
        const uint64_t um = __ballot(fresh);
        const uint32_t cnt = (uint32_t)__popcll(um);
        if (fresh) lst[graph_rank(um, lane)] = nb;
        __syncthreads();
        scored += cnt;
        for (uint32_t b = 0; b < cnt && !broken; b += 8) {
            // Room for the 8 admissions of this step.  C only nears its capacity while R is full; worst.dist never rises then, so an
            // entry beyond it can only ever end the search when it is popped — dropping it ends the search the same way (C runs empty).
            // HNSW, c_cap = 2 ef + 8: what stays is in R or ties with worst.dist: fewer than 2 ef entries.
            // DiskANN, c_cap = 2 ef + 8 + 33: while R is not full C holds nothing R does not (fewer than ef entries).  With R
            // full, what a compaction keeps is in R, was evicted from R at worst.dist (at most ef - 1) or is a start that lost the
            // start phase and ties with worst.dist (at most 32): 2 ef + 31 entries.
            if (Cn + 8 > c_cap) {
                Cn = graph_compact(Ck, Cn, (uint32_t)(worst >> 32), lane);
                if (Cn + 8 > c_cap) {
                    if (lane == 0) *status = 1u;
                    broken = true;
                }
            }
            if (!broken) {
                const uint32_t idx = b + grp;
                const uint32_t node = lst[idx < cnt ? idx : b];
                const float d = graph_dist(metric, qv, V + (size_t)node * ld, D, g);
                const uint32_t nbt = cnt - b < 8u ? cnt - b : 8u;
                for (uint32_t t = 0; t < nbt; ++t) {
                    const float dt = graph_lane(d, t * 8);
                    const uint32_t nt = graph_lane(node, t * 8);
                    const bool full = Rn >= ef;
                    const uint64_t key = make_key(dt, nt, true);
                    if (!full || (uint32_t)(key >> 32) < (uint32_t)(worst >> 32)) {   // d < worst.dist, strict and on the distance alone
                        // admitted to C and R; with R full the new entry is below the maximum, which leaves: its slot
                        if (lane == 0) {
                            Ck[Cn] = key;
                            Rk[full ? worst_pos : Rn] = key;
                        }
                        ++Cn;
                        if (!full) ++Rn;
                        __syncthreads();
                        worst_pos = graph_argmax(Rk, Rn, lane);
                        worst = graph_uniform(Rk[worst_pos]);
                    }
                }
            }
        }
    }
    __syncthreads();
    state.Rn = Rn; state.Cn = Cn; state.worst_pos = worst_pos; state.scored = scored;
    state.worst = worst;
    state.broken = broken;
}

// R in the order (dist, node): emit(rank, key) for every entry of rank below `want`, from the lane that holds it
template <class Emit>
__device__ __forceinline__ void graph_emit_ranked(const uint64_t* Rk, uint32_t Rn, uint32_t want, Emit&& emit) {
    for (uint32_t i = threadIdx.x; i < Rn; i += 64) {
        const uint64_t kx = Rk[i];
        uint32_t rank = 0;
        for (uint32_t j = 0; j < Rn; ++j) rank += Rk[j] < kx ? 1u : 0u;
        if (rank < want) emit(rank, kx);
    }
}

}  // namespace lynse
