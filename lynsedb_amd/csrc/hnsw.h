// hnsw.h — HNSW-{IP,L2,COS} on a FLAT handle (HNSWIndex, src/index/hnsw.rs): the graph beam search and the neighbour-selection
// heuristic of the bulk build.  include/lynse_hip.h states the contract (the HNSW rule block), DESIGN.md §19 the reasoning.
//   k_hnsw_search   one wave per query: greedy descent over the upper levels, then the two-heap beam at level 0 (search_layer,
//                   hnsw.rs:625-699).  The query, R (results) and C (candidates) live in LDS; the 8 groups of 8 lanes score 8
//                   neighbours at a time with the single-row kernels, admission then runs in stored order.
//   k_hnsw_select   one wave per (node, level): select_neighbors_heuristic (hnsw.rs:550-602) over a sorted candidate list
//   k_hnsw_gather   rows by id into a dense query matrix (the build's queries are the shard's own rows)
// Every order is the total order (distance, node): a key is make_key(d, node, ascending) (common.h), so which array slot an entry
// sits in never matters — pops, evictions and the final sort are decided by the keys alone.  The two comparisons on the distance alone
// (c.dist > worst.dist, d < worst.dist) are taken on the high words of the keys, the order-preserving images of the distances: the same
// predicate (no NaN, -0 == +0 by make_key), and the form hipcc 7.2 builds — comparing the decoded floats crashed its instruction selection.
#pragma once

#include "kernels.h"

namespace lynse {

constexpr uint32_t HNSW_PAD = 0xffffffffu;

// the graph distance: compute_distance_f32 in the single-row form, negated for IP (hnsw.rs:536-543); NaN -> +inf at once
__device__ __forceinline__ float hnsw_dist(int metric, const float* q, const float* __restrict__ v, uint32_t D, int g) {
    float s = exact_score<32>(metric, LYNSE_IPFORM_SINGLE, q, v, D, g);
    if (metric == M_IP) s = -s;
    return s != s ? LY_INF : s;
}

__device__ __forceinline__ uint32_t hnsw_rank(uint64_t mask, int lane) { return (uint32_t)__popcll(mask & ((1ull << lane) - 1ull)); }

// lane l's value as a wave-uniform (scalar) one: l must be uniform.  The admission loops branch on these, so their control flow is scalar.
__device__ __forceinline__ float hnsw_lane(float v, uint32_t l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), (int)l)); }
__device__ __forceinline__ uint32_t hnsw_lane(uint32_t v, uint32_t l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)l); }
__device__ __forceinline__ uint64_t hnsw_uniform(uint64_t v) {
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
}

// The slot of the largest key of R (keys are distinct: one per node).  Out of line, like hnsw_compact: the admission loop stays small.
__device__ __noinline__ uint32_t hnsw_argmax(const uint64_t* Rk, uint32_t Rn, int lane) {
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
__device__ __noinline__ uint32_t hnsw_compact(uint64_t* Ck, uint32_t Cn, uint32_t wd, int lane) {
    uint32_t w = 0;
    for (uint32_t base = 0; base < Cn; base += 64) {
        const uint32_t i = base + lane;
        const uint64_t kx = i < Cn ? Ck[i] : 0ull;
        const bool keep = i < Cn && (uint32_t)(kx >> 32) <= wd;
        const uint64_t km = __ballot(keep);
        __syncthreads();
        if (keep) Ck[w + hnsw_rank(km, lane)] = kx;
        w += (uint32_t)__popcll(km);
        __syncthreads();
    }
    return w;
}

struct HnswSearchArgs {
    const float* V;              // the handle's rows
    uint32_t ld, D;
    int metric;
    const float* Q;              // [nq][D]
    uint32_t k, ef, m;           // ef = min(max(ef, k), n): R never fills beyond the graph
    uint32_t entry, top_level;
    const uint32_t* adj0;        // [n][2 m], HNSW_PAD after the last neighbour, no neighbour twice
    const uint32_t* upper_off;   // [n]: index of the node's level-1 list in upper_adj (its level-l list follows at + l - 1)
    const uint32_t* upper_adj;   // [n_upper][m]
    uint32_t* vis;               // [nq][vis_words] visited bits, zero on entry
    uint32_t vis_words;
    uint64_t* out_rows;          // [nq][k]
    float* out_dists;
    uint32_t* out_counts;        // [nq]
    uint32_t* out_scored;        // [nq] distances scored
    uint32_t* status;            // 1: C outgrew its 2 ef + 8 slots (the bound of DESIGN §19 failed: a bug, reported as one)
};

__global__ void __launch_bounds__(64) k_hnsw_search(HnswSearchArgs a) {
    extern __shared__ __align__(16) unsigned char hnsw_smem[];
    uint64_t* Rk = reinterpret_cast<uint64_t*>(hnsw_smem);   // ef result keys, unordered
    uint64_t* Ck = Rk + a.ef;                                // 2 ef + 8 candidate keys, unordered
    uint32_t* lst = reinterpret_cast<uint32_t*>(Ck + 2 * (size_t)a.ef + 8);   // the unvisited neighbours of one expansion, stored order
    float* qv = reinterpret_cast<float*>(lst + 64);
    const int lane = threadIdx.x, g = lane & 7, grp = lane >> 3;
    const uint32_t q = blockIdx.x;
    for (uint32_t i = lane; i < a.D; i += 64) qv[i] = a.Q[(size_t)q * a.D + i];
    __syncthreads();
    uint32_t* vis = a.vis + (size_t)q * a.vis_words;

    // greedy descent (greedy_closest, hnsw.rs:758-777): a pass scans the list of the node it started from
    uint32_t cur = a.entry, scored = 1;
    float cd = hnsw_dist(a.metric, qv, a.V + (size_t)cur * a.ld, a.D, g);
    for (uint32_t lvl = a.top_level; lvl >= 1; --lvl) {
        for (;;) {
            const uint32_t* list = a.upper_adj + ((size_t)a.upper_off[cur] + (lvl - 1)) * a.m;
            const uint32_t nb = (uint32_t)lane < a.m ? list[lane] : HNSW_PAD;
            const uint32_t deg = (uint32_t)__popcll(__ballot(nb != HNSW_PAD));
            bool changed = false;
            for (uint32_t b = 0; b < deg; b += 8) {
                const uint32_t idx = b + grp;
                const uint32_t node = __shfl(nb, (int)(idx < deg ? idx : b));
                const float d = hnsw_dist(a.metric, qv, a.V + (size_t)node * a.ld, a.D, g);
                const uint32_t cnt = deg - b < 8u ? deg - b : 8u;
                for (uint32_t t = 0; t < cnt; ++t) {
                    const float dt = hnsw_lane(d, t * 8);
                    const uint32_t nt = hnsw_lane(node, t * 8);
                    if (dt < cd) { cd = dt; cur = nt; changed = true; }
                }
                scored += cnt;
            }
            if (!changed) break;
        }
    }

    // the beam at level 0
    const uint32_t ef = a.ef, c_cap = 2 * a.ef + 8;
    uint32_t Rn = 1, Cn = 1, worst_pos = 0;
    uint64_t worst = make_key(cd, cur, true);
    if (lane == 0) {
        Rk[0] = worst;
        Ck[0] = worst;
        vis[cur >> 5] = 1u << (cur & 31u);   // (the bitmap is zero on entry and this wave's alone)
    }
    __syncthreads();
    bool broken = false;
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
        best = hnsw_uniform(best);
        bpos = (uint32_t)__builtin_amdgcn_readfirstlane((int)bpos);
        __syncthreads();
        if (lane == 0) Ck[bpos] = Ck[Cn - 1];
        --Cn;
        __syncthreads();
        if (Rn >= ef && (uint32_t)(best >> 32) > (uint32_t)(worst >> 32)) break;   // c.dist > worst.dist, on the order-preserving images
        const uint32_t c = key_row(best);
        // its unvisited neighbours, in stored order
        const uint32_t nb = (uint32_t)lane < 2 * a.m ? a.adj0[(size_t)c * 2 * a.m + lane] : HNSW_PAD;
        bool fresh = false;
        if (nb != HNSW_PAD) fresh = ((atomicOr(&vis[nb >> 5], 1u << (nb & 31u)) >> (nb & 31u)) & 1u) == 0u;
        const uint64_t um = __ballot(fresh);
        const uint32_t cnt = (uint32_t)__popcll(um);
        if (fresh) lst[hnsw_rank(um, lane)] = nb;
        __syncthreads();
        scored += cnt;
        for (uint32_t b = 0; b < cnt && !broken; b += 8) {
            // Room for the 8 admissions of this step.  C only nears its 2 ef + 8 slots while R is full; worst.dist never rises then, so an
            // entry beyond it can only ever end the search when it is popped — dropping it ends the search the same way (C runs empty).
            // What stays is in R or ties with worst.dist: fewer than 2 ef entries.
            if (Cn + 8 > c_cap) {
                Cn = hnsw_compact(Ck, Cn, (uint32_t)(worst >> 32), lane);
                if (Cn + 8 > c_cap) {
                    if (lane == 0) *a.status = 1u;
                    broken = true;
                }
            }
            if (!broken) {
                const uint32_t idx = b + grp;
                const uint32_t node = lst[idx < cnt ? idx : b];
                const float d = hnsw_dist(a.metric, qv, a.V + (size_t)node * a.ld, a.D, g);
                const uint32_t nbt = cnt - b < 8u ? cnt - b : 8u;
                for (uint32_t t = 0; t < nbt; ++t) {
                    const float dt = hnsw_lane(d, t * 8);
                    const uint32_t nt = hnsw_lane(node, t * 8);
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
                        worst_pos = hnsw_argmax(Rk, Rn, lane);
                        worst = hnsw_uniform(Rk[worst_pos]);
                    }
                }
            }
        }
    }
    __syncthreads();

    // the best min(k, |R|) of R by (dist, node); IP distances un-negated (0 - d: exact, and -0 -> +0 like the key)
    const uint32_t n_out = broken ? 0u : (a.k < Rn ? a.k : Rn);
    if (!broken) {
        for (uint32_t i = lane; i < Rn; i += 64) {
            const uint64_t kx = Rk[i];
            uint32_t rank = 0;
            for (uint32_t j = 0; j < Rn; ++j) rank += Rk[j] < kx ? 1u : 0u;
            if (rank < a.k) {
                const float d = key_score(kx, true);
                a.out_rows[(size_t)q * a.k + rank] = key_row(kx);
                a.out_dists[(size_t)q * a.k + rank] = a.metric == M_IP ? 0.0f - d : d;
            }
        }
    }
    for (uint32_t i = n_out + lane; i < a.k; i += 64) {
        a.out_rows[(size_t)q * a.k + i] = ~0ull;
        a.out_dists[(size_t)q * a.k + i] = a.metric == M_IP ? -LY_INF : LY_INF;
    }
    if (lane == 0) {
        a.out_counts[q] = n_out;
        a.out_scored[q] = scored;
    }
}

// select_neighbors_heuristic for item t = one (node, level).  Its candidates, nearest first by (d, node), come either from an exact
// search of the handle (rows64 / d64 / cnt64: `stride` entries asked for, raw metric values, the node itself still among them — it is
// removed, and the last entry dropped instead when it did not come back) or as CSR lists of graph distances (ids32 / d32 / offs).
struct HnswSelectArgs {
    const float* V;
    uint32_t ld, D;
    int metric;
    uint32_t cap;                  // m0 at level 0, m above
    const uint32_t* item_node;     // the node of item t (dense lists only)
    const uint64_t* rows64;
    const float* d64;
    const uint32_t* cnt64;
    uint32_t stride;
    const uint32_t* ids32;
    const float* d32;
    const uint64_t* offs;          // [items + 1]
    uint32_t* out_ids;             // [items][cap] in selection order, HNSW_PAD after the last
    float* out_d;                  // the graph distances d(node, out_ids)
};

__global__ void __launch_bounds__(64) k_hnsw_select(HnswSelectArgs a) {
    extern __shared__ __align__(16) unsigned char hnsw_smem[];
    uint32_t* kept_id = reinterpret_cast<uint32_t*>(hnsw_smem);   // 64
    float* kept_d = reinterpret_cast<float*>(kept_id + 64);       // 64
    float* cvec = kept_d + 64;                                    // D
    const int lane = threadIdx.x, g = lane & 7, grp = lane >> 3;
    const uint32_t t = blockIdx.x, cap = a.cap;
    const bool dense = a.rows64 != nullptr;
    uint32_t ec, self_pos = 0xffffffffu;
    size_t base;
    if (dense) {
        base = (size_t)t * a.stride;
        const uint32_t cnt = a.cnt64[t] < a.stride ? a.cnt64[t] : a.stride, self = a.item_node[t];
        for (uint32_t p0 = 0; p0 < cnt; p0 += 64) {
            const uint32_t p = p0 + lane;
            const uint64_t hit = __ballot(p < cnt && a.rows64[base + p] == (uint64_t)self);
            if (hit) { self_pos = p0 + (uint32_t)__builtin_ctzll(hit); break; }
        }
        ec = self_pos != 0xffffffffu ? cnt - 1 : (cnt < a.stride - 1 ? cnt : a.stride - 1);
    } else {
        base = (size_t)a.offs[t];
        ec = (uint32_t)(a.offs[t + 1] - a.offs[t]);
    }
    auto cand_id = [&](uint32_t p) -> uint32_t { return dense ? (uint32_t)a.rows64[base + (p < self_pos ? p : p + 1)] : a.ids32[base + p]; };
    auto cand_d = [&](uint32_t p) -> float {
        if (!dense) return a.d32[base + p];
        float s = a.d64[base + (p < self_pos ? p : p + 1)];
        if (a.metric == M_IP) s = -s;
        return s != s ? LY_INF : s;
    };
    uint32_t* out_ids = a.out_ids + (size_t)t * cap;
    float* out_d = a.out_d + (size_t)t * cap;
    if (ec <= cap) {   // no more than cap: all of them, as they come
        if ((uint32_t)lane < cap) {
            out_ids[lane] = (uint32_t)lane < ec ? cand_id(lane) : HNSW_PAD;
            out_d[lane] = (uint32_t)lane < ec ? cand_d(lane) : LY_INF;
        }
        return;
    }
    uint32_t kept = 0;
    for (uint32_t p = 0; p < ec && kept < cap; ++p) {
        const uint32_t c = cand_id(p);
        const float dc = cand_d(p);
        __syncthreads();
        for (uint32_t i = lane; i < a.D; i += 64) cvec[i] = a.V[(size_t)c * a.ld + i];
        __syncthreads();
        bool reject = false;
        for (uint32_t b = 0; b < kept && !reject; b += 8) {
            const uint32_t idx = b + grp;
            const uint32_t s = kept_id[idx < kept ? idx : b];
            const float dcs = hnsw_dist(a.metric, cvec, a.V + (size_t)s * a.ld, a.D, g);
            reject = __any(idx < kept && dcs < dc) != 0;   // some kept s is closer to c than the node is
        }
        if (!reject) {
            if (lane == 0) { kept_id[kept] = c; kept_d[kept] = dc; }
            ++kept;
        }
    }
    __syncthreads();
    const uint32_t kept0 = kept;   // free slots go to the nearest candidates the walk did not keep
    for (uint32_t p0 = 0; p0 < ec && kept < cap; p0 += 64) {
        const uint32_t p = p0 + lane;
        const uint32_t c = p < ec ? cand_id(p) : HNSW_PAD;
        bool left = p < ec;
        for (uint32_t j = 0; j < kept0 && left; ++j) left = kept_id[j] != c;
        const uint64_t lm = __ballot(left);
        const uint32_t slot = kept + hnsw_rank(lm, lane);
        if (left && slot < cap) { kept_id[slot] = c; kept_d[slot] = cand_d(p); }
        kept += (uint32_t)__popcll(lm);
        if (kept > cap) kept = cap;
        __syncthreads();
    }
    if ((uint32_t)lane < cap) {
        out_ids[lane] = (uint32_t)lane < kept ? kept_id[lane] : HNSW_PAD;
        out_d[lane] = (uint32_t)lane < kept ? kept_d[lane] : LY_INF;
    }
}

// out[t][0..D) = V[ids ? ids[t] : first + t][0..D)
__global__ void __launch_bounds__(256) k_hnsw_gather(const float* __restrict__ V, uint32_t ld, uint32_t D, const uint32_t* __restrict__ ids,
                                                     uint32_t first, uint64_t n, float* __restrict__ out) {
    const uint64_t total = n * D;
    for (uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (uint64_t)gridDim.x * 256) {
        const uint64_t t = e / D;
        const uint32_t d = (uint32_t)(e % D);
        const uint32_t r = ids ? ids[t] : first + (uint32_t)t;
        out[e] = V[(size_t)r * ld + d];
    }
}

}  // namespace lynse
