// hnsw.h — HNSW-{IP,L2,COS} on a FLAT handle (HNSWIndex, src/index/hnsw.rs): the graph beam search and the neighbour-selection
// heuristic of the bulk build.  include/lynse_hip.h states the contract (the HNSW rule block), DESIGN.md §19 the reasoning.
//   k_hnsw_search   one wave per query: greedy descent over the upper levels, then the two-heap beam at level 0 (graph_beam, graph.h)
//                   from the node the descent ends at.  The query, R (results) and C (candidates) live in LDS (GraphSearchLds).
//   k_hnsw_select   one wave per (node, level): select_neighbors_heuristic (hnsw.rs:550-602) over a sorted candidate list
//   k_hnsw_gather   rows by id into a dense query matrix (the build's queries are the shard's own rows)
//   k_hnsw_reverse_scan   the incremental insert (rule 7): which old members of a level may see a new row enter their candidate list
// The distance, the wave helpers, the beam and the order of its keys are graph.h's, shared with diskann.h.
#pragma once

#include "graph.h"

namespace lynse {

// the slots of C; the host sizes the kernel's LDS with the same count
__host__ __device__ constexpr uint32_t hnsw_c_cap(uint32_t ef) { return 2 * ef + 8; }
static_assert(GraphSearchLds::bytes(1, hnsw_c_cap(1), 2) == 1 * 24 + 64 + 256 + 2 * 4 &&
              GraphSearchLds::bytes(4096, hnsw_c_cap(4096), 768) == (size_t)4096 * 24 + 64 + 256 + 768 * 4,
              "R: ef keys, C: 2 ef + 8 keys, 64 neighbour slots, the query");

struct HnswSearchArgs {
    const float* V;              // the handle's rows
    uint32_t ld, D;
    int metric;
    const float* Q;              // [nq][D]
    uint32_t k, ef, m;           // ef = min(max(ef, k), n): R never fills beyond the graph
    uint32_t entry, top_level;
    const uint32_t* adj0;        // [n][2 m], GRAPH_PAD after the last neighbour, no neighbour twice
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
    const uint32_t ef = a.ef, c_cap = hnsw_c_cap(a.ef);
    const GraphSearchLds lds(hnsw_smem, ef, c_cap);
    uint64_t* Rk = lds.Rk;
    uint64_t* Ck = lds.Ck;
    float* qv = lds.qv;
    const int lane = threadIdx.x, g = lane & 7, grp = lane >> 3;
    const uint32_t q = blockIdx.x;
    for (uint32_t i = lane; i < a.D; i += 64) qv[i] = a.Q[(size_t)q * a.D + i];
    __syncthreads();
    uint32_t* vis = a.vis + (size_t)q * a.vis_words;

    // greedy descent (greedy_closest, hnsw.rs:758-777): a pass scans the list of the node it started from
    uint32_t cur = a.entry, scored = 1;
    float cd = graph_dist(a.metric, qv, a.V + (size_t)cur * a.ld, a.D, g);
    for (uint32_t lvl = a.top_level; lvl >= 1; --lvl) {
        for (;;) {
            const uint32_t* list = a.upper_adj + ((size_t)a.upper_off[cur] + (lvl - 1)) * a.m;
            const uint32_t nb = (uint32_t)lane < a.m ? list[lane] : GRAPH_PAD;
            const uint32_t deg = (uint32_t)__popcll(__ballot(nb != GRAPH_PAD));
            bool changed = false;
            for (uint32_t b = 0; b < deg; b += 8) {
                const uint32_t idx = b + grp;
                const uint32_t node = __shfl(nb, (int)(idx < deg ? idx : b));
                const float d = graph_dist(a.metric, qv, a.V + (size_t)node * a.ld, a.D, g);
                const uint32_t cnt = deg - b < 8u ? deg - b : 8u;
                for (uint32_t t = 0; t < cnt; ++t) {
                    const float dt = graph_lane(d, t * 8);
                    const uint32_t nt = graph_lane(node, t * 8);
                    if (dt < cd) { cd = dt; cur = nt; changed = true; }
                }
                scored += cnt;
            }
            if (!changed) break;
        }
    }

    // the beam at level 0, from the one entry the descent found
    GraphBeamState bs{1, 1, 0, make_key(cd, cur, true), scored, false};
    if (lane == 0) {
        Rk[0] = bs.worst;
        Ck[0] = bs.worst;
        vis[cur >> 5] = 1u << (cur & 31u);   // (the bitmap is zero on entry and this wave's alone)
    }
    __syncthreads();
    graph_beam(a.V, a.ld, a.D, a.metric, a.adj0, 2 * a.m, lds, ef, c_cap, vis, a.status, bs);

    // the best min(k, |R|) of R by (dist, node); IP distances un-negated (0 - d: exact, and -0 -> +0 like the key)
    const uint32_t n_out = bs.broken ? 0u : (a.k < bs.Rn ? a.k : bs.Rn);
    if (!bs.broken)
        graph_emit_ranked(Rk, bs.Rn, a.k, [&](uint32_t rank, uint64_t kx) {
            const float d = key_score(kx, true);
            a.out_rows[(size_t)q * a.k + rank] = key_row(kx);
            a.out_dists[(size_t)q * a.k + rank] = a.metric == M_IP ? 0.0f - d : d;
        });
    for (uint32_t i = n_out + lane; i < a.k; i += 64) {
        a.out_rows[(size_t)q * a.k + i] = ~0ull;
        a.out_dists[(size_t)q * a.k + i] = a.metric == M_IP ? -LY_INF : LY_INF;
    }
    if (lane == 0) {
        a.out_counts[q] = n_out;
        a.out_scored[q] = bs.scored;
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
    uint32_t* out_ids;             // [items][cap] in selection order, GRAPH_PAD after the last
    float* out_d;                  // the graph distances d(node, out_ids)
    float* out_thr;                // dense lists, may be NULL: the raw score of entry `stride` of the search, NaN when it returned fewer (rule 7)
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
        if (a.out_thr && lane == 0) a.out_thr[t] = cnt == a.stride ? a.d64[base + a.stride - 1] : __int_as_float(0x7fc00000);
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
            out_ids[lane] = (uint32_t)lane < ec ? cand_id(lane) : GRAPH_PAD;
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
            const float dcs = graph_dist(a.metric, cvec, a.V + (size_t)s * a.ld, a.D, g);
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
        const uint32_t c = p < ec ? cand_id(p) : GRAPH_PAD;
        bool left = p < ec;
        for (uint32_t j = 0; j < kept0 && left; ++j) left = kept_id[j] != c;
        const uint64_t lm = __ballot(left);
        const uint32_t slot = kept + graph_rank(lm, lane);
        if (left && slot < cap) { kept_id[slot] = c; kept_d[slot] = cand_d(p); }
        kept += (uint32_t)__popcll(lm);
        if (kept > cap) kept = cap;
        __syncthreads();
    }
    if ((uint32_t)lane < cap) {
        out_ids[lane] = (uint32_t)lane < kept ? kept_id[lane] : GRAPH_PAD;
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

// Rule 7, the reverse scan of one level: old member t (row old_ids[t], or t itself at level 0) is flagged when some new row x of the
// tile scores against it not strictly worse than thr[t], the last entry its exact search returned (NaN: the search came back short,
// so every comparison flags) — ties and NaN scores flag.  The score is exact_score in the single-row form, the bits the candidate
// search ranks by, on the raw metric value (ip: larger is better); the forms are symmetric bit for bit, so the new row may stand in the
// query's place.  A tile of `tn` new rows sits in LDS (the host sizes it from the 160 KiB the graph kernels share); waves stream the
// old members, 8 at a time on the 8 lane groups as graph_beam does, each row against the whole tile while it is hot in the caches.
// A wave whose 8 members are all flagged (by an earlier tile too) moves on.  Control flow is wave-uniform: exact_score shuffles.
struct HnswReverseArgs {
    const float* V;
    uint32_t ld, D;
    int metric;
    const uint32_t* old_ids;     // NULL at level 0: member t is row t
    uint32_t n_old;
    const float* thr;            // [n_old]
    const uint32_t* new_ids;     // the level's new rows; the tile is new_ids[tile0 .. tile0 + tn)
    uint32_t tile0, tn;
    uint8_t* flags;              // [n_old], zero before the first tile
};
constexpr uint32_t HNSW_REVERSE_THREADS = 1024;   // 16 waves: one block holds a CU's LDS, 4 waves per SIMD hide the row loads

__global__ void __launch_bounds__(HNSW_REVERSE_THREADS) k_hnsw_reverse_scan(HnswReverseArgs a) {
    extern __shared__ __align__(16) unsigned char hnsw_smem[];
    float* tile = reinterpret_cast<float*>(hnsw_smem);   // [tn][D]
    const uint32_t tid = threadIdx.x;
    for (uint32_t j = 0; j < a.tn; ++j) {
        const float* src = a.V + (size_t)a.new_ids[a.tile0 + j] * a.ld;
        for (uint32_t e = tid; e < a.D; e += HNSW_REVERSE_THREADS) tile[(size_t)j * a.D + e] = src[e];
    }
    __syncthreads();
    const int lane = tid & 63, g = lane & 7, grp = lane >> 3;
    const uint32_t waves = HNSW_REVERSE_THREADS / 64;
    const uint64_t step = (uint64_t)gridDim.x * waves * 8;
    for (uint64_t base = ((uint64_t)blockIdx.x * waves + (tid >> 6)) * 8; base < a.n_old; base += step) {
        const uint64_t idx = base + grp;
        const bool valid = idx < a.n_old;
        const uint32_t t = (uint32_t)(valid ? idx : base);
        bool flag = a.flags[t] != 0;
        if (__all(flag)) continue;
        const float th = a.thr[t];
        const float* v = a.V + (size_t)(a.old_ids ? a.old_ids[t] : t) * a.ld;
        for (uint32_t j = 0; j < a.tn; ++j) {
            const float s = exact_score<32>(a.metric, LYNSE_IPFORM_SINGLE, tile + (size_t)j * a.D, v, a.D, g);
            const bool worse = a.metric == M_IP ? s < th : s > th;   // false for a tie, a NaN score and a short list
            flag = flag || !worse;
            if (__all(flag)) break;
        }
        if (valid && g == 0 && flag) a.flags[t] = 1;
    }
}

}  // namespace lynse
