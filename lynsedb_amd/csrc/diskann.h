// diskann.h — DISKANN-{L2,COS} on a FLAT handle (DiskANNIndex, src/index/diskann.rs, the in-memory full-precision form): the batched
// Vamana build and the beam search.  include/lynse_hip.h states the contract (the DiskANN rule block), DESIGN.md §21 the reasoning.
//   k_vamana_search   one wave per query: the start phase (the entry and the evenly spaced anchors), then the two-heap beam
//                     (graph_beam, graph.h) over lists of r.  Two outputs: the top k (queries) or the whole of R as keys (the build).
//   k_vamana_prune    one wave per item: robust_prune.  Forward form: the beam of a batch member plus its current list, the result is
//                     installed as its new list.  Commit form: an over-long destination list, scored first.
//   k_vamana_commit   one block per batch: the effective reverse edges of the batch as keys (dst, degree, edge), sorted in LDS; the
//                     append slot of an edge is its place in the run of its dst — no atomic, no arrival order.
//   k_vamana_pairs    d(candidate, ref) for the entry-point sums of rule 2
// The distance, the wave helpers, the beam and the LDS layout of the search (GraphSearchLds) are graph.h's, shared with hnsw.h.
#pragma once

#include "graph.h"

namespace lynse {

constexpr uint32_t VAMANA_BATCH = 256, VAMANA_STARTS = 33;   // a build batch; the entry + at most 32 anchors

// the slots of C; the host sizes the kernel's LDS with the same count
__host__ __device__ constexpr uint32_t vamana_c_cap(uint32_t ef) { return 2 * ef + 8 + VAMANA_STARTS; }
static_assert(GraphSearchLds::bytes(1, vamana_c_cap(1), 2) == 1 * 24 + (8 + 33) * 8 + 256 + 2 * 4 &&
              GraphSearchLds::bytes(4096, vamana_c_cap(4096), 768) == (size_t)4096 * 24 + (8 + 33) * 8 + 256 + 768 * 4,
              "R: ef keys, C: 2 ef + 8 + 33 keys, 64 node slots, the query");

struct VamanaSearchArgs {
    const float* V;              // the handle's rows
    uint32_t ld, D;
    int metric;
    const float* Q;              // [nq][D]; NULL: query q is row qids[q] (the build)
    const uint32_t* qids;
    uint32_t k, ef, r, anchors;  // anchors <= 32
    uint32_t entry;
    uint64_t n;
    const uint32_t* adj;         // [n][r], GRAPH_PAD after the last neighbour, no neighbour twice
    uint32_t* vis;               // [nq][vis_words] visited bits, zero on entry
    uint32_t vis_words;
    uint64_t* out_rows;          // [nq][k]; NULL in the build
    float* out_dists;
    uint32_t* out_counts;        // [nq]
    uint64_t* out_beam;          // [nq][ef]: R as keys, ascending (the build); NULL for queries
    uint32_t* out_beam_n;        // [nq]
    uint32_t* out_scored;        // [nq] distances scored
    uint32_t* status;            // 1: C outgrew its 2 ef + 8 + 33 slots (the bound of DESIGN §21 failed: a bug, reported as one)
};

__global__ void __launch_bounds__(64) k_vamana_search(VamanaSearchArgs a) {
    extern __shared__ __align__(16) unsigned char vam_smem[];
    const uint32_t ef = a.ef, c_cap = vamana_c_cap(a.ef);
    const GraphSearchLds lds(vam_smem, ef, c_cap);
    uint64_t* Rk = lds.Rk;
    uint64_t* Ck = lds.Ck;
    uint32_t* lst = lds.lst;   // the starts first
    float* qv = lds.qv;
    const int lane = threadIdx.x, g = lane & 7, grp = lane >> 3;
    const uint32_t q = blockIdx.x;
    const float* qsrc = a.Q ? a.Q + (size_t)q * a.D : a.V + (size_t)a.qids[q] * a.ld;
    for (uint32_t i = lane; i < a.D; i += 64) qv[i] = qsrc[i];
    uint32_t* vis = a.vis + (size_t)q * a.vis_words;

    // the starts (search_entry_points): the entry, then a n / A for a = 0 .. A - 1 unless it is the entry; all distinct
    const uint32_t A = (uint32_t)(a.n < a.anchors ? a.n : a.anchors);
    uint32_t snode = GRAPH_PAD;
    if (lane == 0) snode = a.entry;
    else if ((uint32_t)lane <= A) {
        const uint32_t idx = (uint32_t)((uint64_t)(lane - 1) * a.n / A);
        if (idx != a.entry) snode = idx;
    }
    const uint64_t sm = __ballot(snode != GRAPH_PAD);
    const uint32_t ns = (uint32_t)__popcll(sm);
    if (snode != GRAPH_PAD) {
        lst[graph_rank(sm, lane)] = snode;
        atomicOr(&vis[snode >> 5], 1u << (snode & 31u));
    }
    __syncthreads();
    for (uint32_t b = 0; b < ns; b += 8) {   // every start is scored and pushed to C
        const uint32_t idx = b + grp;
        const uint32_t node = lst[idx < ns ? idx : b];
        const float d = graph_dist(a.metric, qv, a.V + (size_t)node * a.ld, a.D, g);
        if (g == 0 && idx < ns) Ck[idx] = make_key(d, node, true);
    }
    __syncthreads();
    // R = the best ef of the starts by (d, node), no admission test; ef may be below the number of starts
    if ((uint32_t)lane < ns) {
        const uint64_t kx = Ck[lane];
        uint32_t rank = 0;
        for (uint32_t j = 0; j < ns; ++j) rank += Ck[j] < kx ? 1u : 0u;
        if (rank < ef) Rk[rank] = kx;
    }
    __syncthreads();
    const uint32_t Rn0 = ns < ef ? ns : ef;
    GraphBeamState bs{Rn0, ns, Rn0 - 1, graph_uniform(Rk[Rn0 - 1]), ns, false};
    graph_beam(a.V, a.ld, a.D, a.metric, a.adj, a.r, lds, ef, c_cap, vis, a.status, bs);

    // R by (dist, node): the best min(k, |R|) for a query, all of it for the build
    const uint32_t want = a.out_beam ? ef : a.k;
    const uint32_t n_out = bs.broken ? 0u : (want < bs.Rn ? want : bs.Rn);
    if (!bs.broken) {
        auto beam_key = [&](uint32_t rank, uint64_t kx) { a.out_beam[(size_t)q * ef + rank] = kx; };
        auto row_and_dist = [&](uint32_t rank, uint64_t kx) {
            a.out_rows[(size_t)q * a.k + rank] = key_row(kx);
            a.out_dists[(size_t)q * a.k + rank] = key_score(kx, true);
        };
        // (one rank sort in the kernel's code, the form chosen per entry)
        graph_emit_ranked(Rk, bs.Rn, want, [&](uint32_t rank, uint64_t kx) { a.out_beam ? beam_key(rank, kx) : row_and_dist(rank, kx); });
    }
    if (!a.out_beam) {
        for (uint32_t i = n_out + lane; i < a.k; i += 64) {
            a.out_rows[(size_t)q * a.k + i] = ~0ull;
            a.out_dists[(size_t)q * a.k + i] = LY_INF;
        }
    }
    if (lane == 0) {
        if (a.out_beam) a.out_beam_n[q] = n_out;
        else a.out_counts[q] = n_out;
        a.out_scored[q] = bs.scored;
    }
}

// A commit key: the destination, its degree after the installs, the edge number s r + j of the batch (s: the slot of the source).
__host__ __device__ inline uint64_t vamana_ckey(uint32_t dst, uint32_t deg, uint32_t e) { return ((uint64_t)dst << 32) | ((uint64_t)deg << 24) | e; }
__host__ __device__ inline uint32_t vamana_ckey_deg(uint64_t k) { return (uint32_t)(k >> 24) & 0xffu; }
__host__ __device__ inline uint32_t vamana_ckey_edge(uint64_t k) { return (uint32_t)k & 0xffffffu; }

struct VamanaPruneArgs {
    const float* V;
    uint32_t ld, D;
    int metric;
    uint32_t r, cap;             // cap: key slots of one LDS array (>= the longest candidate list)
    float alpha;
    uint32_t* adj;               // [n][r]: the list of the item's node is read, then replaced
    const uint32_t* items;       // [B] the nodes of the batch, in batch order
    const uint64_t* beam;        // forward form: [B][beam_stride] keys of d(p, .) and beam_n[B]
    const uint32_t* beam_n;
    uint32_t beam_stride;
    const uint64_t* ckeys;       // commit form (not NULL): the sorted commit keys, n_ckeys of them, KEY_SENTINEL after the last
    uint32_t n_ckeys;
};

__global__ void __launch_bounds__(64) k_vamana_prune(VamanaPruneArgs a) {
    extern __shared__ __align__(16) unsigned char vam_smem[];
    uint64_t* K0 = reinterpret_cast<uint64_t*>(vam_smem);
    uint64_t* K1 = K0 + a.cap;
    float* pvec = reinterpret_cast<float*>(K1 + a.cap);
    float* bvec = pvec + a.D;
    uint32_t* raw = reinterpret_cast<uint32_t*>(K1);   // nodes still to be scored against p
    const int lane = threadIdx.x, g = lane & 7, grp = lane >> 3;
    const uint32_t t = blockIdx.x, r = a.r;
    uint32_t p, m = 0, nraw;
    if (!a.ckeys) {
        p = a.items[t];
        const uint32_t bn = a.beam_n[t];
        for (uint32_t i = lane; i < bn; i += 64) K0[i] = a.beam[(size_t)t * a.beam_stride + i];
        m = bn;
        const uint32_t nb = (uint32_t)lane < r ? a.adj[(size_t)p * r + lane] : GRAPH_PAD;
        const uint64_t nm = __ballot(nb != GRAPH_PAD);
        if (nb != GRAPH_PAD) raw[graph_rank(nm, lane)] = nb;
        nraw = (uint32_t)__popcll(nm);
    } else {
        // the grid covers every key slot; a wave works only at the head of the run of a destination whose list outgrew r
        const uint64_t key = a.ckeys[t];
        if (key == KEY_SENTINEL) return;
        p = (uint32_t)(key >> 32);
        if (t > 0 && (uint32_t)(a.ckeys[t - 1] >> 32) == p) return;
        const uint32_t deg = vamana_ckey_deg(key);
        uint32_t run = 0;
        for (uint32_t base = t;; base += 64) {
            const uint32_t i = base + lane;
            const bool same = i < a.n_ckeys && (uint32_t)(a.ckeys[i] >> 32) == p;
            const uint64_t sm = __ballot(same);
            const uint32_t c = sm == ~0ull ? 64u : (uint32_t)__builtin_ctzll(~sm);
            run += c;
            if (c < 64) break;
        }
        if (deg + run <= r) return;
        if ((uint32_t)lane < deg) raw[lane] = a.adj[(size_t)p * r + lane];
        for (uint32_t i = lane; i < run; i += 64) raw[deg + i] = a.items[vamana_ckey_edge(a.ckeys[t + i]) / r];
        nraw = deg + run;
    }
    for (uint32_t i = lane; i < a.D; i += 64) pvec[i] = a.V[(size_t)p * a.ld + i];
    __syncthreads();
    for (uint32_t b = 0; b < nraw; b += 8) {
        const uint32_t idx = b + grp;
        const uint32_t node = raw[idx < nraw ? idx : b];
        const float d = graph_dist(a.metric, pvec, a.V + (size_t)node * a.ld, a.D, g);
        if (g == 0 && idx < nraw) K0[m + idx] = make_key(d, node, true);
    }
    m += nraw;
    __syncthreads();
    // drop p, keep one entry per node (equal nodes carry equal keys), order by (d, node): a rank count over the keys
    for (uint32_t i = lane; i < m; i += 64) {
        const uint64_t kx = K0[i];
        bool dead = key_row(kx) == p;
        for (uint32_t j = 0; j < i && !dead; ++j) dead = K0[j] == kx;
        K1[i] = dead ? KEY_SENTINEL : kx;
    }
    __syncthreads();
    uint32_t cnt = 0;
    for (uint32_t i0 = 0; i0 < m; i0 += 64) {
        const uint32_t i = i0 + lane;
        const uint64_t kx = i < m ? K1[i] : KEY_SENTINEL;
        if (kx != KEY_SENTINEL) {
            uint32_t rank = 0;
            for (uint32_t j = 0; j < m; ++j) rank += K1[j] < kx ? 1u : 0u;
            K0[rank] = kx;
        }
        cnt += (uint32_t)__popcll(__ballot(kx != KEY_SENTINEL));
    }
    __syncthreads();
    // the walk: select the first remaining b, keep v iff alpha d(b, v) > d(p, v) (one f32 multiply, then the comparison)
    uint32_t sel = 0, my_id = GRAPH_PAD;
    while (cnt && sel < r) {
        const uint32_t bnode = key_row(graph_uniform(K0[0]));
        if ((uint32_t)lane == sel) my_id = bnode;
        ++sel;
        if (sel == r) break;
        __syncthreads();
        for (uint32_t i = lane; i < a.D; i += 64) bvec[i] = a.V[(size_t)bnode * a.ld + i];
        __syncthreads();
        uint32_t w = 0;
        for (uint32_t i0 = 1; i0 < cnt; i0 += 8) {
            const uint32_t idx = i0 + grp;
            const bool valid = idx < cnt;
            const uint64_t kx = K0[valid ? idx : i0];
            const float d = graph_dist(a.metric, bvec, a.V + (size_t)key_row(kx) * a.ld, a.D, g);
            const bool keep = valid && g == 0 && __fmul_rn(a.alpha, d) > key_score(kx, true);
            const uint64_t km = __ballot(keep);
            __syncthreads();
            if (keep) K0[w + graph_rank(km, lane)] = kx;
            w += (uint32_t)__popcll(km);
            __syncthreads();
        }
        cnt = w;
    }
    if ((uint32_t)lane < r) a.adj[(size_t)p * r + lane] = my_id;
}

// Rule 7 for one batch whose forward lists are installed.  An edge (src = items[s], dst = adj[src][j]) is effective when dst does not
// name src.  Its key sorts by (dst, s): the run of a dst lists its new sources in batch order, so an edge's append slot is its place in
// the run.  Lists that stay within r are appended here; the others are left to k_vamana_prune, which reads the sorted keys.
struct VamanaCommitArgs {
    uint32_t* adj;
    uint32_t r, B, P;            // P: the power of two >= max(B r, 2) keys sorted
    const uint32_t* items;
    uint64_t* ckeys;             // [P] out
};

__global__ void __launch_bounds__(1024) k_vamana_commit(VamanaCommitArgs a) {
    extern __shared__ __align__(16) unsigned char vam_smem[];
    uint64_t* K = reinterpret_cast<uint64_t*>(vam_smem);
    const uint32_t tid = threadIdx.x, r = a.r, E = a.B * r, P = a.P;
    for (uint32_t e = tid; e < P; e += 1024) {
        uint64_t key = KEY_SENTINEL;
        if (e < E) {
            const uint32_t src = a.items[e / r], dst = a.adj[(size_t)src * r + e % r];
            if (dst != GRAPH_PAD && dst != src) {
                bool found = false;
                uint32_t deg = 0;
                for (; deg < r; ++deg) {
                    const uint32_t x = a.adj[(size_t)dst * r + deg];
                    if (x == GRAPH_PAD) break;
                    found |= x == src;
                }
                if (!found) key = vamana_ckey(dst, deg, e);
            }
        }
        K[e] = key;
    }
    __syncthreads();   // (every read of adj above precedes every append below: one block)
    for (uint32_t k = 2; k <= P; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t i = tid; i < P; i += 1024) {
                const uint32_t x = i ^ j;
                if (x > i) {
                    const uint64_t u = K[i], v = K[x];
                    if ((u > v) == ((i & k) == 0)) { K[i] = v; K[x] = u; }
                }
            }
            __syncthreads();
        }
    }
    for (uint32_t i = tid; i < P; i += 1024) {
        const uint64_t key = K[i];
        a.ckeys[i] = key;
        if (key == KEY_SENTINEL) continue;
        const uint32_t dst = (uint32_t)(key >> 32), deg = vamana_ckey_deg(key);
        auto first_at_least = [&](uint64_t v) {   // the first index whose key is >= v
            uint32_t lo = 0, hi = P;
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (K[mid] < v) lo = mid + 1; else hi = mid;
            }
            return lo;
        };
        const uint32_t lo = first_at_least((uint64_t)dst << 32), hi = first_at_least(((uint64_t)dst + 1) << 32);
        if (deg + (hi - lo) <= r) a.adj[(size_t)dst * r + deg + (i - lo)] = a.items[vamana_ckey_edge(key) / r];
    }
}

// out[c][j] = d(cands[c], refs[j]): one block per candidate
__global__ void __launch_bounds__(64) k_vamana_pairs(const float* __restrict__ V, uint32_t ld, uint32_t D, int metric, const uint32_t* __restrict__ cands,
                                                     const uint32_t* __restrict__ refs, uint32_t nr, float* __restrict__ out) {
    extern __shared__ __align__(16) unsigned char vam_smem[];
    float* cvec = reinterpret_cast<float*>(vam_smem);
    const int lane = threadIdx.x, g = lane & 7, grp = lane >> 3;
    const uint32_t c = blockIdx.x;
    for (uint32_t i = lane; i < D; i += 64) cvec[i] = V[(size_t)cands[c] * ld + i];
    __syncthreads();
    for (uint32_t b = 0; b < nr; b += 8) {
        const uint32_t idx = b + grp;
        const uint32_t node = refs[idx < nr ? idx : b];
        const float d = graph_dist(metric, cvec, V + (size_t)node * ld, D, g);
        if (g == 0 && idx < nr) out[(size_t)c * nr + idx] = d;
    }
}

}  // namespace lynse
