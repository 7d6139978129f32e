// spann.h — SPANN-{IP,L2,COS}[-SQ8] kernels (SPANNIndex, src/index/spann.rs).  Included by lynse_hip.hip after ivf.h.
//
// A row sits in up to R + 1 posting lists (R = replica_count).  The lists of a row follow posting_centroids_for_vector
// (spann.rs:130-186): the canonical (rank, centroid) top-keep of the centroids (keep = min(R + 1, nlist); rank = distance, or
// -distance for IP), then the first one plus every later one whose rank is within threshold = p + max(|p|, EPS) * 0.35000002
// of the first rank p.  For finite ranks the top-keep is the exact FLAT search of the row against the centroid store; a row
// that can meet a NaN (or an infinite) rank anywhere follows the sequential insertion rule literally (k_spann_slow).
//
// Search runs the IVF list scan with k' = k (R + 1): a row's replicas carry the same (distance, row) key and sit next to each
// other in the canonical order, so k_spann_unique compacts the first k' keys to the first min(k, distinct) distinct rows.

#pragma once

namespace lynse {

// The factor of the replica threshold: REPLICA_DISTANCE_FACTOR - 1.0 in f32 (spann.rs: 1.35f32 - 1.0 = 0.35000002).
#define SPANN_SLACK (1.35f - 1.0f)
#define SPANN_EPS 1.1920929e-07f   // f32::EPSILON
#define SPANN_MAX_KEEP 64u         // R + 1 <= 64: the slow path keeps its slots in LDS

// ------------------------------------------------------------------------------------------------
// k_spann_flag — rows that must take the sequential rule: any non-finite element, or magnitudes at which a distance to some
// centroid can overflow (an overflowed inner product can sum +inf and -inf to NaN; cosine norms likewise).  One wave per row.
// cmax: the largest |element| of the centroids (host); all_slow != 0 flags every row (non-finite centroids).
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_spann_flag(const float* __restrict__ V, uint32_t ld, uint32_t D, uint64_t n, float cmax,
                                                    int metric, int all_slow, uint8_t* __restrict__ flag) {
    const uint32_t lane = threadIdx.x & 63;
    for (uint64_t r = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < n; r += (uint64_t)gridDim.x * 4) {
        const float* v = V + r * ld;
        float m = 0.0f;
        int bad = 0;
        for (uint32_t d = lane; d < D; d += 64) {
            const float x = v[d];
            bad |= !isfinite(x);
            m = fmaxf(m, fabsf(x));
        }
        for (int o = 32; o > 0; o >>= 1) {
            m = fmaxf(m, __shfl_xor(m, o));
            bad |= __shfl_xor(bad, o);
        }
        if (lane == 0) {
            // |partial sums| <= D * max|v| * max|c| (IP, cosine dot), D * max|v|^2 (cosine norm), D * (max|v| + max|c|)^2 (L2): far below
            // f32::MAX, no partial sum can be infinite and no NaN can form
            const double mv = m, mc = cmax, lim = 1e37 / (double)(D ? D : 1);
            bool risky = metric == M_L2 ? (mv + mc) * (mv + mc) > lim : (mv * mc > lim || mv * mv > lim || mc * mc > lim);
            flag[r] = (all_slow || bad || risky) ? 1 : 0;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// k_spann_postings — the lists of each row from its canonical top-keep (ids / distances / count from the FLAT search of the
// rows against the centroid store, `keep` per row).  One thread per row: lists[r * keep + j], cnt[r].  A flagged row, a short
// top-keep or a non-finite distance goes to the slow list instead (k_spann_slow answers it).
// ------------------------------------------------------------------------------------------------
struct SpannPostArgs {
    const uint64_t* top_c;   // [n][keep] centroid ids
    const float* top_d;      // [n][keep] distances
    const uint32_t* top_cnt; // [n]
    const uint8_t* flag;     // [n] (k_spann_flag), indexed by row0 + r
    uint64_t n, row0;        // rows of this batch, the first one's row id
    uint32_t keep, R;
    int metric;
    uint32_t* lists;         // [rows][keep], indexed by row0 + r
    uint32_t* cnt;           // [rows]
    uint32_t* slow;          // the slow rows (row ids) ...
    uint32_t* n_slow;        // ... and their count
};

__global__ void __launch_bounds__(256) k_spann_postings(SpannPostArgs a) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= a.n) return;
    const uint64_t row = a.row0 + r;
    const bool asc = metric_ascending(a.metric);
    bool slow = a.flag[row] != 0 || a.top_cnt[r] < a.keep;
    for (uint32_t j = 0; j < a.keep && !slow; ++j) slow = !isfinite(a.top_d[r * a.keep + j]);
    if (slow) {
        a.slow[atomicAdd(a.n_slow, 1u)] = (uint32_t)row;
        a.cnt[row] = 0;
        return;
    }
    uint32_t* out = a.lists + row * a.keep;
    const float p = asc ? a.top_d[r * a.keep] : -a.top_d[r * a.keep];
    out[0] = (uint32_t)a.top_c[r * a.keep];
    uint32_t len = 1;
    if (a.R > 0) {
        const float slack = __fmul_rn(fmaxf(fabsf(p), SPANN_EPS), SPANN_SLACK);
        const float threshold = __fadd_rn(p, slack);
        for (uint32_t j = 1; j < a.keep; ++j) {
            const float d = a.top_d[r * a.keep + j];
            const float rank = asc ? d : -d;
            if (len <= a.R && rank <= threshold) out[len++] = (uint32_t)a.top_c[r * a.keep + j];
        }
    }
    a.cnt[row] = len;
}

// ------------------------------------------------------------------------------------------------
// k_spann_slow — posting_centroids_for_vector literally for the flagged rows: every centroid's rank (compute_distance_f32, the
// single-row kernels) into LDS, then the insertion of c = 0 .. nlist - 1 into keep slots in order (a NaN rank never satisfies
// rank >= last, so it lands in the last slot; a NaN there lets anything displace it), then the threshold rule.  One workgroup
// per row; dynamic LDS = nlist floats + 2 keep words.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_spann_slow(const float* __restrict__ V, uint32_t ld, const float* __restrict__ C, uint32_t ldc,
                                                    uint32_t D, uint32_t nlist, uint32_t keep, uint32_t R, int metric,
                                                    const uint32_t* __restrict__ slow, uint32_t* __restrict__ lists, uint32_t* __restrict__ cnt) {
    extern __shared__ float s_rank[];
    float* s_best = s_rank + nlist;
    uint32_t* s_bc = reinterpret_cast<uint32_t*>(s_best + keep);
    const uint32_t row = slow[blockIdx.x];
    const float* v = V + (uint64_t)row * ld;
    const bool asc = metric_ascending(metric);
    const int g = threadIdx.x & 7;
    const uint32_t bound = (nlist + 31u) / 32u * 32u;   // whole 8-lane groups run the same trip count (exact_score shuffles)
    for (uint32_t c = threadIdx.x >> 3; c < bound; c += 32) {
        const uint32_t cc = c < nlist ? c : nlist - 1;
        const float s = exact_score<8>(metric, LYNSE_IPFORM_SINGLE, v, C + (uint64_t)cc * ldc, D, g);
        if (g == 0 && c < nlist) s_rank[c] = asc ? s : -s;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (uint32_t j = 0; j < keep; ++j) { s_best[j] = INFINITY; s_bc[j] = 0xffffffffu; }
    for (uint32_t c = 0; c < nlist; ++c) {
        const float rank = s_rank[c];
        if (rank >= s_best[keep - 1]) continue;
        uint32_t pos = keep - 1;
        while (pos > 0 && rank < s_best[pos - 1]) {
            s_best[pos] = s_best[pos - 1];
            s_bc[pos] = s_bc[pos - 1];
            --pos;
        }
        s_best[pos] = rank;
        s_bc[pos] = c;
    }
    uint32_t* out = lists + (uint64_t)row * keep;
    if (s_bc[0] == 0xffffffffu) { out[0] = 0; cnt[row] = 1; return; }   // no finite-ranked centroid: list 0
    out[0] = s_bc[0];
    uint32_t len = 1;
    if (R > 0) {
        const float p = s_best[0];
        const float slack = __fmul_rn(fmaxf(fabsf(p), SPANN_EPS), SPANN_SLACK);   // (fmaxf ignores a NaN operand, as f32::max)
        const float threshold = __fadd_rn(p, slack);
        for (uint32_t j = 1; j < keep; ++j) {
            if (s_bc[j] == 0xffffffffu) continue;
            if (len <= R && s_best[j] <= threshold) out[len++] = s_bc[j];
        }
    }
    cnt[row] = len;
}

// ------------------------------------------------------------------------------------------------
// k_spann_unique — one wave per query: the query's canonically sorted keys (rows[i], dists[i], i < cnt[q], stride in_k) hold the
// replicas of a row next to each other; the first k_sel DISTINCT rows go to out_rows / out_dists (stride out_k) of output query
// qmap[q] (q when qmap is NULL), their number to out_cnt.  With out_dists the slots behind them up to out_k are padded as every
// search result of the C ABI is (row ~0, the worst distance of the metric: +inf ascending, -inf for IP); out_dists may be NULL (the
// SQ8 pool keeps rows and counts only).
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) k_spann_unique(const uint64_t* __restrict__ rows, const float* __restrict__ dists,
                                                     const uint32_t* __restrict__ cnt, uint32_t in_k, uint32_t nq, uint32_t k_sel,
                                                     const uint32_t* __restrict__ qmap, uint64_t* __restrict__ out_rows,
                                                     float* __restrict__ out_dists, uint32_t* __restrict__ out_cnt, uint32_t out_k, int asc) {
    const uint32_t q = blockIdx.x;
    if (q >= nq) return;
    const uint32_t lane = threadIdx.x;
    const uint32_t oq = qmap ? qmap[q] : q;
    const uint64_t* r = rows + (uint64_t)q * in_k;
    const uint32_t n = min(cnt[q], in_k);
    uint32_t written = 0;
    for (uint32_t base = 0; base < n && written < k_sel; base += 64) {
        const uint32_t i = base + lane;
        const bool first = i < n && (i == 0 || r[i] != r[i - 1]);
        const uint64_t m = __ballot(first);
        const uint32_t slot = written + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (first && slot < k_sel) {
            out_rows[(uint64_t)oq * out_k + slot] = r[i];
            if (out_dists) out_dists[(uint64_t)oq * out_k + slot] = dists[(uint64_t)q * in_k + i];
        }
        written += (uint32_t)__popcll(m);
    }
    const uint32_t got = min(written, k_sel);
    if (out_dists)
        for (uint32_t i = got + lane; i < out_k; i += 64) {
            out_rows[(uint64_t)oq * out_k + i] = ~0ull;
            out_dists[(uint64_t)oq * out_k + i] = asc ? INFINITY : -INFINITY;
        }
    if (lane == 0) out_cnt[oq] = got;
}

}  // namespace lynse
