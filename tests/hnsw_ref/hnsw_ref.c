/* hnsw_ref.c — the CPU restatement of the HNSW rule block of include/lynse_hip.h: levels (rule 1), the bulk build (rules 2-4) and
 * the search (rule 5, HNSWIndex::search, src/index/hnsw.rs:625-699, :758-777, :1040-1140).  TEST INFRASTRUCTURE: plain C, no
 * cleverness — every distance is computed afresh through the function pointer (the oracle's lo_compute_distance), the heaps are
 * unbounded binary heaps ordered by (dist, node), the visited set is one byte per node.  Built by the tests that use it. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef float (*dist_fn)(const float *a, const float *b, size_t n, int metric);
#define PAD 0xffffffffu
#define M_IP 0

typedef struct { float d; uint32_t node; } DN;

static int dn_less(DN a, DN b) { return a.d < b.d || (a.d == b.d && a.node < b.node); }
static int dn_cmp(const void *x, const void *y) {
    const DN a = *(const DN *)x, b = *(const DN *)y;
    return dn_less(a, b) ? -1 : (dn_less(b, a) ? 1 : 0);
}

/* the graph distance: lower = closer, ip negated (hnsw.rs:536-543); NaN -> +inf at once */
static float gd(dist_fn dist, const float *a, const float *b, size_t dim, int metric) {
    float r = dist(a, b, dim, metric);
    if (metric == M_IP) r = -r;
    return isnan(r) ? INFINITY : r;
}

/* ---- rule 1: SmallRng::seed_from_u64 = xoshiro256++ seeded by SplitMix64 ---- */
static uint64_t rotl(uint64_t x, int k) { return (x << k) | (x >> (64 - k)); }
void hr_levels(uint64_t seed, uint32_t m, int32_t max_level, size_t n, uint32_t *out) {
    uint64_t s[4], st = seed;
    for (int i = 0; i < 4; ++i) {
        st += 0x9e3779b97f4a7c15ull;
        uint64_t z = st;
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        s[i] = z ^ (z >> 31);
    }
    for (size_t i = 0; i < n; ++i) {
        const uint64_t w = rotl(s[0] + s[3], 23) + s[0], t17 = s[1] << 17;
        s[2] ^= s[0]; s[3] ^= s[1]; s[1] ^= s[2]; s[0] ^= s[3]; s[2] ^= t17;
        s[3] = rotl(s[3], 45);
        uint64_t t = w >> 11;
        if (t < 1) t = 1;
        uint32_t level = 0;
        while ((max_level < 0 || level < (uint32_t)max_level) && t * m < (1ull << 53)) { t *= m; ++level; }
        out[i] = level;
    }
}

/* ---- select_neighbors_heuristic (hnsw.rs:550-602); returns the count written to out ---- */
static size_t heuristic(const float *data, size_t dim, int metric, dist_fn dist, const DN *cand, size_t nc, size_t cap, uint32_t *out) {
    size_t ns = 0;
    if (nc <= cap) {
        for (size_t i = 0; i < nc; ++i) out[i] = cand[i].node;
        return nc;
    }
    for (size_t i = 0; i < nc && ns < cap; ++i) {
        int keep = 1;
        for (size_t s = 0; s < ns; ++s)
            if (gd(dist, data + (size_t)cand[i].node * dim, data + (size_t)out[s] * dim, dim, metric) < cand[i].d) { keep = 0; break; }
        if (keep) out[ns++] = cand[i].node;
    }
    for (size_t i = 0; i < nc && ns < cap; ++i) {
        int in = 0;
        for (size_t s = 0; s < ns; ++s) in |= out[s] == cand[i].node;
        if (!in) out[ns++] = cand[i].node;
    }
    return ns;
}

/* ---- rules 2-4.  levels[n] given; adj0[n][2 m] and upper_adj[sum of levels][m] (ascending (node, level)) are filled, PAD-padded.
 * Returns the entry point. ---- */
uint32_t hr_build(const float *data, size_t n, size_t dim, int metric, uint32_t m, uint32_t ef_construction, const uint32_t *levels,
                  dist_fn dist, uint32_t *adj0, uint32_t *upper_adj) {
    uint32_t top = 0, entry = 0;
    size_t nu = 0;
    size_t *uoff = (size_t *)malloc(n * sizeof(size_t));
    for (size_t i = 0; i < n; ++i) { uoff[i] = nu; nu += levels[i]; if (levels[i] > top) top = levels[i]; }
    for (size_t i = 0; i < n; ++i) if (levels[i] == top) { entry = (uint32_t)i; break; }
    memset(adj0, 0xff, n * 2 * m * sizeof(uint32_t));
    memset(upper_adj, 0xff, nu * m * sizeof(uint32_t));
    uint32_t *S = (uint32_t *)malloc(n * sizeof(uint32_t));
    DN *row = (DN *)malloc((n + 1) * sizeof(DN));
    for (uint32_t l = 0; l <= top; ++l) {
        const size_t cap = l == 0 ? 2 * (size_t)m : m;
        size_t ns = 0;
        for (size_t i = 0; i < n; ++i) if (levels[i] >= l) S[ns++] = (uint32_t)i;
        uint32_t *F = (uint32_t *)malloc(ns * cap * sizeof(uint32_t));
        size_t *Fn = (size_t *)calloc(ns, sizeof(size_t));
        size_t *item = (size_t *)malloc(n * sizeof(size_t));
        for (size_t t = 0; t < ns; ++t) item[S[t]] = t;
        for (size_t t = 0; t < ns; ++t) {   /* rules 2 and 3 */
            const uint32_t i = S[t];
            size_t nc = 0;
            for (size_t u = 0; u < ns; ++u)
                if (S[u] != i) { row[nc].node = S[u]; row[nc].d = gd(dist, data + (size_t)i * dim, data + (size_t)S[u] * dim, dim, metric); ++nc; }
            qsort(row, nc, sizeof(DN), dn_cmp);
            if (nc > ef_construction) nc = ef_construction;
            Fn[t] = heuristic(data, dim, metric, dist, row, nc, cap, F + t * cap);
        }
        /* rule 4: U(i) = F(i) and every j with i in F(j) */
        size_t *rcnt = (size_t *)calloc(ns + 1, sizeof(size_t));
        for (size_t t = 0; t < ns; ++t) for (size_t s = 0; s < Fn[t]; ++s) ++rcnt[item[F[t * cap + s]] + 1];
        for (size_t t = 0; t < ns; ++t) rcnt[t + 1] += rcnt[t];
        uint32_t *rev = (uint32_t *)malloc((rcnt[ns] + 1) * sizeof(uint32_t));
        size_t *rfill = (size_t *)malloc((ns + 1) * sizeof(size_t));
        memcpy(rfill, rcnt, (ns + 1) * sizeof(size_t));
        for (size_t t = 0; t < ns; ++t) for (size_t s = 0; s < Fn[t]; ++s) rev[rfill[item[F[t * cap + s]]]++] = S[t];
        for (size_t t = 0; t < ns; ++t) {
            const uint32_t i = S[t];
            size_t nc = 0;
            for (size_t s = 0; s < Fn[t]; ++s) row[nc++].node = F[t * cap + s];
            for (size_t r = rcnt[t]; r < rcnt[t + 1]; ++r) {
                int in = 0;
                for (size_t s = 0; s < Fn[t]; ++s) in |= F[t * cap + s] == rev[r];
                if (!in) row[nc++].node = rev[r];
            }
            for (size_t c = 0; c < nc; ++c) row[c].d = gd(dist, data + (size_t)i * dim, data + (size_t)row[c].node * dim, dim, metric);
            qsort(row, nc, sizeof(DN), dn_cmp);
            uint32_t *dst = l == 0 ? adj0 + (size_t)i * 2 * m : upper_adj + (uoff[i] + l - 1) * m;
            heuristic(data, dim, metric, dist, row, nc, cap, dst);   /* (no more than cap: the ordered list itself) */
        }
        free(rfill); free(rev); free(rcnt); free(item); free(Fn); free(F);
    }
    free(row); free(S); free(uoff);
    return entry;
}

/* ---- rule 5 ---- */
typedef struct { DN *a; size_t n; int max; } Heap;
static int h_before(const Heap *h, DN x, DN y) { return h->max ? dn_less(y, x) : dn_less(x, y); }
static void h_push(Heap *h, DN v) {
    size_t i = h->n++;
    h->a[i] = v;
    while (i && h_before(h, h->a[i], h->a[(i - 1) / 2])) { DN t = h->a[i]; h->a[i] = h->a[(i - 1) / 2]; h->a[(i - 1) / 2] = t; i = (i - 1) / 2; }
}
static DN h_pop(Heap *h) {
    DN top = h->a[0];
    h->a[0] = h->a[--h->n];
    size_t i = 0;
    for (;;) {
        size_t l = 2 * i + 1, r = l + 1, b = i;
        if (l < h->n && h_before(h, h->a[l], h->a[b])) b = l;
        if (r < h->n && h_before(h, h->a[r], h->a[b])) b = r;
        if (b == i) break;
        DN t = h->a[i]; h->a[i] = h->a[b]; h->a[b] = t;
        i = b;
    }
    return top;
}

/* lists: adj0[n][2 m]; upper_adj rows in ascending (node, level) order, found through the levels; PAD entries are skipped.
 * ef is the caller's max(ef_query or ef_search, k).  Returns the count; *scored = distances computed. */
size_t hr_search(const float *data, size_t n, size_t dim, int metric, uint32_t m, const uint32_t *levels, const uint32_t *adj0,
                 const uint32_t *upper_adj, uint32_t entry, const float *query, size_t k, size_t ef, dist_fn dist, uint64_t *out_rows,
                 float *out_dists, uint64_t *scored) {
    size_t *uoff = (size_t *)malloc(n * sizeof(size_t));
    size_t nu = 0, ns = 0;
    for (size_t i = 0; i < n; ++i) { uoff[i] = nu; nu += levels[i]; }
    uint32_t cur = entry;
    float cd = gd(dist, data + (size_t)cur * dim, query, dim, metric);
    ns = 1;
    for (uint32_t l = levels[entry]; l >= 1; --l) {   /* greedy_closest: a pass scans the list of the node it started from */
        for (;;) {
            const uint32_t *list = upper_adj + (uoff[cur] + l - 1) * m;
            int changed = 0;
            for (uint32_t s = 0; s < m; ++s) {
                if (list[s] == PAD) continue;
                const float d = gd(dist, data + (size_t)list[s] * dim, query, dim, metric);
                ++ns;
                if (d < cd) { cd = d; cur = list[s]; changed = 1; }
            }
            if (!changed) break;
        }
    }
    uint8_t *vis = (uint8_t *)calloc(n, 1);
    Heap C = {(DN *)malloc((n + 1) * sizeof(DN)), 0, 0}, R = {(DN *)malloc((n + 2) * sizeof(DN)), 0, 1};
    const DN e = {cd, cur};
    vis[cur] = 1;
    h_push(&C, e);
    h_push(&R, e);
    while (C.n) {
        const DN c = h_pop(&C);
        if (c.d > R.a[0].d && R.n >= ef) break;
        const uint32_t *list = adj0 + (size_t)c.node * 2 * m;
        for (uint32_t s = 0; s < 2 * m; ++s) {
            const uint32_t nb = list[s];
            if (nb == PAD || vis[nb]) continue;
            vis[nb] = 1;
            const DN v = {gd(dist, data + (size_t)nb * dim, query, dim, metric), nb};
            ++ns;
            if (R.n < ef || v.d < R.a[0].d) {
                h_push(&C, v);
                h_push(&R, v);
                if (R.n > ef) (void)h_pop(&R);
            }
        }
    }
    qsort(R.a, R.n, sizeof(DN), dn_cmp);
    const size_t cnt = k < R.n ? k : R.n;
    for (size_t i = 0; i < cnt; ++i) {
        out_rows[i] = R.a[i].node;
        out_dists[i] = metric == M_IP ? -R.a[i].d : R.a[i].d;
    }
    if (scored) *scored = ns;
    free(C.a); free(R.a); free(vis); free(uoff);
    return cnt;
}
