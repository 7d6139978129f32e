/* diskann_ref.c — the CPU restatement of the DiskANN rule block of include/lynse_hip.h: the random draws (rules 1-4), the batched
 * Vamana build (rules 5-7: vamana_pass, robust_prune, apply_vamana_updates, src/index/diskann.rs:830-875, :979-1113) and the search
 * (rule 8: search_graph, :880-973).  TEST INFRASTRUCTURE: plain C, no cleverness — every distance is computed afresh through the
 * function pointer (the oracle's lo_compute_distance), the heaps are unbounded binary heaps ordered by (dist, node), the visited set is
 * one byte per node, the commit is sequential exactly as apply_vamana_updates reads.  Built by the tests that use it. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef float (*dist_fn)(const float *a, const float *b, size_t n, int metric);
#define PAD 0xffffffffu
#define BATCH 256

typedef struct { float d; uint32_t node; } DN;
typedef struct { uint32_t *a; size_t n, cap; } List;

static int dn_less(DN a, DN b) { return a.d < b.d || (a.d == b.d && a.node < b.node); }
static int dn_cmp(const void *x, const void *y) {
    const DN a = *(const DN *)x, b = *(const DN *)y;
    return dn_less(a, b) ? -1 : (dn_less(b, a) ? 1 : 0);
}
static void l_push(List *l, uint32_t v) {
    if (l->n == l->cap) { l->cap = l->cap ? 2 * l->cap : 8; l->a = (uint32_t *)realloc(l->a, l->cap * sizeof(uint32_t)); }
    l->a[l->n++] = v;
}
static int l_has(const List *l, uint32_t v) {
    for (size_t i = 0; i < l->n; ++i) if (l->a[i] == v) return 1;
    return 0;
}

/* rule 0: lower = closer (l2 / cosine only); NaN -> +inf at once */
static float gd(dist_fn dist, const float *a, const float *b, size_t dim, int metric) {
    const float r = dist(a, b, dim, metric);
    return isnan(r) ? INFINITY : r;
}

/* ---- rule 1: SmallRng::seed_from_u64 = xoshiro256++ seeded by SplitMix64 ---- */
typedef struct { uint64_t s[4]; } Rng;
static uint64_t rotl(uint64_t x, int k) { return (x << k) | (x >> (64 - k)); }
static void rng_seed(Rng *g, uint64_t seed) {
    uint64_t st = seed;
    for (int i = 0; i < 4; ++i) {
        st += 0x9e3779b97f4a7c15ull;
        uint64_t z = st;
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        g->s[i] = z ^ (z >> 31);
    }
}
static uint64_t rng_next(Rng *g) {
    uint64_t *s = g->s;
    const uint64_t w = rotl(s[0] + s[3], 23) + s[0], t17 = s[1] << 17;
    s[2] ^= s[0]; s[3] ^= s[1]; s[1] ^= s[2]; s[0] ^= s[3]; s[2] ^= t17;
    s[3] = rotl(s[3], 45);
    return w;
}
static uint64_t rng_draw(Rng *g, uint64_t b) { return ((rng_next(g) >> 32) * b) >> 32; }
static void shuffle(Rng *g, uint32_t *a, size_t n) {
    for (size_t i = 0; i < n; ++i) a[i] = (uint32_t)i;
    for (size_t i = n; i-- > 1;) {
        const size_t j = (size_t)rng_draw(g, i + 1);
        const uint32_t t = a[i]; a[i] = a[j]; a[j] = t;
    }
}

/* rules 1-4 without the rows: refs[min(32, n)], cands[min(64, n)], order[n] before the entry swap, adj0[n][r] padded */
void dr_draws(uint64_t seed, size_t n, uint32_t r, uint32_t *refs, uint32_t *cands, uint32_t *order, uint32_t *adj0) {
    Rng g;
    rng_seed(&g, seed);
    memset(adj0, 0xff, n * r * sizeof(uint32_t));
    if (n <= 1) {
        if (n) refs[0] = cands[0] = order[0] = 0;
        return;
    }
    uint32_t *tmp = (uint32_t *)malloc(n * sizeof(uint32_t));
    shuffle(&g, tmp, n);
    memcpy(refs, tmp, (n < 32 ? n : 32) * sizeof(uint32_t));
    shuffle(&g, tmp, n);
    memcpy(cands, tmp, (n < 64 ? n : 64) * sizeof(uint32_t));
    const size_t deg = r < n - 1 ? r : n - 1;
    for (size_t i = 0; i < n; ++i) {
        uint32_t *row = adj0 + i * r;
        size_t c = 0;
        while (c < deg) {
            const uint32_t j = (uint32_t)rng_draw(&g, n);
            int in = j == i;
            for (size_t s = 0; s < c; ++s) in |= row[s] == j;
            if (!in) row[c++] = j;
        }
    }
    shuffle(&g, order, n);
    free(tmp);
}

/* search_entry_points (:159-174); returns the count */
size_t dr_starts(size_t n, size_t primary, size_t anchors, uint32_t *out) {
    const size_t ac = anchors < n ? anchors : n;
    size_t c = 0;
    out[c++] = (uint32_t)primary;
    for (size_t a = 0; a < ac; ++a) {
        const size_t idx = (size_t)((uint64_t)a * (uint64_t)n / (uint64_t)ac);
        if (idx != primary) out[c++] = (uint32_t)idx;
    }
    return c;
}

/* ---- rule 6: robust_prune, ascending branch; cand is overwritten; returns the count written to out ---- */
static size_t prune(const float *data, size_t dim, int metric, dist_fn dist, uint32_t p, DN *cand, size_t nc, uint32_t r, float alpha, uint32_t *out) {
    size_t m = 0;
    for (size_t i = 0; i < nc; ++i) {
        int skip = cand[i].node == p;
        for (size_t j = 0; j < m && !skip; ++j) skip = cand[j].node == cand[i].node;
        if (!skip) cand[m++] = cand[i];
    }
    qsort(cand, m, sizeof(DN), dn_cmp);
    size_t ns = 0;
    while (m && ns < r) {
        const uint32_t best = cand[0].node;
        out[ns++] = best;
        size_t w = 0;
        for (size_t i = 0; i < m; ++i) {
            if (cand[i].node == best) continue;
            const float dbv = gd(dist, data + (size_t)best * dim, data + (size_t)cand[i].node * dim, dim, metric);
            const float scaled = alpha * dbv;
            if (scaled > cand[i].d) cand[w++] = cand[i];
        }
        m = w;
    }
    return ns;
}
/* the prune alone, over caller-given candidates (d(p, .), node): for known-answer tests */
size_t dr_prune(const float *data, size_t dim, int metric, dist_fn dist, uint32_t p, const float *cd, const uint32_t *cn, size_t nc, uint32_t r, float alpha,
                uint32_t *out) {
    DN *c = (DN *)malloc((nc + 1) * sizeof(DN));
    for (size_t i = 0; i < nc; ++i) { c[i].d = cd[i]; c[i].node = cn[i]; }
    const size_t ns = prune(data, dim, metric, dist, p, c, nc, r, alpha, out);
    free(c);
    return ns;
}

/* ---- rule 8 ---- */
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

/* search_graph: R sorted by (dist, node) into out (room for n + 2), the count returned; *scored += distances computed */
static size_t search_graph(const float *data, size_t n, size_t dim, int metric, const List *G, uint32_t entry, const float *query, size_t ef,
                           size_t anchors, dist_fn dist, DN *out, uint64_t *scored) {
    if (ef < 1) ef = 1;
    uint8_t *vis = (uint8_t *)calloc(n, 1);
    Heap C = {(DN *)malloc((n + 1) * sizeof(DN)), 0, 0}, R = {out, 0, 1};
    uint32_t starts[64];
    const size_t ns = dr_starts(n, entry, anchors, starts);
    for (size_t s = 0; s < ns; ++s) {
        if (vis[starts[s]]) continue;
        vis[starts[s]] = 1;
        const DN v = {gd(dist, data + (size_t)starts[s] * dim, query, dim, metric), starts[s]};
        ++*scored;
        h_push(&C, v);
        h_push(&R, v);
        if (R.n > ef) (void)h_pop(&R);
    }
    while (C.n) {
        const DN c = h_pop(&C);
        if (R.n >= ef && c.d > R.a[0].d) break;
        const List *list = &G[c.node];
        for (size_t s = 0; s < list->n; ++s) {
            const uint32_t nb = list->a[s];
            if (vis[nb]) continue;
            vis[nb] = 1;
            const DN v = {gd(dist, data + (size_t)nb * dim, query, dim, metric), nb};
            ++*scored;
            if (R.n < ef || v.d < R.a[0].d) {
                h_push(&C, v);
                h_push(&R, v);
                if (R.n > ef) (void)h_pop(&R);
            }
        }
    }
    qsort(R.a, R.n, sizeof(DN), dn_cmp);
    free(C.a); free(vis);
    return R.n;
}

static List *lists_from(const uint32_t *adj, size_t n, uint32_t r) {
    List *G = (List *)calloc(n ? n : 1, sizeof(List));
    for (size_t i = 0; i < n; ++i)
        for (uint32_t s = 0; s < r; ++s)
            if (adj[i * r + s] != PAD && !l_has(&G[i], adj[i * r + s])) l_push(&G[i], adj[i * r + s]);
    return G;
}
static void lists_free(List *G, size_t n) {
    for (size_t i = 0; i < n; ++i) free(G[i].a);
    free(G);
}

/* a query over adj[n][r] (PAD entries skipped): ef is the caller's min(max(ef_query, l, 10 k), n).  Returns the count. */
size_t dr_search(const float *data, size_t n, size_t dim, int metric, uint32_t r, const uint32_t *adj, uint32_t entry, const float *query, size_t k,
                 size_t ef, size_t anchors, dist_fn dist, uint64_t *out_rows, float *out_dists, uint64_t *scored) {
    List *G = lists_from(adj, n, r);
    DN *res = (DN *)malloc((n + 2) * sizeof(DN));
    uint64_t sc = 0;
    const size_t rn = search_graph(data, n, dim, metric, G, entry, query, ef, anchors, dist, res, &sc);
    const size_t cnt = k < rn ? k : rn;
    for (size_t i = 0; i < cnt; ++i) { out_rows[i] = res[i].node; out_dists[i] = res[i].d; }
    if (scored) *scored = sc;
    free(res);
    lists_free(G, n);
    return cnt;
}

/* ---- rules 1-7.  adj[n][r] is filled, PAD-padded; *longest = the longest list a commit pruned.  Returns the entry point. ---- */
uint32_t dr_build(const float *data, size_t n, size_t dim, int metric, uint32_t r, uint32_t l, float alpha, uint64_t seed, uint64_t max_batches,
                  dist_fn dist, uint32_t *adj, uint32_t *longest) {
    if (l < r) l = r;
    uint32_t *refs = (uint32_t *)malloc(64 * sizeof(uint32_t)), *cands = (uint32_t *)malloc(64 * sizeof(uint32_t));
    uint32_t *order = (uint32_t *)malloc((n + 1) * sizeof(uint32_t));
    dr_draws(seed, n, r, refs, cands, order, adj);
    uint32_t entry = 0;
    if (n > 1) {   /* rule 2 */
        const size_t nr = n < 32 ? n : 32, nc = n < 64 ? n : 64;
        float best_sum = INFINITY;
        entry = cands[0];
        for (size_t c = 0; c < nc; ++c) {
            float sum = 0.0f;
            for (size_t j = 0; j < nr; ++j) sum += gd(dist, data + (size_t)cands[c] * dim, data + (size_t)refs[j] * dim, dim, metric);
            if (sum < best_sum) { best_sum = sum; entry = cands[c]; }
        }
    }
    for (size_t i = 0; i < n; ++i)   /* rule 4 */
        if (order[i] == entry) { const uint32_t t = order[0]; order[0] = order[i]; order[i] = t; break; }
    List *G = lists_from(adj, n, r);
    const size_t Lb = (l < 128 ? l : 128) > r ? (l < 128 ? l : 128) : r;
    DN *res = (DN *)malloc((n + r + 2 + BATCH) * sizeof(DN));
    uint32_t *F = (uint32_t *)malloc((size_t)BATCH * r * sizeof(uint32_t));
    size_t *Fn = (size_t *)malloc(BATCH * sizeof(size_t));
    uint32_t *touched = (uint32_t *)malloc((size_t)BATCH * r * sizeof(uint32_t)), *tmp = (uint32_t *)malloc(r * sizeof(uint32_t));
    uint8_t *was = (uint8_t *)calloc(n ? n : 1, 1);
    uint64_t sc = 0, batches = 0;
    int stop = 0;
    *longest = 0;
    const int passes = alpha > 1.0f + 1.1920929e-7f ? 2 : 1;
    for (int pass = 0; pass < passes && !stop; ++pass) {
        const float al = pass == 0 ? 1.0f : alpha;
        for (size_t b0 = 0; b0 < n && !stop; b0 += BATCH) {
            const size_t B = n - b0 < BATCH ? n - b0 : BATCH;
            for (size_t t = 0; t < B; ++t) {   /* rule 5, against the graph as the batch found it */
                const uint32_t p = order[b0 + t];
                size_t nc = search_graph(data, n, dim, metric, G, entry, data + (size_t)p * dim, Lb, 32, dist, res, &sc);
                for (size_t s = 0; s < G[p].n; ++s) {
                    res[nc].node = G[p].a[s];
                    res[nc].d = gd(dist, data + (size_t)p * dim, data + (size_t)G[p].a[s] * dim, dim, metric);
                    ++nc;
                }
                Fn[t] = prune(data, dim, metric, dist, p, res, nc, r, al, F + t * r);
            }
            /* rule 7: apply_vamana_updates */
            for (size_t t = 0; t < B; ++t) {
                List *g = &G[order[b0 + t]];
                g->n = 0;
                for (size_t s = 0; s < Fn[t]; ++s) l_push(g, F[t * r + s]);
            }
            size_t nt = 0;
            for (size_t t = 0; t < B; ++t) {
                const uint32_t src = order[b0 + t];
                for (size_t s = 0; s < Fn[t]; ++s) {
                    const uint32_t dst = F[t * r + s];
                    if (dst == src) continue;
                    if (!l_has(&G[dst], src)) l_push(&G[dst], src);
                    if (!was[dst]) { was[dst] = 1; touched[nt++] = dst; }
                }
            }
            for (size_t u = 0; u < nt; ++u) {
                const uint32_t dst = touched[u];
                was[dst] = 0;
                List *g = &G[dst];
                if (g->n <= r) continue;
                if (g->n > *longest) *longest = (uint32_t)g->n;
                for (size_t s = 0; s < g->n; ++s) {
                    res[s].node = g->a[s];
                    res[s].d = gd(dist, data + (size_t)dst * dim, data + (size_t)g->a[s] * dim, dim, metric);
                }
                const size_t ns = prune(data, dim, metric, dist, dst, res, g->n, r, al, tmp);
                g->n = 0;
                for (size_t s = 0; s < ns; ++s) l_push(g, tmp[s]);
            }
            stop = ++batches == max_batches;
        }
    }
    memset(adj, 0xff, n * r * sizeof(uint32_t));
    for (size_t i = 0; i < n; ++i) memcpy(adj + i * r, G[i].a, G[i].n * sizeof(uint32_t));
    lists_free(G, n);
    free(was); free(tmp); free(touched); free(Fn); free(F); free(res); free(order); free(cands); free(refs);
    return entry;
}
