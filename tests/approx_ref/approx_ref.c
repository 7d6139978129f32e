/* A restatement of THE APPROXIMATE FLAT SEARCH of include/lynse_hip.h, written from that contract block: plain C, eight explicit lanes,
 * f32 throughout, one thread.  Compiled by the tests with -O2 -ffp-contract=off -fno-fast-math (fused operations are written as fmaf).
 * Ties follow the contract: every selection — the pool and the final k — is by the canonical key (score in metric order, row
 * ascending), a NaN score ordering last with the worst infinity and -0.0 being +0.0.  Besides the answer it hands out the coarse scores
 * and the pool, so that a test can plant a row at a chosen coarse rank. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

enum { M_IP = 0, M_L2 = 1, M_COS = 2, M_L1 = 7, M_CHEB = 8, M_CANB = 9, M_BRAY = 10 };

/* ---- eps ---- */
float apx_normalize_eps(float eps) {
    if (isfinite(eps) && eps > 0.0f) return eps > 1e-8f ? eps : 1e-8f;
    return 1e-4f;
}

float apx_round_to_eps(float v, float eps) {
    if (!isfinite(v) || !(eps > 0.0f)) return v;
    float scaled = v / eps;
    if (!isfinite(scaled)) return v;
    float r = roundf(scaled) * eps; /* half away from zero */
    return isfinite(r) ? r : v;
}

/* ---- the size policy ---- */
static int band(float eps) {
    if (eps <= 1e-6f) return 0;
    if (eps <= 1e-5f) return 1;
    if (eps <= 1e-4f) return 2;
    if (eps <= 1e-3f) return 3;
    if (eps <= 1e-2f) return 4;
    return 5;
}
static uint64_t umax(uint64_t a, uint64_t b) { return a > b ? a : b; }
static uint64_t umin(uint64_t a, uint64_t b) { return a < b ? a : b; }

uint64_t apx_ip_order_pool(uint64_t k, uint64_t n, float eps) {
    static const uint64_t per_k[6] = {1000, 750, 500, 250, 120, 60}, div[6] = {100, 133, 200, 400, 800, 1600};
    int b = band(eps);
    uint64_t p = umax(umax(k * per_k[b], n / div[b]), k + 128);
    return umin(umin(p, n), umax(20000, umin(k, n)));
}
uint64_t apx_hybrid_ip_pool(uint64_t k, uint64_t n, float eps) {
    static const uint64_t per_k[6] = {8000, 6000, 5000, 3000, 2000, 1000}, div[6] = {20, 20, 20, 40, 80, 160};
    int b = band(eps);
    return umin(umin(umax(umax(k * per_k[b], n / div[b]), k + 128), n), 100000);
}
uint64_t apx_hybrid_pool(uint64_t k, uint64_t n, float eps) {
    static const uint64_t per_k[6] = {4000, 3000, 2000, 1000, 500, 250}, div[6] = {50, 50, 50, 100, 200, 400};
    int b = band(eps);
    return umin(umin(umax(umax(k * per_k[b], n / div[b]), k + 128), n), 100000);
}
static uint32_t sample_of(uint32_t dim, float ratio) {
    if (dim <= 32) return dim;
    uint32_t s = (uint32_t)roundf((float)dim * ratio);
    if (s < 32) s = 32;
    return s < dim ? s : dim;
}
uint32_t apx_hybrid_ip_sample(uint32_t dim, float eps) {
    static const float r[6] = {0.75f, 0.625f, 0.5f, 0.375f, 0.25f, 0.25f};
    return sample_of(dim, r[band(eps)]);
}
uint32_t apx_hybrid_sample(uint32_t dim, float eps) {
    static const float r[6] = {0.875f, 0.75f, 0.625f, 0.5f, 0.375f, 0.25f};
    return sample_of(dim, r[band(eps)]);
}
/* head, middle, tail: start[i], len[i]; returns the number of blocks */
uint32_t apx_blocks(uint32_t dim, uint32_t sample, uint32_t *start, uint32_t *len) {
    if (sample > dim) sample = dim;
    if (sample == 0) return 0;
    if (sample == dim) { start[0] = 0; len[0] = dim; return 1; }
    uint32_t nb = sample < 3 ? sample : 3;
    if (nb == 1) { start[0] = (dim - sample) / 2; len[0] = sample; return 1; }
    uint32_t remaining = sample;
    for (uint32_t i = 0; i < nb; ++i) {
        uint32_t left = nb - i, l = (remaining + left - 1) / left;
        remaining -= l;
        uint32_t max_start = dim > l ? dim - l : 0;
        start[i] = (i * max_start + (nb - 1) / 2) / (nb - 1);
        len[i] = l;
    }
    return nb;
}

/* ---- the forms ---- */
static float hsum8(const float *t) { return ((t[0] + t[4]) + (t[1] + t[5])) + ((t[2] + t[6]) + (t[3] + t[7])); }

/* single-row IP: two accumulators over chunks of 16 (fused), one more chunk of 8 into the first, acc0 + acc1, the pairwise sum, the tail */
static float ip_single(const float *a, const float *b, size_t D) {
    float a0[8] = {0, 0, 0, 0, 0, 0, 0, 0}, a1[8] = {0, 0, 0, 0, 0, 0, 0, 0}, t[8];
    size_t chunks = D / 8, dbl = chunks / 2;
    for (size_t i = 0; i < dbl; ++i)
        for (int g = 0; g < 8; ++g) {
            a0[g] = fmaf(a[16 * i + g], b[16 * i + g], a0[g]);
            a1[g] = fmaf(a[16 * i + 8 + g], b[16 * i + 8 + g], a1[g]);
        }
    if (chunks & 1)
        for (int g = 0; g < 8; ++g) a0[g] = fmaf(a[16 * dbl + g], b[16 * dbl + g], a0[g]);
    for (int g = 0; g < 8; ++g) t[g] = a0[g] + a1[g];
    float s = hsum8(t);
    for (size_t i = chunks * 8; i < D; ++i) s = s + a[i] * b[i];
    return s;
}
/* batch-of-8 IP: one accumulator (fused), the pairwise sum, the tail */
static float ip_batch8(const float *a, const float *b, size_t D) {
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    size_t chunks = D / 8;
    for (size_t i = 0; i < chunks; ++i)
        for (int g = 0; g < 8; ++g) acc[g] = fmaf(a[8 * i + g], b[8 * i + g], acc[g]);
    float s = hsum8(acc);
    for (size_t i = chunks * 8; i < D; ++i) s = s + a[i] * b[i];
    return s;
}
static float ip_form(int batch8, const float *a, const float *b, size_t D) { return batch8 ? ip_batch8(a, b, D) : ip_single(a, b, D); }

static float rmax(float x, float y) { /* Rust's f32::max */
    if (x != x) return y;
    if (y != y) return x;
    return x > y ? x : y;
}
static float l1(const float *a, const float *b, size_t D) {
    size_t chunks = D / 8;
    float lane[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (size_t i = 0; i < chunks; ++i)
        for (int g = 0; g < 8; ++g) lane[g] = lane[g] + fabsf(a[8 * i + g] - b[8 * i + g]);
    float s = 0.0f;
    for (int g = 0; g < 8; ++g) s = s + lane[g];
    for (size_t i = chunks * 8; i < D; ++i) s = s + fabsf(a[i] - b[i]);
    return s;
}
static float chebyshev(const float *a, const float *b, size_t D) {
    size_t chunks = D / 8;
    float lane[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (size_t i = 0; i < chunks; ++i)
        for (int g = 0; g < 8; ++g) {
            float d = fabsf(a[8 * i + g] - b[8 * i + g]);
            lane[g] = (lane[g] > d) ? lane[g] : d;
        }
    float m = 0.0f;
    for (int g = 0; g < 8; ++g) m = rmax(m, lane[g]);
    for (size_t i = chunks * 8; i < D; ++i) m = rmax(m, fabsf(a[i] - b[i]));
    return m;
}
static float canberra(const float *a, const float *b, size_t D) {
    size_t chunks = D / 8;
    float lane[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (size_t i = 0; i < chunks; ++i)
        for (int g = 0; g < 8; ++g) {
            float x = a[8 * i + g], y = b[8 * i + g], den = fabsf(x) + fabsf(y), q = fabsf(x - y) / den;
            lane[g] = lane[g] + (((den < 0.0f) || (den > 0.0f)) ? q : 0.0f);
        }
    float s = 0.0f;
    for (int g = 0; g < 8; ++g) s = s + lane[g];
    for (size_t i = chunks * 8; i < D; ++i) {
        float den = fabsf(a[i]) + fabsf(b[i]);
        if (den != 0.0f) s = s + fabsf(a[i] - b[i]) / den;
    }
    return s;
}
static float bray_finish(float num, float den) { return den == 0.0f ? (num == 0.0f ? 0.0f : INFINITY) : num / den; }
static float bray_curtis(const float *a, const float *b, size_t D) {
    size_t chunks = D / 8;
    float nl[8] = {0, 0, 0, 0, 0, 0, 0, 0}, dl[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (size_t i = 0; i < chunks; ++i)
        for (int g = 0; g < 8; ++g) {
            nl[g] = nl[g] + fabsf(a[8 * i + g] - b[8 * i + g]);
            dl[g] = dl[g] + fabsf(a[8 * i + g] + b[8 * i + g]);
        }
    float num = 0.0f, den = 0.0f;
    for (int g = 0; g < 8; ++g) num = num + nl[g];
    for (int g = 0; g < 8; ++g) den = den + dl[g];
    for (size_t i = chunks * 8; i < D; ++i) {
        num = num + fabsf(a[i] - b[i]);
        den = den + fabsf(a[i] + b[i]);
    }
    return bray_finish(num, den);
}
static float additive(int metric, const float *a, const float *b, size_t D) {
    switch (metric) {
    case M_L1: return l1(a, b, D);
    case M_CHEB: return chebyshev(a, b, D);
    case M_CANB: return canberra(a, b, D);
    default: return bray_curtis(a, b, D);
    }
}

/* four 8-lane accumulators over chunks of 32, (acc0 + acc1) + (acc2 + acc3), the lanes 0 -> 7 from 0.0, the tail */
float apx_row_sum(const float *v, size_t D) {
    float acc[4][8];
    memset(acc, 0, sizeof acc);
    size_t c32 = D / 32;
    for (size_t c = 0; c < c32; ++c)
        for (int j = 0; j < 4; ++j)
            for (int g = 0; g < 8; ++g) acc[j][g] = acc[j][g] + v[32 * c + 8 * j + g];
    float s = 0.0f;
    for (int g = 0; g < 8; ++g) s = s + ((acc[0][g] + acc[1][g]) + (acc[2][g] + acc[3][g]));
    for (size_t i = c32 * 32; i < D; ++i) s = s + v[i];
    return s;
}

/* ---- the canonical key ---- */
static uint64_t key_of(float s, uint32_t row, int asc) {
    if (s != s) s = asc ? INFINITY : -INFINITY;
    s = s + 0.0f;
    uint32_t u;
    memcpy(&u, &s, 4);
    uint32_t o = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    if (!asc) o = ~o;
    return ((uint64_t)o << 32) | row;
}
static float key_score(uint64_t key, int asc) {
    uint32_t o = (uint32_t)(key >> 32);
    if (!asc) o = ~o;
    uint32_t u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
    float s;
    memcpy(&s, &u, 4);
    return s;
}
static int cmp_u64(const void *a, const void *b) {
    uint64_t x = *(const uint64_t *)a, y = *(const uint64_t *)b;
    return x < y ? -1 : (x > y ? 1 : 0);
}
/* the best `take` of m keys, best first, into rows / dists; returns their number */
static uint32_t best_of(uint64_t *keys, size_t m, size_t take, int asc, uint64_t *rows, float *dists) {
    qsort(keys, m, 8, cmp_u64);
    if (take > m) take = m;
    for (size_t i = 0; i < take; ++i) {
        rows[i] = (uint32_t)keys[i];
        dists[i] = key_score(keys[i], asc);
    }
    return (uint32_t)take;
}

static float exact_of(int metric, int batch8, const float *q, const float *v, size_t D) {
    return metric == M_IP ? ip_form(batch8, q, v, D) : additive(metric, q, v, D);
}

/* info: path, ip_case (1 sum descending, 2 sum ascending, 3 hybrid), pool, sample_dims, fell_back.
 * ip_form: 0 = by the row count (single below 4,096 rows), 1 = single, 2 = batch-of-8.
 * coarse (n floats, may be NULL): the coarse score of every row — paths 1 and 2: the distance itself, a sum order: the row sum.
 * pool_rows (may be NULL; room for 100,000): the pool in canonical order, *pool_cnt its size.  eps is normalised here.
 * Returns the number of results (raw distances, best first). */
uint32_t apx_search(const float *q, const float *rows, size_t n, size_t D, uint32_t k_in, int metric, float eps, int ip_form_set,
                    uint64_t *out_rows, float *out_dists, uint32_t *info, float *coarse, uint32_t *pool_rows, uint32_t *pool_cnt) {
    memset(info, 0, 5 * sizeof(uint32_t));
    if (pool_cnt) *pool_cnt = 0;
    if (n == 0 || k_in == 0) return 0;
    eps = apx_normalize_eps(eps);
    size_t k = k_in < n ? k_in : n;
    int asc = metric != M_IP, big = D > 16 && n > 65536;
    int batch8 = ip_form_set == 2 || (ip_form_set == 0 && n >= 4096);
    uint64_t *keys = malloc(n * 8);
    uint32_t cnt = 0;
    size_t pool = 0;
    int pooled = 0, exact = 0, score_asc = asc;
    uint32_t start[3] = {0, 0, 0}, len[3] = {(uint32_t)D, 0, 0}, nb = 1;

    if (metric == M_IP && big) {
        info[0] = 3;
        int nonneg = 1, nonpos = 1;
        for (size_t i = 0; i < D; ++i) { nonneg = nonneg && q[i] >= 0.0f; nonpos = nonpos && q[i] <= 0.0f; }
        pooled = 1;
        if (nonneg || nonpos) {
            info[1] = nonneg ? 1 : 2;
            pool = apx_ip_order_pool(k, n, eps);
            info[2] = (uint32_t)pool;
            score_asc = !nonneg;
            size_t m = 0;
            for (size_t r = 0; r < n; ++r) {
                float s = apx_row_sum(rows + r * D, D);
                if (coarse) coarse[r] = s;
                if (isfinite(s)) keys[m++] = key_of(s, (uint32_t)r, score_asc);
            }
            qsort(keys, m, 8, cmp_u64);
            if (pool > m) pool = m;
        } else {
            info[1] = 3;
            uint32_t sample = apx_hybrid_ip_sample((uint32_t)D, eps);
            pool = apx_hybrid_ip_pool(k, n, eps);
            info[2] = (uint32_t)pool;
            info[3] = sample;
            if (sample >= D || pool >= n) exact = 1;
            else {
                nb = apx_blocks((uint32_t)D, sample, start, len);
                for (size_t r = 0; r < n; ++r) {
                    float acc = 0.0f;
                    for (uint32_t b = 0; b < nb; ++b) acc = acc + ip_form(batch8, q + start[b], rows + r * D + start[b], len[b]);
                    if (coarse) coarse[r] = acc;
                    keys[r] = key_of(acc, (uint32_t)r, 0);
                }
                qsort(keys, n, 8, cmp_u64);
            }
        }
    } else if (metric == M_L2 || metric == M_COS) {
        info[0] = 1;
        float qn2 = ip_single(q, q, D), qinv = qn2 > 1e-30f ? 1.0f / sqrtf(qn2) : 0.0f;
        if (metric == M_COS && qinv <= 0.0f) {
            for (size_t i = 0; i < k; ++i) { out_rows[i] = i; out_dists[i] = 1.0f; }
            free(keys);
            return (uint32_t)k;
        }
        for (size_t r = 0; r < n; ++r) {
            const float *v = rows + r * D;
            float n2 = ip_single(v, v, D), inv = n2 > 1e-30f ? 1.0f / sqrtf(n2) : 0.0f, dot = ip_form(batch8, q, v, D), d;
            if (metric == M_L2) {
                d = (qn2 + n2) - 2.0f * dot;
                d = d > 0.0f ? d : 0.0f;
            } else {
                d = inv <= 0.0f ? 1.0f : 1.0f - (dot * qinv) * inv;
            }
            if (coarse) coarse[r] = d;
            keys[r] = key_of(d, (uint32_t)r, 1);
        }
        cnt = best_of(keys, n, k, 1, out_rows, out_dists);
    } else if (big) {
        info[0] = 4;
        pooled = 1;
        uint32_t sample = apx_hybrid_sample((uint32_t)D, eps);
        pool = apx_hybrid_pool(k, n, eps);
        info[2] = (uint32_t)pool;
        info[3] = sample;
        if (sample >= D || pool >= n) exact = 1;
        else {
            nb = apx_blocks((uint32_t)D, sample, start, len);
            float scale = (float)D / (float)sample;
            for (size_t r = 0; r < n; ++r) {
                const float *v = rows + r * D;
                float c;
                if (metric == M_L1 || metric == M_CANB) {
                    float s = 0.0f;
                    for (uint32_t b = 0; b < nb; ++b) s = s + additive(metric, q + start[b], v + start[b], len[b]);
                    c = s * scale;
                } else if (metric == M_CHEB) {
                    c = 0.0f;
                    for (uint32_t b = 0; b < nb; ++b) c = rmax(c, chebyshev(q + start[b], v + start[b], len[b]));
                } else {
                    float num = 0.0f, den = 0.0f;
                    for (uint32_t b = 0; b < nb; ++b)
                        for (uint32_t i = start[b]; i < start[b] + len[b]; ++i) {
                            num = num + fabsf(q[i] - v[i]);
                            den = den + fabsf(q[i] + v[i]);
                        }
                    c = bray_finish(num, den);
                }
                if (coarse) coarse[r] = c;
                keys[r] = key_of(c, (uint32_t)r, 1);
            }
            qsort(keys, n, 8, cmp_u64);
        }
    } else {
        info[0] = 2;
        for (size_t r = 0; r < n; ++r) {
            float d = exact_of(metric, 0, q, rows + r * D, D); /* ip: the single-row form whatever n is */
            if (coarse) coarse[r] = d;
            keys[r] = key_of(d, (uint32_t)r, asc);
        }
        cnt = best_of(keys, n, k, asc, out_rows, out_dists);
    }

    if (exact) { /* the exact search: ip in the shard's form */
        info[4] = 1;
        for (size_t r = 0; r < n; ++r) keys[r] = key_of(exact_of(metric, batch8, q, rows + r * D, D), (uint32_t)r, asc);
        cnt = best_of(keys, n, k, asc, out_rows, out_dists);
    } else if (pooled) { /* keys[0 .. pool) is the pool, in canonical order of the coarse score: scored exactly */
        uint64_t *pk = malloc((pool ? pool : 1) * 8);
        for (size_t i = 0; i < pool; ++i) {
            uint32_t r = (uint32_t)keys[i];
            if (pool_rows) pool_rows[i] = r;
            pk[i] = key_of(exact_of(metric, 0, q, rows + (size_t)r * D, D), r, asc);
        }
        if (pool_cnt) *pool_cnt = (uint32_t)pool;
        cnt = best_of(pk, pool, k, asc, out_rows, out_dists);
        free(pk);
    }
    free(keys);
    return cnt;
}
