/* TEST INFRASTRUCTURE (tests/test_gpu_flat_rabitq.py): RaBitQIndex's encode, query transform and binary score
 * (src/storage/rabitq_mmap.rs:101-132, :202-213, :345-407, :560-585) stated from scratch in plain sequential C.  The sign words come
 * from the test's own SmallRng restatement, the exact distances from the oracle's exported single-pair kernel, handed in as a function
 * pointer.  Build with -O2 -ffp-contract=off -fno-fast-math: every sum and product here is a separate f32 operation, as in Rust. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef float (*dist_fn)(const float *, const float *, size_t, int);

static size_t next_pow2(size_t d) {
    size_t p = 1;
    while (p < d) p <<= 1;
    return p;
}

/* pad to P, apply_signs, fwht */
static void rotate(const float *x, size_t dim, size_t P, const uint64_t *sign, size_t n_sign, float *buf) {
    for (size_t i = 0; i < P; ++i) buf[i] = i < dim ? x[i] : 0.0f;
    for (size_t i = 0; i < P; ++i)
        if (i / 64 < n_sign && ((sign[i / 64] >> (i % 64)) & 1)) buf[i] = -buf[i];
    for (size_t h = 1; h < P; h *= 2)
        for (size_t i = 0; i < P; i += 2 * h)
            for (size_t j = 0; j < h; ++j) {
                float a = buf[i + j], b = buf[i + j + h];
                buf[i + j] = a + b;
                buf[i + j + h] = a - b;
            }
}

/* codes[n][code_bytes], norms[n] */
void rbr_encode(const float *data, size_t n, size_t dim, const uint64_t *sign, size_t n_sign, uint8_t *codes, float *norms) {
    size_t P = next_pow2(dim), cb = (P + 7) / 8;
    float *buf = malloc(sizeof(float) * P);
    for (size_t r = 0; r < n; ++r) {
        const float *x = data + r * dim;
        float s = 0.0f;
        for (size_t i = 0; i < dim; ++i) s += x[i] * x[i];
        norms[r] = sqrtf(s);
        rotate(x, dim, P, sign, n_sign, buf);
        for (size_t b = 0; b < cb; ++b) {
            uint8_t v = 0;
            for (size_t bit = 0; bit < 8; ++bit) {
                size_t d = b * 8 + bit;
                if (d < P && buf[d] >= 0.0f) v |= (uint8_t)(1u << bit);
            }
            codes[r * cb + b] = v;
        }
    }
    free(buf);
}

/* lut[code_bytes][256] and total_q of one query */
void rbr_query(const float *q, size_t dim, const uint64_t *sign, size_t n_sign, float *lut, float *total) {
    size_t P = next_pow2(dim), cb = (P + 7) / 8;
    float *buf = malloc(sizeof(float) * P);
    rotate(q, dim, P, sign, n_sign, buf);
    float t = 0.0f;
    for (size_t i = 0; i < P; ++i) t += buf[i];
    *total = t;
    for (size_t b = 0; b < cb; ++b)
        for (unsigned v = 0; v < 256; ++v) {
            float s = 0.0f;
            for (size_t bit = 0; bit < 8; ++bit)
                if (((v >> bit) & 1u) && b * 8 + bit < P) s += buf[b * 8 + bit];
            lut[b * 256 + v] = s;
        }
    free(buf);
}

/* compute_binary_score of every row */
void rbr_scores(const uint8_t *codes, const float *norms, size_t n, size_t dim, const float *lut, float total, int ascending, float *out) {
    size_t P = next_pow2(dim), cb = (P + 7) / 8;
    for (size_t r = 0; r < n; ++r) {
        float sum_set = 0.0f;
        for (size_t b = 0; b < cb; ++b) sum_set += lut[b * 256 + codes[r * cb + b]];
        float ip_raw = 2.0f * sum_set - total;
        float norm = norms[r];
        out[r] = ascending ? norm * norm - 2.0f * ip_raw * norm / (float)P : ip_raw * norm;
    }
}

/* compute_distance_f32 of one query against the listed rows */
void rbr_dists(const float *query, const float *data, size_t dim, const uint64_t *rows, size_t n_rows, int metric, dist_fn fn, float *out) {
    for (size_t r = 0; r < n_rows; ++r) out[r] = fn(query, data + rows[r] * dim, dim, metric);
}
