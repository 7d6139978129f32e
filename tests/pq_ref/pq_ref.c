/* TEST INFRASTRUCTURE (tests/test_gpu_flat_pq.py): the control flow of PQIndex::build_with_clusters, kmeans_subspace and
 * encode_vectors (src/storage/pq_mmap.rs:73-149, :577-662, :696-735) restated in C for the training cases that are too slow in
 * Python.  Every distance is the oracle's exported single-pair kernel, handed in as a function pointer (lo_l2_single /
 * lo_ip_single / lo_compute_distance); the random draws come from the test's own SmallRng restatement.  Build with
 * -ffp-contract=off: the sums and products here are separate f32 operations, as in Rust. */
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <float.h>

typedef float (*pair_fn)(const float *, const float *, size_t);
typedef float (*dist_fn)(const float *, const float *, size_t, int);

/* kmeans_subspace for every subspace over `train` (train_n x dim), centroids in cb[M][K][ss] */
void pqr_train(const float *train, size_t train_n, size_t dim, size_t M, size_t K, size_t iters, const uint32_t *idx,
               const uint32_t *chosen, pair_fn l2, float *cb) {
    size_t ss = dim / M;
    float *sub = malloc(sizeof(float) * train_n * ss), *nc = malloc(sizeof(float) * K * ss);
    uint32_t *asg = malloc(sizeof(uint32_t) * train_n), *cnt = malloc(sizeof(uint32_t) * K);
    for (size_t m = 0; m < M; ++m) {
        float *c = cb + m * K * ss;
        for (size_t i = 0; i < train_n; ++i) memcpy(sub + i * ss, train + i * dim + m * ss, ss * sizeof(float));
        size_t ch = chosen[m];
        for (size_t j = 0; j < ch; ++j) memcpy(c + j * ss, sub + (size_t)idx[m * K + j] * ss, ss * sizeof(float));
        for (size_t j = ch; j < K; ++j)
            for (size_t d = 0; d < ss; ++d) c[j * ss + d] = c[(j - 1) * ss + d] * (1.0f + 0.001f * (float)d);
        memset(asg, 0, sizeof(uint32_t) * train_n);
        for (size_t it = 0; it < (iters ? iters : 1); ++it) {
            int changed = 0;
            for (size_t i = 0; i < train_n; ++i) {
                uint32_t bc = 0;
                float bd = FLT_MAX;
                for (size_t j = 0; j < K; ++j) {
                    float d = l2(sub + i * ss, c + j * ss, ss);
                    if (d < bd) { bd = d; bc = (uint32_t)j; }
                }
                if (asg[i] != bc) { asg[i] = bc; changed = 1; }
            }
            if (!changed) break;
            memset(cnt, 0, sizeof(uint32_t) * K);
            memset(nc, 0, sizeof(float) * K * ss);
            for (size_t i = 0; i < train_n; ++i) {
                cnt[asg[i]] += 1;
                for (size_t d = 0; d < ss; ++d) nc[asg[i] * ss + d] += sub[i * ss + d];
            }
            size_t src = 0;
            for (size_t j = 0; j < K; ++j) if (cnt[j] >= cnt[src]) src = j;   /* max_by_key: the last maximum */
            for (size_t j = 0; j < K; ++j) {
                if (cnt[j] > 0) {
                    float inv = 1.0f / (float)cnt[j];
                    for (size_t d = 0; d < ss; ++d) nc[j * ss + d] *= inv;
                } else {
                    for (size_t d = 0; d < ss; ++d) nc[j * ss + d] = nc[src * ss + d] * (1.0f + 0.01f * ((float)(d % 2) - 0.5f));
                }
            }
            memcpy(c, nc, sizeof(float) * K * ss);
        }
    }
    free(sub); free(nc); free(asg); free(cnt);
}

/* encode_vectors for the rows listed in `rows` (n_rows of them) */
void pqr_encode(const float *data, size_t dim, const uint64_t *rows, size_t n_rows, size_t M, size_t K, const float *cb, pair_fn l2,
                uint8_t *codes) {
    size_t ss = dim / M;
    for (size_t r = 0; r < n_rows; ++r)
        for (size_t m = 0; m < M; ++m) {
            uint32_t bc = 0;
            float bd = FLT_MAX;
            for (size_t j = 0; j < K; ++j) {
                float d = l2(data + rows[r] * dim + m * ss, cb + (m * K + j) * ss, ss);
                if (d < bd) { bd = d; bc = (uint32_t)j; }
            }
            codes[r * M + m] = (uint8_t)bc;
        }
}

/* build_lut for nq queries: lut[q][m][c] with `fn` (lo_ip_single or lo_l2_single) */
void pqr_lut(const float *queries, size_t nq, size_t dim, size_t M, size_t K, const float *cb, pair_fn fn, float *lut) {
    size_t ss = dim / M;
    for (size_t q = 0; q < nq; ++q)
        for (size_t m = 0; m < M; ++m)
            for (size_t c = 0; c < K; ++c) lut[(q * M + m) * K + c] = fn(queries + q * dim + m * ss, cb + (m * K + c) * ss, ss);
}

/* compute_distance_f32 of one query against the listed rows */
void pqr_dists(const float *query, const float *data, size_t dim, const uint64_t *rows, size_t n_rows, int metric, dist_fn fn,
               float *out) {
    for (size_t r = 0; r < n_rows; ++r) out[r] = fn(query, data + rows[r] * dim, dim, metric);
}
