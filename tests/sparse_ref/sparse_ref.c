/* sparse_ref.c — a plain-C restatement of the reference's sparse-vector arithmetic (src/engine.rs:6925-6965), written the way the
 * reference writes it: an ordered map for the normaliser, the two-pointer merge for the inner product.  TEST INFRASTRUCTURE: the tests
 * compile it with -O2 -ffp-contract=off -fno-fast-math and compare the library against it bit for bit. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

/* normalize_sparse_entries: (index, value) pairs in any order -> ascending indices, duplicates summed in input order from 0.0f,
 * zeros skipped, zero sums dropped.  Returns the entries written, or -1 for a non-finite value.  The map is a sorted array. */
long sr_normalize(const uint32_t *idx, const float *val, size_t n, uint32_t *o_idx, float *o_val) {
    size_t m = 0;
    for (size_t i = 0; i < n; ++i) {
        if (!isfinite(val[i])) return -1;
        if (val[i] == 0.0f) continue;
        size_t lo = 0, hi = m;
        while (lo < hi) {
            size_t mid = (lo + hi) / 2;
            if (o_idx[mid] < idx[i]) lo = mid + 1; else hi = mid;
        }
        if (lo == m || o_idx[lo] != idx[i]) { /* entry(index).or_insert(0.0) */
            memmove(o_idx + lo + 1, o_idx + lo, (m - lo) * sizeof *o_idx);
            memmove(o_val + lo + 1, o_val + lo, (m - lo) * sizeof *o_val);
            o_idx[lo] = idx[i];
            o_val[lo] = 0.0f;
            ++m;
        }
        o_val[lo] += val[i];
    }
    size_t w = 0;
    for (size_t i = 0; i < m; ++i)
        if (o_val[i] != 0.0f) {
            o_idx[w] = o_idx[i];
            o_val[w] = o_val[i];
            ++w;
        }
    return (long)w;
}

/* sparse_inner_product: both vectors normalised */
float sr_ip(const uint32_t *qi, const float *qv, size_t nq, const uint32_t *vi, const float *vv, size_t nv) {
    size_t q = 0, v = 0;
    float score = 0.0f;
    while (q < nq && v < nv) {
        if (qi[q] == vi[v]) {
            score += qv[q] * vv[v];
            ++q;
            ++v;
        } else if (qi[q] < vi[v]) {
            ++q;
        } else {
            ++v;
        }
    }
    return score;
}

/* the same pairs summed from the highest common index down: NOT the reference's order — the tests use it to show that their data
 * can tell a wrong summation order */
float sr_ip_reversed(const uint32_t *qi, const float *qv, size_t nq, const uint32_t *vi, const float *vv, size_t nv) {
    size_t q = nq, v = nv;
    float score = 0.0f;
    while (q > 0 && v > 0) {
        if (qi[q - 1] == vi[v - 1]) {
            score += qv[q - 1] * vv[v - 1];
            --q;
            --v;
        } else if (qi[q - 1] > vi[v - 1]) {
            --q;
        } else {
            --v;
        }
    }
    return score;
}

/* one query against every row of a CSR store -> out[n] */
void sr_scores(const uint32_t *qi, const float *qv, size_t nq, const uint64_t *indptr, const uint32_t *indices, const float *values,
               size_t n, int reversed, float *out) {
    for (size_t r = 0; r < n; ++r) {
        const size_t a = (size_t)indptr[r], len = (size_t)(indptr[r + 1] - indptr[r]);
        out[r] = reversed ? sr_ip_reversed(qi, qv, nq, indices + a, values + a, len) : sr_ip(qi, qv, nq, indices + a, values + a, len);
    }
}
