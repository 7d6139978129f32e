/* A restatement of the four additive distances of include/lynse_hip.h (ids 7-10), written from the contract block next to the metric
 * enum: plain C, eight explicit lanes, f32 throughout.  Compiled by the tests with -O2 -ffp-contract=off -fno-fast-math.
 *   shape: chunks = D / 8; lane g takes the elements 8 i + g in order; the lanes are reduced from lane 0 to lane 7, one after the
 *   other; the D % 8 tail elements follow one by one. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>

enum { ADD_L1 = 7, ADD_CHEBYSHEV = 8, ADD_CANBERRA = 9, ADD_BRAY_CURTIS = 10 };

/* Rust's f32::max: the operand that is not NaN */
static float rmax(float x, float y) {
    if (x != x) return y;
    if (y != y) return x;
    return x > y ? x : y;
}

static float l1(const float *a, const float *b, size_t D) {
    size_t chunks = D / 8;
    float lane[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (size_t i = 0; i < chunks; ++i)
        for (int g = 0; g < 8; ++g) lane[g] = lane[g] + fabsf(a[8 * i + g] - b[8 * i + g]);
    float sum = 0.0f;
    for (int g = 0; g < 8; ++g) sum = sum + lane[g];
    for (size_t i = chunks * 8; i < D; ++i) sum = sum + fabsf(a[i] - b[i]);
    return sum;
}

static float chebyshev(const float *a, const float *b, size_t D) {
    size_t chunks = D / 8;
    float lane[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (size_t i = 0; i < chunks; ++i)
        for (int g = 0; g < 8; ++g) {
            float d = fabsf(a[8 * i + g] - b[8 * i + g]);
            lane[g] = (lane[g] > d) ? lane[g] : d; /* d when either is NaN */
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
            float x = a[8 * i + g], y = b[8 * i + g];
            float den = fabsf(x) + fabsf(y);
            float q = fabsf(x - y) / den;
            int ordered_nonzero = (den < 0.0f) || (den > 0.0f); /* false for a NaN den */
            lane[g] = lane[g] + (ordered_nonzero ? q : 0.0f);
        }
    float sum = 0.0f;
    for (int g = 0; g < 8; ++g) sum = sum + lane[g];
    for (size_t i = chunks * 8; i < D; ++i) {
        float den = fabsf(a[i]) + fabsf(b[i]);
        if (den != 0.0f) sum = sum + fabsf(a[i] - b[i]) / den; /* true for a NaN den */
    }
    return sum;
}

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
    if (den == 0.0f) return num == 0.0f ? 0.0f : INFINITY;
    return num / den;
}

float add_dist(int metric, const float *a, const float *b, size_t D) {
    switch (metric) {
    case ADD_L1: return l1(a, b, D);
    case ADD_CHEBYSHEV: return chebyshev(a, b, D);
    case ADD_CANBERRA: return canberra(a, b, D);
    default: return bray_curtis(a, b, D);
    }
}

/* out[r] = the distance of the query q and row r of the n x D matrix */
void add_dists(int metric, const float *q, const float *rows, size_t n, size_t D, float *out) {
    for (size_t r = 0; r < n; ++r) out[r] = add_dist(metric, q, rows + r * D, D);
}
