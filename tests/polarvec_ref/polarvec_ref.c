/* TEST INFRASTRUCTURE (tests/polarvec_common.py): PolarVecIndex's fit, encode, bit packing, query tables and table score
 * (src/storage/polarvec_mmap.rs:137-208, :310-332, :703-852, :926-1135, :1202-1207) stated from scratch in plain sequential C.  The sign
 * words come from the test's own SmallRng restatement, the exact distances from the oracle's exported single-pair kernel, handed in as a
 * function pointer.  Build with -O2 -ffp-contract=off -fno-fast-math: every sum and product here is a separate f32 operation, as in Rust. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef float (*dist_fn)(const float *, const float *, size_t, int);
enum { IP = 0, L2 = 1, COS = 2 };

static size_t next_pow2(size_t d) {
    size_t p = 1;
    while (p < d) p <<= 1;
    return p;
}
static size_t bytes_per_vec(size_t P, size_t bits) { return (P * bits + 7) / 8; }

/* pad to P, negate where the sign bit is set (a missing word negates nothing), unnormalised FWHT */
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

/* Rust's f32::max / f32::min: the operand that is not a NaN */
static float rmax(float a, float b) { return isnan(a) ? b : (isnan(b) ? a : (a > b ? a : b)); }
static float rmin(float a, float b) { return isnan(a) ? b : (isnan(b) ? a : (a < b ? a : b)); }

float plr_raw_code(float val, float mn, float sc) { return (val - mn) / sc; }

/* round half away from zero, clamp to [0, levels - 1], a NaN is 0 */
unsigned plr_code(float val, float mn, float sc, unsigned levels) {
    float r = rmin(rmax(roundf(plr_raw_code(val, mn, sc)), 0.0f), (float)(levels - 1));
    return (unsigned)r;
}

/* the LSB-first code stream: dimension d at bits [d * bits, (d + 1) * bits) of the row */
void plr_pack(uint8_t *row, size_t d, unsigned code, size_t bits) {
    for (size_t i = 0; i < bits; ++i) {
        size_t bit = d * bits + i;
        uint8_t m = (uint8_t)(1u << (bit % 8));
        if ((code >> i) & 1u) row[bit / 8] |= m;
        else row[bit / 8] &= (uint8_t)~m;
    }
}
unsigned plr_unpack(const uint8_t *row, size_t d, size_t bits) {
    unsigned code = 0;
    for (size_t i = 0; i < bits; ++i) {
        size_t bit = d * bits + i;
        code |= (unsigned)((row[bit / 8] >> (bit % 8)) & 1u) << i;
    }
    return code;
}

/* dim_mins[P], dim_scales[P] from up to 50,000 sample rows at a fixed stride */
void plr_fit(const float *data, size_t n, size_t dim, size_t bits, const uint64_t *sign, size_t n_sign, float *dim_mins, float *dim_scales) {
    size_t P = next_pow2(dim), levels = (size_t)1 << bits;
    size_t n_sample = n < 50000 ? n : 50000, stride = n <= 50000 ? 1 : n / n_sample;
    float *buf = malloc(sizeof(float) * P), *mn = malloc(sizeof(float) * P), *mx = malloc(sizeof(float) * P);
    for (size_t d = 0; d < P; ++d) { mn[d] = INFINITY; mx[d] = -INFINITY; }
    for (size_t si = 0; si < n_sample; ++si) {
        rotate(data + si * stride * dim, dim, P, sign, n_sign, buf);
        for (size_t d = 0; d < P; ++d) {
            if (buf[d] < mn[d]) mn[d] = buf[d];
            if (buf[d] > mx[d]) mx[d] = buf[d];
        }
    }
    const float margin = 0.05f;
    for (size_t d = 0; d < P; ++d) {
        float range = mx[d] - mn[d];
        if (range > 1e-8f) {
            dim_mins[d] = mn[d] - margin * range;
            dim_scales[d] = range * (1.0f + 2.0f * margin) / (float)(levels - 1);
        } else {
            dim_mins[d] = mn[d];
            dim_scales[d] = 1.0f;
        }
    }
    free(buf); free(mn); free(mx);
}

/* codes[n][bytes_per_vec]; residual_sq[n] and inv_v_hat_norms[n] where not NULL */
void plr_encode(const float *data, size_t n, size_t dim, size_t bits, const uint64_t *sign, size_t n_sign, const float *dim_mins,
                const float *dim_scales, uint8_t *codes, float *residual_sq, float *inv_v_hat_norms) {
    size_t P = next_pow2(dim), bpv = bytes_per_vec(P, bits);
    unsigned levels = 1u << bits;
    float *buf = malloc(sizeof(float) * P);
    memset(codes, 0, n * bpv);
    for (size_t r = 0; r < n; ++r) {
        rotate(data + r * dim, dim, P, sign, n_sign, buf);
        float res = 0.0f, vh = 0.0f;
        for (size_t d = 0; d < P; ++d) {
            unsigned code = plr_code(buf[d], dim_mins[d], dim_scales[d], levels);
            plr_pack(codes + r * bpv, d, code, bits);
            float v_hat = dim_mins[d] + (float)code * dim_scales[d];
            float diff = buf[d] - v_hat;
            res += diff * diff;
            vh += v_hat * v_hat;
        }
        if (residual_sq) residual_sq[r] = res;
        if (inv_v_hat_norms) inv_v_hat_norms[r] = 1.0f / rmax(sqrtf(vh), 1e-12f);
    }
    free(buf);
}

/* lut[P][levels] of one query */
void plr_query(const float *q, size_t dim, size_t bits, int metric, const uint64_t *sign, size_t n_sign, const float *dim_mins,
               const float *dim_scales, float *lut) {
    size_t P = next_pow2(dim), levels = (size_t)1 << bits;
    float *x = malloc(sizeof(float) * dim), *buf = malloc(sizeof(float) * P);
    memcpy(x, q, sizeof(float) * dim);
    if (metric == COS) {
        float s = 0.0f;
        for (size_t d = 0; d < dim; ++d) s += q[d] * q[d];
        float qn = rmax(sqrtf(s), 1e-12f);
        for (size_t d = 0; d < dim; ++d) x[d] = q[d] / qn;
    }
    rotate(x, dim, P, sign, n_sign, buf);
    for (size_t d = 0; d < P; ++d)
        for (size_t c = 0; c < levels; ++c) {
            float v = dim_mins[d] + (float)c * dim_scales[d];
            float e;
            if (metric == IP) e = buf[d] * v;
            else if (metric == COS) e = -(buf[d] * v);
            else { float diff = buf[d] - v; e = diff * diff; }
            lut[d * levels + c] = e;
        }
    free(x); free(buf);
}

/* four accumulators over a[0 .. len): a[i] to s[i % 4] for i < (len / 4) * 4, the rest to s0; ((s0 + s1) + s2) + s3 */
static float four_acc(const float *a, size_t len) {
    float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    size_t full = len / 4 * 4;
    for (size_t i = 0; i < full; ++i) s[i % 4] += a[i];
    for (size_t i = full; i < len; ++i) s[0] += a[i];
    return ((s[0] + s[1]) + s[2]) + s[3];
}

/* the table score of every row, then + corr[row] and * mult[row] where not NULL */
void plr_scores(const uint8_t *codes, size_t n, size_t dim, size_t bits, const float *lut, const float *corr, const float *mult, float *out) {
    size_t P = next_pow2(dim), levels = (size_t)1 << bits, bpv = bytes_per_vec(P, bits);
    float *bl = NULL, *term = malloc(sizeof(float) * (P > bpv ? P : bpv));
    if (bits == 4) {   /* the byte table: low nibble = the even dimension */
        bl = malloc(sizeof(float) * bpv * 256);
        for (size_t b = 0; b < bpv; ++b)
            for (size_t v = 0; v < 256; ++v) {
                float s = lut[(2 * b) * 16 + (v & 15)];
                if (2 * b + 1 < P) s += lut[(2 * b + 1) * 16 + (v >> 4)];
                bl[b * 256 + v] = s;
            }
    }
    for (size_t r = 0; r < n; ++r) {
        const uint8_t *row = codes + r * bpv;
        float score;
        if (bits == 4) {
            for (size_t b = 0; b < bpv; ++b) term[b] = bl[b * 256 + row[b]];
            score = four_acc(term, bpv);
        } else if (bits == 8) {
            for (size_t b = 0; b < bpv; ++b) term[b] = lut[b * 256 + row[b]];
            score = four_acc(term, bpv);
        } else if (bits == 3) {   /* whole groups of 8 dimensions only: dimension j of a group to s[j % 4], which is s[d % 4] */
            size_t dims = P / 8 * 8;
            float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            for (size_t d = 0; d < dims; ++d) s[d % 4] += lut[d * levels + plr_unpack(row, d, bits)];
            score = ((s[0] + s[1]) + s[2]) + s[3];
        } else {
            score = 0.0f;
            for (size_t d = 0; d < P; ++d) score += lut[d * levels + plr_unpack(row, d, bits)];
        }
        if (corr) score += corr[r];
        if (mult) score *= mult[r];
        out[r] = score;
    }
    free(bl); free(term);
}

/* compute_distance_f32 of one query against the listed rows */
void plr_dists(const float *query, const float *data, size_t dim, const uint64_t *rows, size_t n_rows, int metric, dist_fn fn, float *out) {
    for (size_t r = 0; r < n_rows; ++r) out[r] = fn(query, data + rows[r] * dim, dim, metric);
}
