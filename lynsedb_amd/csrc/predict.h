// predict.h — the PREDICTED first threshold of the certified int8 pass: per-column statistics of a code set and the
// normal model of the integer dot product.  The scan kernels are not involved: k_scan_qs only sees a different a.thr.
//
// For a query image u (k_i8c_prep_queries) the integer dot product over the coded rows, dot_r = sum_d u_d c_{r,d}, has over the n rows
//   mean      m_q = sum_d u_d mu_d                     mu_d      = (sum_r c_{r,d}) / n          (exact)
//   variance  v_q = sum_d u_d^2 sigma_d^2 + (cross)    sigma_d^2 = (sum_r c_{r,d}^2) / n - mu_d^2
// and the DIAGONAL model drops the cross terms.  With z from n (1 - Phi(z)) = C the threshold B_q + s_q (m_q + z sqrt(v_q)) admits about
// C rows per query when the dot products are roughly normal.  Nothing relies on that: k_select_final checks afterwards, from what the
// scan emitted, that the threshold was valid (TailArgs::pred_chk) and the host answers the chunk again on the sampled plan when not.
#pragma once
#include "common.h"

namespace lynse {

// Column sums of a code set: sums[d] += sum_r c[r][d], sums[cols + d] += sum_r c[r][d]^2 over rows [0, n) at `codes` (pitch ld bytes),
// d < cols.  64-bit integer sums: exact and order-independent (two's complement adds), so rows appended later simply add.  A thread
// owns four adjacent columns; a block walks strips of 1024 rows (|sum c^2| <= 2^24 per strip in 32 bits) and adds once at the end.
__global__ void __launch_bounds__(256) k_code_colsums(const int8_t* __restrict__ codes, uint32_t ld, uint32_t cols, uint64_t n,
                                                      unsigned long long* __restrict__ sums) {
    constexpr uint64_t STRIP = 1024;
    const uint64_t nstrips = (n + STRIP - 1) / STRIP;
    for (uint32_t c0 = threadIdx.x * 4u; c0 < cols; c0 += 1024u) {   // (ld is a multiple of 4: the word at c0 < cols lies inside the row)
        long long t1[4] = {0, 0, 0, 0}, t2[4] = {0, 0, 0, 0};
        for (uint64_t s = blockIdx.x; s < nstrips; s += gridDim.x) {
            const uint64_t r0 = s * STRIP, r1 = r0 + STRIP < n ? r0 + STRIP : n;
            int a1[4] = {0, 0, 0, 0}, a2[4] = {0, 0, 0, 0};
            const int8_t* p = codes + r0 * ld + c0;
#pragma unroll 8
            for (uint64_t r = r0; r < r1; ++r, p += ld) {
                const uint32_t wd = *reinterpret_cast<const uint32_t*>(p);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int c = (int)(int8_t)(wd >> (8 * j));
                    a1[j] += c;
                    a2[j] += c * c;
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) { t1[j] += a1[j]; t2[j] += a2[j]; }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (c0 + j < cols) {
                atomicAdd(&sums[c0 + j], (unsigned long long)t1[j]);
                atomicAdd(&sums[cols + c0 + j], (unsigned long long)t2[j]);
            }
    }
}

// ---- host side of the model (no device needed: lynse_hip_predict_z / lynse_hip_predict_threshold expose it to the tests)

// mu_d and sigma_d^2 of the columns from their exact integer sums (f64; sigma_d^2 clamped at 0)
inline void predict_col_stats(const long long* sums, uint32_t cols, uint64_t n, double* mu, double* var) {
    for (uint32_t d = 0; d < cols; ++d) {
        const double m = n ? (double)sums[d] / (double)n : 0.0;
        const double v = n ? (double)sums[cols + d] / (double)n - m * m : 0.0;
        mu[d] = m;
        var[d] = v > 0.0 ? v : 0.0;
    }
}

// z with n (1 - Phi(z)) = c, by bisection of the f64 erfc over [0, 40] (c >= n / 2: 0 — the threshold never goes below the mean)
inline double predict_z(uint64_t n, double c) {
    if (n == 0 || !(c > 0.0) || c >= 0.5 * (double)n) return 0.0;
    const double p = c / (double)n;
    double lo = 0.0, hi = 40.0;
    for (int it = 0; it < 200; ++it) {
        const double mid = 0.5 * (lo + hi);
        if (0.5 * erfc(mid * 0.7071067811865476) > p) lo = mid; else hi = mid;
    }
    return 0.5 * (lo + hi);
}

// The threshold of one query as k_i8c_prep_queries forms it: sequential f64 sums over the columns (the kernel's tree sums differ by f64
// rounding only), then ONE f32 rounding of the whole expression.
inline float predict_threshold(const int8_t* u, const double* mu, const double* var, uint32_t cols, double z, float bq, float sq,
                               double* out_m, double* out_v) {
    double m = 0.0, v = 0.0;
    for (uint32_t d = 0; d < cols; ++d) {
        const double x = (double)u[d];
        m += x * mu[d];
        v += x * x * var[d];
    }
    if (out_m) *out_m = m;
    if (out_v) *out_v = v;
    return (float)((double)bq + (double)sq * (m + z * sqrt(v)));
}

}  // namespace lynse
