"""The model of the predicted first threshold (csrc/predict.h) restated in numpy and checked against the library's host
functions — no device involved: z from n (1 - Phi(z)) = C, mu_d / sigma_d^2 from exact integer column sums, and
thr = fl(B_q + s_q (m_q + z sqrt(v_q))) with m_q = sum u_d mu_d, v_q = sum u_d^2 sigma_d^2.  Tolerances are f64 rounding only.
"""
import ctypes as C
import math

import numpy as np

from lynsedb_amd import _lib

lib = _lib.lib


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def z_numpy(n, c):
    """Bisection of 0.5 erfc(z / sqrt 2) = c / n over [0, 40]; 0 when the target is half the rows or more."""
    if n == 0 or not c > 0 or c >= 0.5 * n:
        return 0.0
    p, lo, hi = c / n, 0.0, 40.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if 0.5 * math.erfc(mid * 0.7071067811865476) > p:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def lib_z(n, c):
    z = C.c_double(-1.0)
    assert lib.lynse_hip_predict_z(n, float(c), C.byref(z)) == 0
    return z.value


def test_z_solves_the_tail_equation():
    for n, c in [(10_000_000, 400), (10_000_000, 160), (10_000_000, 1000), (1_250_000, 400), (70_000, 40), (70_000, 1280), (327_680, 400)]:
        z = lib_z(n, c)
        assert abs(z - z_numpy(n, c)) <= 1e-12 * max(1.0, z), (n, c, z)
        assert abs(n * 0.5 * math.erfc(z / math.sqrt(2.0)) - c) <= 1e-6 * c, (n, c, z)      # it IS the solution, not only the same number
    assert 3.9 < lib_z(10_000_000, 400) < 4.0                                                 # 10M rows, k = 10: 1 - Phi(3.9) = 4.8e-5 > 4e-5 > 3.2e-5 = 1 - Phi(4.0)
    assert lib_z(100, 50) == 0.0 and lib_z(100, 80) == 0.0 and lib_z(0, 1) == 0.0             # never below the mean


def test_column_statistics_from_exact_sums():
    rng = np.random.default_rng(2701)
    n, cols = 5000, 300
    codes = rng.integers(-128, 128, (n, cols)).astype(np.int64)
    codes[:, 7] = 37                                                                          # a constant column: variance exactly 0
    sums = np.concatenate([codes.sum(axis=0), (codes * codes).sum(axis=0)]).astype(np.int64)
    mu, var = np.zeros(cols), np.zeros(cols)
    assert lib.lynse_hip_predict_col_stats(ptr(sums), cols, n, ptr(mu), ptr(var)) == 0
    mu_np = sums[:cols] / n
    var_np = np.maximum(sums[cols:] / n - mu_np * mu_np, 0.0)
    assert np.array_equal(mu, mu_np) and np.array_equal(var, var_np)                          # the same two f64 operations
    assert var[7] == 0.0 and mu[7] == 37.0
    assert np.allclose(var, codes.var(axis=0), rtol=1e-9, atol=1e-6)
    # sums far past 2^31: 10M rows of the extreme codes
    big = np.array([127 * 10_000_000, -128 * 10_000_000, 127 * 127 * 10_000_000, 128 * 128 * 10_000_000], np.int64)
    mu2, var2 = np.zeros(2), np.zeros(2)
    assert lib.lynse_hip_predict_col_stats(ptr(big), 2, 10_000_000, ptr(mu2), ptr(var2)) == 0
    assert mu2.tolist() == [127.0, -128.0] and var2.tolist() == [0.0, 0.0]


def test_threshold_of_an_image():
    rng = np.random.default_rng(2702)
    cols = 768
    mu = rng.uniform(-100, 100, cols)
    var = rng.uniform(0, 4000, cols)
    for z, bq, sq in [(4.1, 12.5, 3.0e-4), (2.5, -1.0, 1.0e-5), (0.0, 0.0, 1.0)]:
        u = rng.integers(-127, 128, cols).astype(np.int8)
        m, v, thr = C.c_double(0), C.c_double(0), C.c_float(0)
        assert lib.lynse_hip_predict_threshold(ptr(u), ptr(mu), ptr(var), cols, z, bq, sq, C.byref(m), C.byref(v), C.byref(thr)) == 0
        ud = u.astype(np.float64)
        m_np, v_np = float(np.dot(ud, mu)), float(np.dot(ud * ud, var))
        assert abs(m.value - m_np) <= 1e-12 * np.dot(np.abs(ud), np.abs(mu)) and abs(v.value - v_np) <= 1e-12 * v_np
        want = np.float64(np.float32(bq)) + np.float64(np.float32(sq)) * (m.value + z * math.sqrt(v.value))
        assert thr.value == float(np.float32(want)), (thr.value, want)                       # one f32 rounding of the f64 expression
