"""Shared by the tests of the PREDICTED plan: the helpers of tests/test_gpu_predict.py, a numpy model of the SQ8 quantiser and
of the threshold the prep kernel predicts, the restatement of the coarse scores a predicted stage compares with that threshold, and the
generators of tests/test_gpu_predict_verify.py (tests/test_predict_verify_design.py checks them without a GPU).

Everything here that models the device (`sq8_fit_model`, `model_threshold`, `model_coarse`) describes INPUTS — how many rows a threshold
admits, where a planted row lands — and is never the expectation of a search: ids and distances are compared with the CPU oracle only.
"""
import math
import os

import numpy as np

f32 = np.float32

PLAN_SAMPLED, PLAN_THR_ONLY, PLAN_I8C = 1, 2, 4
PLAN_SQ7, PLAN_PREDICT = 1 << 26, 1 << 28
CAP = 16384              # keys per query the candidate buffer holds (the default plan)
KEEP_MAX = CAP // 2      # more survivors than this take the compaction exit of select_body (sa.keep_max = w.cap / 2)
PRED_MISS, PRED_NONE = 2, 4      # bits of a query's overflow word beside the overflow bit 1 (kernels.h)
PREDICT_C_DEFAULT = 40   # LYNSE_HIP_PREDICT_C when unset: the keys per query the threshold aims at, in units of k


class knobs:
    """LYNSE_HIP_PREDICT / LYNSE_HIP_SQ7 / LYNSE_HIP_PREDICT_C for the duration of a block (None: unset)."""

    def __init__(self, predict, sq7=0, c=None):
        self.want = {"LYNSE_HIP_PREDICT": predict, "LYNSE_HIP_SQ7": sq7, "LYNSE_HIP_PREDICT_C": c}

    def __enter__(self):
        self.old = {k: os.environ.pop(k, None) for k in self.want}
        for k, v in self.want.items():
            if v is not None:
                os.environ[k] = str(v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def search(idx, queries, k, metric, predict, sq7=0, c=None):
    """One profiled blocking batch -> (rows, dists, counts, profile)."""
    with knobs(predict, sq7, c):
        idx.profile_enable(True)
        idx.profile_get(reset=True)
        r, d, cn = idx.search_batch_arrays(queries, k, metric)
        return r, d, cn, idx.profile_get(reset=True)


def stages(p):
    return (int(p["last_plan"]) >> 8) & 0xff


def assert_exact(want, rows, dists, counts, tag):
    for qi, (e_ids, e_d) in enumerate(want):
        c = int(counts[qi])
        assert c == len(e_ids), (tag, qi, c, len(e_ids))
        assert np.array_equal(dists[qi, :c].view(np.uint32), e_d.view(np.uint32)), (tag, qi, dists[qi, :c], e_d)
        assert np.array_equal(rows[qi, :c].astype(np.uint64), e_ids.astype(np.uint64)), (tag, qi, rows[qi, :c], e_ids)


def assert_same(a, b, tag):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and np.array_equal(a[2], b[2]), tag


def build(L, data):
    idx = L.FlatIndex(None, data.shape[1])
    idx.write(data)
    idx.finalize()
    return idx


def assert_predicted(p, nq, tag):
    lp = int(p["last_plan"])
    assert lp & PLAN_PREDICT and lp & PLAN_I8C and not lp & (PLAN_SAMPLED | PLAN_THR_ONLY), (tag, hex(lp))
    assert stages(p) == 1 and p["scan_launches"] == 1 and ((lp >> 16) & 0xff) == 0x81, (tag, p)
    assert p["fallback_queries"] == 0 and p["predicted_queries"] == nq and p["predict_miss_queries"] == 0, (tag, p)


def admitted(idx, data, queries, k, metric, sq7=0, c=None):
    """Rows per query whose exact score reaches the predicted threshold (numpy, f32 matmul in blocks; cosine: similarity - 1)."""
    with knobs(1, sq7, c):
        dbg = idx.predict_debug(queries, k, metric)
    q = queries.astype(f32)
    if metric == "cosine":
        q = q / np.linalg.norm(q.astype(np.float64), axis=1, keepdims=True).astype(f32)
    cnt = np.zeros(len(q), np.int64)
    for r0 in range(0, len(data), 65536):
        blk = data[r0:r0 + 65536]
        if metric == "cosine":
            blk = blk / np.maximum(np.linalg.norm(blk, axis=1, keepdims=True), f32(1e-30))
        s = q @ blk.T - (f32(1.0) if metric == "cosine" else f32(0.0))
        cnt += (s >= dbg["thr"][:, None]).sum(axis=1)
    return cnt, dbg


def check_inputs(idx, data, queries, k, metric, sq7=0):
    """Before relying on "no fallback": the predicted threshold admits comfortably >= k and <= cap rows for every query of the set
    (a factor 3 either way stands in for the int8 margin, which moves a row's coarse score by a fraction of the threshold's distance
    to the k-th best)."""
    cnt, dbg = admitted(idx, data, queries, k, metric, sq7)
    assert cnt.min() >= 3 * k and cnt.max() <= CAP // 3, (metric, k, int(cnt.min()), int(cnt.max()))
    return cnt, dbg


def perturbed(rng, data, nq, eps, return_rows=False):
    rows = np.sort(rng.choice(len(data), nq, replace=False))
    q = (data[rows] + eps * rng.standard_normal((nq, data.shape[1])).astype(f32)).astype(f32)
    return (q, rows) if return_rows else q


def clustered(rng, n, dim, blocks):
    """Clusters on disjoint coordinate blocks: a row of cluster j is 1 + noise on block j and noise elsewhere — the columns of different
    blocks are NEGATIVELY correlated, which the diagonal model does not know."""
    data = (0.1 * rng.standard_normal((n, dim))).astype(f32)
    w = dim // blocks
    lab = rng.integers(0, blocks, n)
    for j in range(blocks):
        data[lab == j, j * w:(j + 1) * w] += f32(1.0)
    return data


def between_clusters(rng, nq, dim):
    return (1.0 + 0.02 * rng.standard_normal((nq, dim))).astype(f32)      # equal weight on every cluster's block


def planted_tail(rng, n, dim):
    """Gaussian rows with one direction q0 whose score distribution is cut: every row above 1.2 sigma along q0 but five is pushed below it,
    the five are moved far out with distinct scores.  -> (data, q0, the five rows)."""
    data = rng.standard_normal((n, dim)).astype(f32)
    q0 = rng.standard_normal(dim).astype(f32)
    qn = q0.astype(np.float64) / np.linalg.norm(q0.astype(np.float64))
    s = data.astype(np.float64) @ qn                                         # unit-variance scores along q0
    high = np.flatnonzero(s > 1.2)
    keep = rng.choice(high, 5, replace=False)
    push = np.setdiff1d(high, keep)
    data[push] -= np.outer(s[push] - rng.uniform(0.0, 1.2, len(push)), qn).astype(f32)
    data[keep] += np.outer(4.0 - s[keep] + 0.1 * np.arange(5), qn).astype(f32)      # the planted five: far out, distinct scores
    return data, q0, keep


# ---- the quantiser and the predicted threshold in numpy (inputs only; the plain SQ8 IP form, LYNSE_HIP_SQ7=0)
def sq8_fit_model(data):
    """k_sq8_minmax / k_sq8_scales: mins = the column minima, scales = fl(255 / fl(max - min)) (0 for a constant column)."""
    mn, mx = data.min(axis=0).astype(f32), data.max(axis=0).astype(f32)
    rng_ = (mx - mn).astype(f32)
    with np.errstate(divide="ignore"):
        scales = np.where(rng_ > f32(1e-30), f32(255.0) / rng_, f32(0.0)).astype(f32)
    return mn, scales


def sq8_codes(data, mins, scales):
    """The CENTRED codes (code - 128) as f32 integers, the f32 operations of sq8_code: round half away from zero of fl(fl(v - min) * scale)
    (x >= 0 and x - floor(x) is exact), clipped to 0..255.  Restated as tests/test_gpu_predict.py restates them against mu / var."""
    out = np.empty(data.shape, f32)
    for r0 in range(0, len(data), 32768):
        x = (data[r0:r0 + 32768] - mins) * scales
        fl = np.floor(x)
        out[r0:r0 + 32768] = np.clip(fl + (x - fl >= f32(0.5)), 0, 255) - f32(128.0)
    return out


def code_stats(codes):
    n = len(codes)
    mu = codes.sum(axis=0, dtype=np.float64) / n
    var = np.maximum((codes.astype(np.float64) ** 2).sum(axis=0) / n - mu * mu, 0.0)
    return mu, var


def z_numpy(n, c):
    """Bisection of 0.5 erfc(z / sqrt 2) = c / n over [0, 40] (predict.h); 0 when the target is half the rows or more."""
    if n == 0 or not c > 0 or c >= 0.5 * n:
        return 0.0
    p, lo, hi = c / n, 0.0, 40.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if 0.5 * math.erfc(mid * 0.7071067811865476) > p else (lo, mid)
    return 0.5 * (lo + hi)


def _weights(queries, mins, scales):
    q = queries.astype(np.float64)
    w = np.divide(q, scales.astype(np.float64), out=np.zeros_like(q), where=scales > 0)
    return w, q @ mins.astype(np.float64) + 128.0 * w.sum(axis=1)


def model_threshold(queries, mins, scales, mu, var, n, c, k):
    """thr = B_q + (w . mu + z sqrt(w^2 . var)) with the UNQUANTISED query, w = q / scale: the device's threshold up to the rounding of
    the query's int8 image."""
    w, b = _weights(queries, mins, scales)
    return b + w @ mu + z_numpy(n, c * k) * np.sqrt((w * w) @ var)


def model_coarse(queries, mins, scales, codes):
    """Dequantised score of every (query, row), f64: B_q + w . c — the coarse score up to the rounding of the query's int8 image."""
    w, b = _weights(queries, mins, scales)
    out = np.empty((len(queries), len(codes)), np.float64)
    for r0 in range(0, len(codes), 32768):
        out[:, r0:r0 + 32768] = w @ codes[r0:r0 + 32768].astype(np.float64).T
    return out + b[:, None]


def restated_coarse(idx, data, dbg):
    """The coarse score the predicted stage compares with thr for every (query, row), f64: bq + sq * (u . c) with the centred codes c
    restated from idx.sq8_params() and u, bq, sq of idx.predict_debug (the integer dot products are exact in f32: |u . c| <= 127 * 128 *
    cols < 2^24 for cols <= 1024).  Plain SQ8 IP form only.  Also delta[q] = 4e-6 (|bq| + 127 sq sum |u|): the prep kernel's own slack
    is 1e-6 of a quantity this bounds, and the factor 4 covers the f32 rounding of the scan's fl(bq + fl(sq * fl(dot))).  A row with
    coarse >= thr + delta was surely emitted, one with coarse < thr - delta surely not; between the two the query is undetermined."""
    mins, scales = idx.sq8_params()
    cols = dbg["cols"]
    assert cols == data.shape[1] <= 1024 and dbg["u"].shape[1] == cols
    c = sq8_codes(data, mins, scales)
    u = dbg["u"].astype(f32)
    bq, sq = dbg["bq"].astype(np.float64), dbg["sq"].astype(np.float64)
    coarse = np.empty((len(u), len(c)), np.float64)
    for r0 in range(0, len(c), 32768):
        coarse[:, r0:r0 + 32768] = u @ c[r0:r0 + 32768].T
    coarse *= sq[:, None]
    coarse += bq[:, None]
    delta = 4e-6 * (np.abs(bq) + 127.0 * sq * np.abs(dbg["u"].astype(np.float64)).sum(axis=1))
    return coarse, delta


def emitted_counts(coarse, thr, delta):
    """(rows surely emitted, rows not surely left out) per query."""
    t = thr.astype(np.float64)
    return (coarse >= (t + delta)[:, None]).sum(axis=1), (coarse >= (t - delta)[:, None]).sum(axis=1)


# ---- generators
BAND_N, BAND_DIM, BAND_NQ, BAND_K, BAND_PICKS = 70_000, 256, 256, 10, 8


def band_inputs():
    """The shard family of the band cases: unit-Gaussian rows, 256 queries perturbed from rows of the shard -> (data, queries, source rows)."""
    rng = np.random.default_rng(2741)
    data = rng.standard_normal((BAND_N, BAND_DIM)).astype(f32)
    queries, src = perturbed(rng, data, BAND_NQ, 0.1, return_rows=True)
    return data, queries, src


def pick_band_queries(cnt, picks=BAND_PICKS, at_most=6):
    """The first `picks` queries with at most `at_most` rows at or above their threshold: six helper rows bring them to k .. k + 2."""
    return np.flatnonzero(np.asarray(cnt) <= at_most)[:picks]


def plant_band(rng, data, queries, thr, picks, k, mins=None, scales=None, avoid=(), victim_at=-1.0, helpers_up=0.0):
    """For each picked query q, into rows that are neither in `avoid` (the queries' source rows) nor hold a column's minimum or maximum:
    six helper rows r = 0.3 N(0, I) moved along q so that q . r = thr + 0.8 + 0.12 j (+ helpers_up), j = 0..5 — with the at most six rows
    already there, k or more keys arrive —, and one victim: the same kind of row at q . r = thr + victim_at, snapped to the quantiser's
    grid, plus 0.45 / scale_d * sign(q_d) in every dimension.  The victim still codes as the grid point, which dequantises
    0.45 sum |q_d| / scale_d (about 3 on unit-Gaussian rows) BELOW its exact score — the aligned worst case of
    tests/test_gpu_certificate.py: its exact score is in the top-k, its coarse score under the threshold.  All planted values lie inside
    the columns' ranges, so the fit does not move.  -> (planted copy, victim row per pick, helper rows per pick)."""
    assert k > 6, "six helpers must not make k keys on their own"
    if mins is None:
        mins, scales = sq8_fit_model(data)
    lo, hi = data.min(axis=0), data.max(axis=0)
    banned = np.zeros(len(data), bool)
    banned[np.asarray(avoid, np.int64)] = True
    banned[data.argmin(axis=0)] = True
    banned[data.argmax(axis=0)] = True
    rows = rng.choice(np.flatnonzero(~banned), 7 * len(picks), replace=False).reshape(len(picks), 7)
    out = data.copy()
    mn, sc = mins.astype(np.float64), scales.astype(np.float64)
    assert (sc > 0).all()
    for i, qi in enumerate(picks):
        q = queries[qi].astype(np.float64)

        def along(target):
            r = 0.3 * rng.standard_normal(len(q))
            return r + (target - q @ r) / (q @ q) * q

        for j in range(6):
            out[rows[i, j]] = along(float(thr[qi]) + 0.8 + helpers_up + 0.12 * j).astype(f32)
        r = along(float(thr[qi]) + victim_at)
        grid = np.round((r - mn) * sc) / sc + mn
        out[rows[i, 6]] = (grid + 0.45 / sc * np.sign(q)).astype(f32)
    planted = out[rows.reshape(-1)]
    assert (planted >= lo).all() and (planted <= hi).all(), "a planted value left the fitted range"
    return out, rows[:, 6].copy(), rows[:, :6].copy()


def duplicated(rng, n, dim, copies):
    """Gaussian rows with `copies` rows overwritten by one of them -> (data, the ids of the copies, ascending)."""
    data = rng.standard_normal((n, dim)).astype(f32)
    ids = np.sort(rng.choice(n, copies, replace=False))
    data[ids] = data[ids[0]]
    return data, ids


OVER_N, OVER_C = 163_840, 2000      # predict_wanted needs n >= 8 C k


def overflow_inputs():
    """Uniform rows and a target of C k = 20,000 keys per query: above the 16,384 the candidate buffer holds."""
    rng = np.random.default_rng(2743)
    data = rng.random((OVER_N, 256), dtype=f32)
    return data, perturbed(rng, data, 256, 0.03)


DUP_N, DUP_COPIES, DUP_NEAR, DUP_FAR = 100_000, 9_000, 136, 120


def duplicate_inputs():
    """9,000 equal rows among 100,000: 136 queries near the copied row see 9,000 equal coarse scores far above the threshold — more than
    KEEP_MAX survivors, fewer than CAP keys —, 120 queries perturbed from other rows see an ordinary tail.  -> (data, copy ids, queries:
    the near ones first)."""
    rng = np.random.default_rng(2746)
    data, ids = duplicated(rng, DUP_N, 256, DUP_COPIES)
    near = (data[ids[0]] + 0.1 * rng.standard_normal((DUP_NEAR, 256)).astype(f32)).astype(f32)
    base = data[ids[0]].astype(np.float64)
    along = data.astype(np.float64) @ base / np.linalg.norm(base)           # unit-variance scores along the copied row
    others = np.setdiff1d(np.flatnonzero(np.abs(along) < 2.0), ids)         # (a far query must not admit the 9,000 copies: its threshold lies near 3 sigma)
    far_rows = np.sort(rng.choice(others, DUP_FAR, replace=False))
    far = (data[far_rows] + 0.1 * rng.standard_normal((DUP_FAR, 256)).astype(f32)).astype(f32)
    return data, ids, np.vstack([near, far])
