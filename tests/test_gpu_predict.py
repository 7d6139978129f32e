"""`-m gpu` tests of the PREDICTED plan of the certified int8 pass (`LYNSE_HIP_PREDICT` = 1 / 0 / unset: wherever eligible /
never / auto from 4M rows): prep -> one threshold stage over every row on a threshold predicted from the column statistics of the codes
-> k_select_final, which verifies it.  The plan only ever changes speed: every case goes through the C-ABI and is compared, ids and f32
distance bits, with the CPU oracle and with the same handle answered with LYNSE_HIP_PREDICT=0; `last_plan` bit 28 tells which plan ran.
"""
import math

import numpy as np
import pytest

import oracle as O
from conftest import oracle_for_every_query
from predict_common import (CAP, PLAN_I8C, PLAN_PREDICT, PLAN_SAMPLED, PLAN_SQ7, PLAN_THR_ONLY, admitted, assert_exact, assert_predicted,  # noqa: F401
                            assert_same, between_clusters, build, check_inputs, clustered, knobs, perturbed, planted_tail, search, stages)

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def L():
    import lynsedb_amd as L_

    assert L_._lib.device_count() >= 1
    return L_


# ---- parity and plan: one shard and one oracle answer per (distribution, size, width), shared by the batch sizes
CASES = {
    # name: (rows kind, n, dim, metric, k, seed)
    "uniform-327680x768-ip-k10": ("uniform", 327_680, 768, "ip", 10, 2711),
    "gauss-327680x256-ip-k32": ("gauss", 327_680, 256, "ip", 32, 2712),
    "gauss-70000x768-cos-k1": ("gauss", 70_000, 768, "cosine", 1, 2713),
    "uniform-70001x256-ip-k10": ("uniform", 70_001, 256, "ip", 10, 2714),           # ragged: n is no multiple of 64
    "gauss-70001x256-cos-k10": ("gauss", 70_001, 256, "cosine", 10, 2717),          # (cosine over uniform rows: a miss case below)
    "gauss-70000x256-ip-k10": ("gauss", 70_000, 256, "ip", 10, 2715),
    "uniform-70000x768-ip-k32": ("uniform", 70_000, 768, "ip", 32, 2716),
}
_shards = {}


def shard(L, oracle, name):
    if name not in _shards:
        kind, n, dim, metric, k, seed = CASES[name]
        rng = np.random.default_rng(seed)
        data = rng.random((n, dim), dtype=f32) if kind == "uniform" else rng.standard_normal((n, dim)).astype(f32)
        queries = perturbed(rng, data, 256, 0.03 if kind == "uniform" else 0.1)
        om = O.IP if metric == "ip" else O.COS
        want = oracle_for_every_query(lambda qi: oracle.canonical_topk(queries[qi], data, k, om), 256)
        _shards[name] = (build(L, data), data, queries, want, metric, k)
    return _shards[name]


@pytest.mark.parametrize("nq", [256, 200, 130])
@pytest.mark.parametrize("name", list(CASES))
def test_parity_with_the_oracle_and_with_the_sampled_plan(L, oracle, name, nq):
    idx, data, queries, want, metric, k = shard(L, oracle, name)
    q = queries[:nq]
    cnt, dbg = check_inputs(idx, data, q, k, metric)
    rp = search(idx, q, k, metric, 1)
    print(f"{name} nq={nq}: z={dbg['z']:.3f}, rows at or above the threshold {int(cnt.min())}..{int(cnt.max())} (target {40 * k}), rescored per query {rp[3]['pool_entries'] / nq:.1f}")
    assert_predicted(rp[3], nq, name)
    assert_exact(want[:nq], *rp[:3], (name, nq))
    r0 = search(idx, q, k, metric, 0)
    assert not int(r0[3]["last_plan"]) & PLAN_PREDICT and int(r0[3]["last_plan"]) & PLAN_SAMPLED and r0[3]["predicted_queries"] == 0, r0[3]
    assert_same(rp, r0, (name, nq))
    assert idx.predict_state()["predict_strikes"] == 0


def test_sq7_codes_and_auto_below_its_start(L, oracle):
    """The SQ7 copy has statistics of its own (uncentred codes); under auto a shard this small keeps the sampled plan; fewer than 129
    queries, k = 33, squared L2 and a subset filter keep their plans under the forced knob."""
    idx, data, queries, want, metric, k = shard(L, oracle, "uniform-327680x768-ip-k10")
    check_inputs(idx, data, queries, k, metric, sq7=1)
    r7 = search(idx, queries, k, metric, 1, sq7=1)
    assert int(r7[3]["last_plan"]) & PLAN_SQ7, r7[3]
    assert_predicted(r7[3], 256, "sq7")
    assert_exact(want, *r7[:3], "sq7")
    assert idx.predict_state()["stats_rows_sq7"] == len(data) and idx.predict_state()["stats_rows_sq8"] == len(data)
    r_auto = search(idx, queries, k, metric, None)
    assert not int(r_auto[3]["last_plan"]) & PLAN_PREDICT and int(r_auto[3]["last_plan"]) & PLAN_SAMPLED, r_auto[3]
    assert_same(r_auto, r7, "auto")
    for q, kk, m in [(queries[:128], k, "ip"), (queries, 33, "ip"), (queries, k, "l2")]:
        r = search(idx, q, kk, m, 1)
        assert not int(r[3]["last_plan"]) & PLAN_PREDICT and r[3]["predicted_queries"] == 0, (len(q), kk, m, r[3])
    with knobs(1):
        idx.profile_enable(True)
        idx.profile_get(reset=True)
        idx.search_filtered_batch_arrays(queries, k, "ip", np.arange(0, len(data), 2, dtype=np.uint64))
        assert idx.profile_get(reset=True)["predicted_queries"] == 0


def test_kernel_statistics_match_the_host_model(L, oracle):
    """m_q, v_q and the threshold of the prep kernel against the numpy restatement over the image and the column statistics it read;
    the statistics against a numpy restatement of the SQ8 codes (f32 operations of the quantiser)."""
    idx, data, queries, want, metric, k = shard(L, oracle, "gauss-70000x256-ip-k10")
    with knobs(1):
        dbg = idx.predict_debug(queries, k, "ip")
    n, cols = len(data), dbg["cols"]
    assert cols == 256 and dbg["u"].shape == (256, cols)
    mins, scales = idx.sq8_params()
    x = (data - mins) * scales                                               # f32, >= 0
    fl = np.floor(x)
    code = (fl + (x - fl >= f32(0.5))).astype(np.int64).clip(0, 255) - 128   # round half away from zero (x - floor(x) is exact)
    mu_np = code.sum(axis=0) / n
    var_np = np.maximum((code * code).sum(axis=0) / n - mu_np * mu_np, 0.0)
    assert np.array_equal(dbg["mu"], mu_np) and np.array_equal(dbg["var"], var_np)
    u = dbg["u"].astype(np.float64)
    m_np, v_np = u @ dbg["mu"], (u * u) @ dbg["var"]
    assert np.all(np.abs(dbg["m"] - m_np) <= 1e-12 * (np.abs(u) @ np.abs(dbg["mu"]))) and np.all(np.abs(dbg["v"] - v_np) <= 1e-12 * v_np)
    c = 40 * k
    lo, hi = 0.0, 40.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if 0.5 * math.erfc(mid * 0.7071067811865476) > c / n else (lo, mid)
    assert abs(dbg["z"] - 0.5 * (lo + hi)) <= 1e-12 * dbg["z"]
    thr_np = (dbg["bq"].astype(np.float64) + dbg["sq"].astype(np.float64) * (dbg["m"] + dbg["z"] * np.sqrt(dbg["v"]))).astype(f32)
    assert np.array_equal(thr_np.view(np.uint32), dbg["thr"].view(np.uint32))


# ---- verification and the miss path: the model is wrong on purpose, the answers stay exact
def miss_case(L, oracle, data, queries, k, metric, tag, sampled_plan_fits=True):
    idx = build(L, data)
    om = O.IP if metric == "ip" else O.COS
    want = oracle_for_every_query(lambda qi: oracle.canonical_topk(queries[qi], data, k, om), len(queries))
    rp = search(idx, queries, k, metric, 1)
    p = rp[3]
    print(f"{tag}: predicted {p['predicted_queries']}, missed {p['predict_miss_queries']}, fallback {p['fallback_queries']}, plan {hex(int(p['last_plan']))}")
    assert p["predicted_queries"] == len(queries) and p["predict_miss_queries"] > 0 and p["fallback_queries"] > 0, p
    assert not int(p["last_plan"]) & PLAN_PREDICT, hex(int(p["last_plan"]))      # the batch was answered again, without prediction
    assert_exact(want, *rp[:3], tag)
    assert idx.predict_state()["predict_strikes"] == 1 and idx.sq7_state()["sq7_strikes"] == 0
    if sampled_plan_fits:      # (a miss is no strike against the int8 pass; what the sampled plan then does with 69,995 ties is its own)
        assert idx.coarse_state()["i8c_strikes"] == 0
    return idx, rp, want


def test_one_repeated_vector_and_a_handful_of_outliers(L, oracle):
    """Variance near zero, massive ties: the five outliers pull the threshold above the 69,995 equal rows; fewer than k keys arrive."""
    rng = np.random.default_rng(2721)
    n, dim, nq, k = 70_000, 256, 130, 10
    base = rng.random(dim, dtype=f32)
    data = np.tile(base, (n, 1))
    out_rows = rng.choice(n, 5, replace=False)
    data[out_rows] = rng.random((5, dim), dtype=f32) * f32(2.0)
    queries = (base + 0.05 * rng.standard_normal((nq, dim)).astype(f32)).astype(f32)
    miss_case(L, oracle, data, queries, k, "ip", "repeated vector", sampled_plan_fits=False)


def test_cosine_over_non_negative_rows_is_a_systematic_miss(L, oracle):
    """Unit rows of uniform[0,1) data: the norm constraint ties the columns together (the component along the all-ones direction hardly
    varies), the diagonal model adds their variances up as if they were free and puts the threshold where only the query's own source row
    reaches it (measured: 1..3 rows per query at k = 10).  Every query misses; the batch is exact on the sampled plan."""
    rng = np.random.default_rng(2724)
    n, dim, nq, k = 70_001, 256, 200, 10
    data = rng.random((n, dim), dtype=f32)
    queries = perturbed(rng, data, nq, 0.03)
    idx, rp, want = miss_case(L, oracle, data, queries, k, "cosine", "cosine over uniform rows")
    cnt, _ = admitted(idx, data, queries, k, "cosine")
    assert cnt.max() < k, int(cnt.max())


def test_clustered_shard_with_queries_between_the_clusters(L, oracle):
    """Every row scores about dim / blocks against a query that weighs all blocks alike, so the true spread is the noise alone, while the
    diagonal model adds the block variances up: its tail — and the threshold — lies far above every row.  Nothing is emitted."""
    rng = np.random.default_rng(2722)
    n, dim, nq, k = 70_000, 256, 200, 10
    data = clustered(rng, n, dim, 8)
    queries = between_clusters(rng, nq, dim)
    idx, rp, want = miss_case(L, oracle, data, queries, k, "ip", "between clusters")
    cnt, _ = admitted(idx, data, queries, k, "ip")
    assert cnt.max() < k, int(cnt.max())                                     # (numpy agrees: fewer than k rows reach the threshold)


def test_fewer_than_k_rows_above_the_prediction(L, oracle):
    """Planted: for query 0 every row but five is pushed below 1.2 sigma of its score distribution, so the normal tail the model predicts
    above ~2.5 sigma holds the five planted rows only — fewer than k.  The other queries are unrelated directions and predict fine."""
    rng = np.random.default_rng(2723)
    n, dim, nq, k = 70_000, 256, 130, 10
    data, q0, keep = planted_tail(rng, n, dim)
    queries = rng.standard_normal((nq, dim)).astype(f32)
    queries[0] = q0
    idx, rp, want = miss_case(L, oracle, data, queries, k, "ip", "planted tail")
    cnt, _ = admitted(idx, data, queries, k, "ip")
    assert cnt[0] == 5 and cnt[1:].min() >= k, (int(cnt[0]), int(cnt[1:].min()))
    assert set(int(r) for r in rp[0][0, :5]) == set(int(r) for r in keep)


# ---- strikes and life cycle
def test_three_misses_switch_prediction_off_until_the_codes_are_fitted_again(L, oracle):
    rng = np.random.default_rng(2731)
    n, dim, nq, k = 70_000, 256, 130, 10
    data = clustered(rng, n, dim, 8)
    queries = between_clusters(rng, nq, dim)
    idx = build(L, data)
    r0 = search(idx, queries, k, "ip", 0)
    for strike in (1, 2, 3):
        r = search(idx, queries, k, "ip", 1)
        assert r[3]["predict_miss_queries"] > 0 and r[3]["predicted_queries"] == nq, (strike, r[3])
        assert_same(r, r0, strike)
        assert idx.predict_state()["predict_strikes"] == strike and idx.coarse_state()["i8c_strikes"] == 0
    r = search(idx, queries, k, "ip", 1)
    assert r[3]["predicted_queries"] == 0 and r[3]["fallback_queries"] == 0 and int(r[3]["last_plan"]) & PLAN_SAMPLED, r[3]      # struck out: the batch starts on the sampled plan
    assert_same(r, r0, "struck out")
    idx.update_rows(np.array([0], np.uint64), data[:1])                      # the derived state is rebuilt: prediction gets its three strikes back
    r = search(idx, queries, k, "ip", 1)
    assert r[3]["predicted_queries"] == nq and idx.predict_state()["predict_strikes"] == 1, r[3]


def test_statistics_follow_appends_updates_and_compaction(L, oracle):
    """After an append inside the fitted ranges (the sums take the new rows in), an append that forces a refit, update_rows and compact the
    statistics equal those of a fresh handle over the same rows, and so do the predicted-plan answers, bit for bit."""
    rng = np.random.default_rng(2732)
    n0, dim, nq, k = 100_000, 256, 200, 10
    data = rng.random((n0, dim), dtype=f32)
    queries = perturbed(rng, data, nq, 0.03)
    idx = build(L, data)

    def check(rows, tag):
        fresh = build(L, rows)
        a, b = search(idx, queries, k, "ip", 1), search(fresh, queries, k, "ip", 1)
        assert_predicted(a[3], nq, tag)
        assert_predicted(b[3], nq, tag)
        assert_same(a, b, tag)
        with knobs(1):
            da, db = idx.predict_debug(queries, k, "ip"), fresh.predict_debug(queries, k, "ip")
        assert np.array_equal(da["mu"], db["mu"]) and np.array_equal(da["var"], db["var"]), tag
        assert np.array_equal(da["thr"].view(np.uint32), db["thr"].view(np.uint32)), tag
        assert idx.predict_state()["stats_rows_sq8"] == len(rows) == len(idx), tag
        assert_same(a, search(idx, queries, k, "ip", 0), tag)

    check(data, "first build")
    fit = idx.coarse_state()
    inside = (0.1 + 0.8 * rng.random((5_001, dim), dtype=f32)).astype(f32)      # inside every column's fitted range: only these rows are coded
    idx.write(inside)
    idx.finalize()
    data = np.vstack([data, inside])
    check(data, "append inside the ranges")
    wider = (rng.random((3_000, dim), dtype=f32) * f32(1.5)).astype(f32)        # new maxima: a new fit, every row coded again
    idx.write(wider)
    idx.finalize()
    data = np.vstack([data, wider])
    check(data, "append with a refit")
    rows = np.sort(rng.choice(len(data), 700, replace=False)).astype(np.uint64)
    new = rng.random((700, dim), dtype=f32)
    idx.update_rows(rows, new)
    data[rows.astype(np.int64)] = new
    check(data, "update_rows")
    keep = rng.random(len(data)) < 0.9
    assert idx.compact(keep) == int(keep.sum())
    data = np.ascontiguousarray(data[keep])
    check(data, "compact")
    assert fit["i8c_strikes"] == 0 and idx.predict_state()["predict_strikes"] == 0
