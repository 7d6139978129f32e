"""`-m gpu` tests of the VERIFICATION of the predicted plan (`k_select_final`, `TailArgs::pred_chk`) at the places where only
the check keeps the answer exact, and of the miss machinery behind it (`search_impl`): k keys arrived but a row of the true top-k was not
emitted (the second half of the check), a query the model cannot serve, an overflow under too low a threshold, misses in one chunk of
several, three strikes inside one call, the compaction exit of the select under a valid prediction.  `LYNSE_HIP_PREDICT_C` moves the
threshold where a case needs it.

Every case goes through the C-ABI with LYNSE_HIP_PREDICT=1 and LYNSE_HIP_SQ7=0 and is compared, ids and f32 distance bits, with the CPU
oracle and with the same handle under LYNSE_HIP_PREDICT=0.  Before its results count, each case asserts the property of its inputs on
`restated_coarse` of the shard it built (tests/predict_common.py; tests/test_predict_verify_design.py checks the generators without a GPU).
"""
import numpy as np
import pytest

import oracle as O
import predict_common as P
from conftest import oracle_for_every_query
from predict_common import CAP, KEEP_MAX, PLAN_PREDICT, PLAN_SAMPLED, admitted, assert_exact, assert_predicted, assert_same, build, knobs, search

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def L():
    import lynsedb_amd as L_

    assert L_._lib.device_count() >= 1
    return L_


def oracle_ip(oracle, data, queries, k):
    return oracle_for_every_query(lambda qi: oracle.canonical_topk(queries[qi], data, k, O.IP), len(queries))


def restate(idx, data, queries, k, c):
    """(coarse scores, delta, surely emitted, not surely left out, predict_debug) of a batch of 129..256 queries at C = c."""
    with knobs(1, 0, c):
        dbg = idx.predict_debug(queries, k, "ip")
    coarse, delta = P.restated_coarse(idx, data, dbg)
    sure, maybe = P.emitted_counts(coarse, dbg["thr"], delta)
    return coarse, delta, sure, maybe, dbg


@pytest.fixture(scope="module")
def band(L, oracle):
    """The unplanted band shard, its handle and the oracle's answers: cases 1 and 2."""
    data, queries, src = P.band_inputs()
    return build(L, data), data, queries, src, oracle_ip(oracle, data, queries, P.BAND_K)


# ---- 1. the band: k keys arrived and the plan is still invalid
@pytest.fixture(scope="module")
def planted(L, oracle, band):
    """plant_band on the band shard at C = 1: for 8 queries six helper rows bring the keys at or above the threshold to k or more, and one
    victim row lies in the exact top-k with a coarse score under the threshold.  A picked query COUNTS when, on the restatement, at least k
    rows are surely emitted, the victim is surely not, and the oracle's top-k holds the victim.  The construction of the issue stood as
    written on the device: victim at thr - 1.0, helpers from thr + 0.8 (the figures of one run are in DESIGN 24)."""
    idx0, data0, queries, src, _ = band
    k, c = P.BAND_K, 1
    coarse0, _, _, _, dbg0 = restate(idx0, data0, queries, k, c)
    picks = P.pick_band_queries((coarse0 >= dbg0["thr"].astype(np.float64)[:, None]).sum(axis=1))
    assert len(picks) == P.BAND_PICKS
    mins, scales = idx0.sq8_params()
    data, victims, _ = P.plant_band(np.random.default_rng(2742), data0, queries, dbg0["thr"], picks, k, mins=mins, scales=scales, avoid=src)
    idx = build(L, data)
    m1, s1 = idx.sq8_params()
    assert np.array_equal(m1.view(np.uint32), mins.view(np.uint32)) and np.array_equal(s1.view(np.uint32), scales.view(np.uint32))
    coarse, delta, sure, maybe, dbg = restate(idx, data, queries, k, c)
    thr = dbg["thr"].astype(np.float64)
    want = oracle_ip(oracle, data, queries, k)
    counting = {int(qi): int(v) for qi, v in zip(picks, victims)
                if sure[qi] >= k and coarse[qi, v] < thr[qi] - delta[qi] and v in want[qi][0].astype(np.int64)}
    print(f"band, planted: {len(counting)} of {len(picks)} planted queries count; {int((maybe < k).sum())} queries surely short of k, "
          f"{int(((sure < k) & (maybe >= k)).sum())} undetermined; "
          + "; ".join(f"q{qi}: {int(sure[qi])} emitted, victim {thr[qi] - coarse[qi, v]:.2f} under thr" for qi, v in zip(picks, victims)))
    assert len(counting) >= 4, counting                                     # a condition on the inputs, not a tolerance
    return idx, data, queries, want, counting, sure, maybe, picks


def test_k_keys_arrived_and_a_top_k_row_was_not_emitted(planted):
    """Only `a.s.thr[q] >= chk` in k_select_final notices a counting query: the lower bound on predict_miss_queries shows that it fired."""
    idx, data, queries, want, counting, sure, maybe, _ = planted
    k, short = P.BAND_K, int((maybe < P.BAND_K).sum())
    rp = search(idx, queries, k, "ip", 1, c=1)
    p = rp[3]
    print(f"band, planted: predicted {p['predicted_queries']}, missed {p['predict_miss_queries']}, fallback {p['fallback_queries']}, plan {hex(int(p['last_plan']))}")
    assert_exact(want, *rp[:3], "band planted")
    for qi, v in counting.items():
        assert v in rp[0][qi].astype(np.int64), (qi, v, rp[0][qi])
    assert p["predicted_queries"] == 256
    assert p["predict_miss_queries"] >= len(counting) + short, (p["predict_miss_queries"], len(counting), short)
    assert idx.predict_state()["predict_strikes"] == 1 and idx.coarse_state()["i8c_strikes"] == 0
    assert not int(p["last_plan"]) & PLAN_PREDICT, hex(int(p["last_plan"]))
    assert_same(rp, search(idx, queries, k, "ip", 0), "band planted")


def test_the_band_alone_sends_the_chunk_back(L, planted):
    """The same shard with nothing but the second half of the check to fire: a batch of the counting queries and of queries that surely
    received k keys, repeated to 256.  No query of it is short of k, so without `thr[q] >= chk` the chunk would not be answered again and
    the victims' rows would be missing from the result."""
    _, data, queries, want, counting, sure, _, picks = planted
    k = P.BAND_K
    fine = [int(qi) for qi in np.flatnonzero(sure >= k) if qi not in picks]
    sel = np.array((list(counting) + fine) * 256)[:256]
    assert fine and (sure[sel] >= k).all()
    idx = build(L, data)
    rb = search(idx, queries[sel], k, "ip", 1, c=1)
    p = rb[3]
    print(f"band, planted, no short query: predicted {p['predicted_queries']}, missed {p['predict_miss_queries']}, fallback {p['fallback_queries']}")
    for j, qi in enumerate(sel):
        if int(qi) in counting:
            assert counting[int(qi)] in rb[0][j].astype(np.int64), (j, qi, counting[int(qi)], rb[0][j])
    assert_exact([want[qi] for qi in sel], *rb[:3], "band planted, no short query")
    assert p["predicted_queries"] == 256 and p["predict_miss_queries"] >= sum(int(qi) in counting for qi in sel), p
    assert idx.predict_state()["predict_strikes"] == 1 and not int(p["last_plan"]) & PLAN_PREDICT
    assert_same(rb, search(idx, queries[sel], k, "ip", 0), "band planted, no short query")


# ---- 2. the band without planting
def test_the_band_on_random_rows(L, oracle, band):
    """C = 2: nearly every query receives k keys or more, and whether its plan is valid is decided by the second half of the check alone.
    Nothing is pinned but exactness and the bounds the restatement gives; the split printed here is the only view of how wide the band is."""
    idx, data, queries, _, want = band
    k, c = P.BAND_K, 2
    _, _, sure, maybe, _ = restate(idx, data, queries, k, c)
    assert int((sure >= k).sum()) >= 200, int((sure >= k).sum())
    short, undet = int((maybe < k).sum()), int(((sure < k) & (maybe >= k)).sum())
    rp = search(idx, queries, k, "ip", 1, c=c)
    p = rp[3]
    miss = int(p["predict_miss_queries"])
    print(f"band, unplanted, C = 2: valid {256 - miss}, missed with at least k keys {miss - short}{' (+-' + str(undet) + ' undetermined)' if undet else ''}, "
          f"missed short of k {short}; fallback {p['fallback_queries']}, plan {hex(int(p['last_plan']))}")
    assert_exact(want, *rp[:3], "band unplanted")
    assert p["predicted_queries"] == 256 and short <= miss <= 256, (miss, short)
    assert_same(rp, search(idx, queries, k, "ip", 0), "band unplanted")


# ---- 3. too low a threshold
def test_an_overflow_under_a_predicted_threshold_is_a_strike(L, oracle):
    data, queries = P.overflow_inputs()
    k, c = 10, P.OVER_C
    idx = build(L, data)
    _, _, sure, _, _ = restate(idx, data, queries, k, c)
    assert sure.min() > CAP, int(sure.min())
    want = oracle_ip(oracle, data, queries, k)
    rp = search(idx, queries, k, "ip", 1, c=c)
    p = rp[3]
    print(f"overflow: {int(sure.min())}..{int(sure.max())} rows surely emitted; predicted {p['predicted_queries']}, missed {p['predict_miss_queries']}, fallback {p['fallback_queries']}, "
          f"i8c strikes {idx.coarse_state()['i8c_strikes']}")
    assert_exact(want, *rp[:3], "overflow")
    assert p["predicted_queries"] == 256 and p["fallback_queries"] >= 256, p
    assert idx.predict_state()["predict_strikes"] == 1 and idx.sq7_state()["sq7_strikes"] == 0
    assert_same(rp, search(idx, queries, k, "ip", 0), "overflow")


# ---- 4. a query the model cannot serve
def test_a_zero_query_is_unpredicted_and_no_strike(L, oracle):
    """Query 17 is all zeros: u = 0, v_q = 0, thr = pred_chk = +inf — PRED_NONE.  The chunk is answered again; it is no strike."""
    rng = np.random.default_rng(2744)
    n, dim, nq, k = 70_000, 256, 200, 10
    data = rng.standard_normal((n, dim)).astype(f32)
    queries = P.perturbed(rng, data, nq, 0.1)
    queries[17] = 0
    idx = build(L, data)
    with knobs(1):
        dbg = idx.predict_debug(queries, k, "ip")
    assert not dbg["u"][17].any() and dbg["v"][17] == 0.0 and dbg["thr"][17] == np.inf and np.isfinite(np.delete(dbg["thr"], 17)).all()
    others = np.delete(np.arange(nq), 17)
    cnt, _ = admitted(idx, data, queries[others], k, "ip")
    assert cnt.min() >= 3 * k and cnt.max() <= CAP // 3, (int(cnt.min()), int(cnt.max()))
    want = oracle_ip(oracle, data, queries, k)
    assert want[17][0].astype(np.int64).tolist() == list(range(k))          # every score ties: rows 0 .. k - 1
    rp = search(idx, queries, k, "ip", 1)
    p = rp[3]
    print(f"zero query: predicted {p['predicted_queries']}, missed {p['predict_miss_queries']}, fallback {p['fallback_queries']}, plan {hex(int(p['last_plan']))}")
    assert_exact(want, *rp[:3], "zero query")
    assert p["predicted_queries"] == nq and p["predict_miss_queries"] == 0 and p["fallback_queries"] >= 1, p
    assert idx.predict_state()["predict_strikes"] == 0
    assert_same(rp, search(idx, queries, k, "ip", 0), "zero query")


# ---- 5. more than one chunk
@pytest.fixture(scope="module")
def tail_shard(oracle):
    """The planted-tail shard of test_fewer_than_k_rows_above_the_prediction: q0 has five rows in its predicted tail; 400 random directions
    predict fine.  One oracle answer per query, shared by the sub-cases."""
    rng = np.random.default_rng(2745)
    n, dim, k = 70_000, 256, 10
    data, q0, _ = P.planted_tail(rng, n, dim)
    pool = rng.standard_normal((400, dim)).astype(f32)
    return data, q0, pool, oracle_ip(oracle, data, pool, k), oracle_ip(oracle, data, q0[None, :], k)[0], k


def chunks_with_a_missing_query(idx, data, queries, k):
    """Per 256-query chunk of the batch that is large enough to predict: does some query have fewer than k rows at or above its threshold
    (exact scores, `admitted`)?  The other queries must have them comfortably (3 k)."""
    out = []
    for q0 in range(0, len(queries), 256):
        q = queries[q0:q0 + 256]
        if len(q) <= 128:
            continue
        cnt, _ = admitted(idx, data, q, k, "ip")
        assert ((cnt < k) | (cnt >= 3 * k)).all(), (q0, np.sort(cnt)[:5])
        out.append(bool((cnt < k).any()))
    return out


@pytest.mark.parametrize("sub,nq,at,missing,bit28", [("a", 400, 300, [False, True], False), ("b", 400, 10, [True, False], True), ("c", 300, None, [False], None)])
def test_a_miss_in_one_chunk_of_several(L, tail_shard, sub, nq, at, missing, bit28):
    """allow_predict is per chunk, strikes are per handle, a re-answered chunk overwrites its own outputs at q0 * k.  (a) the miss is in the
    second chunk (144 queries), which ends sampled; (b) in the first, the second ends predicted; (c) no miss, and the 44-query tail keeps
    its own plan."""
    data, q0, pool, want_pool, want_q0, k = tail_shard
    queries, want = pool[:nq].copy(), list(want_pool[:nq])
    if at is not None:
        queries[at], want[at] = q0, want_q0
    idx = build(L, data)
    assert chunks_with_a_missing_query(idx, data, queries, k) == missing
    rp = search(idx, queries, k, "ip", 1)
    p = rp[3]
    print(f"chunks ({sub}): predicted {p['predicted_queries']}, missed {p['predict_miss_queries']}, fallback {p['fallback_queries']}, plan {hex(int(p['last_plan']))}")
    assert_exact(want, *rp[:3], sub)
    if at is not None:
        assert p["predicted_queries"] == nq and p["predict_miss_queries"] >= 1, p
        assert idx.predict_state()["predict_strikes"] == 1
        assert bool(int(p["last_plan"]) & PLAN_PREDICT) == bit28, hex(int(p["last_plan"]))
    else:
        assert p["predicted_queries"] == 256 and p["predict_miss_queries"] == 0 and p["fallback_queries"] == 0, p
        assert idx.predict_state()["predict_strikes"] == 0
    r0 = search(idx, queries, k, "ip", 0)
    assert r0[3]["predicted_queries"] == 0
    assert_same(rp, r0, sub)


def test_three_strikes_inside_one_call(L, oracle):
    """(d) 1,024 queries between the clusters: the first three chunks miss and are answered again, the fourth starts on the sampled plan."""
    rng = np.random.default_rng(2747)
    n, dim, nq, k = 70_000, 256, 1024, 10
    data = P.clustered(rng, n, dim, 8)
    queries = P.between_clusters(rng, nq, dim)
    idx = build(L, data)
    for q0 in range(0, nq, 256):
        cnt, _ = admitted(idx, data, queries[q0:q0 + 256], k, "ip")
        assert cnt.max() < k, (q0, int(cnt.max()))
    want = oracle_ip(oracle, data, queries, k)
    rp = search(idx, queries, k, "ip", 1)
    p = rp[3]
    print(f"chunks (d): predicted {p['predicted_queries']}, missed {p['predict_miss_queries']}, fallback {p['fallback_queries']}, plan {hex(int(p['last_plan']))}")
    assert_exact(want, *rp[:3], "d")
    assert p["predicted_queries"] == 768 and p["predict_miss_queries"] >= 3, p
    assert idx.predict_state()["predict_strikes"] == 3
    assert not int(p["last_plan"]) & PLAN_PREDICT and int(p["last_plan"]) & PLAN_SAMPLED, hex(int(p["last_plan"]))
    assert_same(rp, search(idx, queries, k, "ip", 0), "d")


# ---- 6. the compaction exit under a valid prediction
def test_the_compaction_exit_writes_a_threshold_the_check_accepts(L, oracle):
    """9,000 equal rows far above the threshold: more than keep_max survivors, so select_body leaves through the compaction exit and the
    check reads x_k - 2E, formed from exact scores.  The plan is valid; the ties are cut by row id."""
    data, ids, queries = P.duplicate_inputs()
    k, near = 10, P.DUP_NEAR
    idx = build(L, data)
    _, _, sure, maybe, _ = restate(idx, data, queries, k, None)
    assert sure[:near].min() >= P.DUP_COPIES > KEEP_MAX and maybe[:near].max() <= 12_000 < CAP, (int(sure[:near].min()), int(maybe[:near].max()))
    assert sure[near:].min() >= 3 * k and maybe[near:].max() <= CAP // 3, (int(sure[near:].min()), int(maybe[near:].max()))
    want = oracle_ip(oracle, data, queries, k)
    rp = search(idx, queries, k, "ip", 1)
    print(f"duplicates: near {int(sure[:near].min())}..{int(maybe[:near].max())} keys, far {int(sure[near:].min())}..{int(maybe[near:].max())}; rescored per query {rp[3]['pool_entries'] / len(queries):.1f}")
    assert_predicted(rp[3], len(queries), "duplicates")
    assert_exact(want, *rp[:3], "duplicates")
    assert (rp[0][:near].astype(np.int64) == ids[:k][None, :]).all()
    rn = search(idx, queries[:near], k, "ip", 1)
    assert_predicted(rn[3], near, "duplicates, near")
    assert rn[3]["pool_entries"] == near * k, rn[3]                        # the compaction hands on exactly k keys per query
    assert_same(rn, tuple(a[:near] for a in rp[:3]), "duplicates, near")
    assert_same(rp, search(idx, queries, k, "ip", 0), "duplicates")
    assert idx.predict_state()["predict_strikes"] == 0
