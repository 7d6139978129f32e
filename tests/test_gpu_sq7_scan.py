"""`-m gpu` tests of the SQ7 form of the FLAT-IP int8 scan: batches of 129..256 queries on the query-stationary tiling may stream a
NON-NEGATIVE 7-bit copy of the codes (scale 127 / range, codes 0..127, no offset) instead of the SQ8 codes (DESIGN 3.2 / 4.2;
`LYNSE_HIP_SQ7` = 1 / 0 / unset: on wherever eligible / off / auto).  The selection only ever changes speed: every case goes through the
C-ABI and is compared, ids and f32 distance bits, with the CPU oracle and with the same batch on the SQ8 codes; `last_plan` bit 26
(include/lynse_hip.h) tells which copy the stages read.
"""
import os

import numpy as np
import pytest

import oracle as O
from conftest import oracle_for_every_query

pytestmark = pytest.mark.gpu
f32 = np.float32

PLAN_I8C = 4
PLAN_QS_SAMPLE = 1 << 25
PLAN_SQ7 = 1 << 26
FORM_I8, FORM_SQ7 = 1, 16


@pytest.fixture(scope="module")
def L():
    import lynsedb_amd as L_

    assert L_._lib.device_count() >= 1
    return L_


def tiling(p):
    return (int(p["last_plan"]) >> 16) & 0xff


def search(idx, queries, k, sq7):
    """One profiled blocking batch with LYNSE_HIP_SQ7 = sq7 (None: unset = auto) -> (rows, dists, counts, profile)."""
    old = os.environ.pop("LYNSE_HIP_SQ7", None)
    if sq7 is not None:
        os.environ["LYNSE_HIP_SQ7"] = str(sq7)
    try:
        idx.profile_enable(True)
        idx.profile_get(reset=True)
        r, d, c = idx.search_batch_arrays(queries, k, "ip")
        return r, d, c, idx.profile_get(reset=True)
    finally:
        os.environ.pop("LYNSE_HIP_SQ7", None)
        if old is not None:
            os.environ["LYNSE_HIP_SQ7"] = old


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


# ---- parity at the smallest shape that reaches the path: 5 sample + threshold stages of the query-stationary tiling, one reference for both batch sizes
@pytest.fixture(scope="module")
def uniform_case(L, oracle):
    n, dim, nq, k = 327_680, 768, 256, 10
    rng = np.random.default_rng(2601)
    data = rng.random((n, dim), dtype=f32)
    q_rows = np.sort(rng.integers(0, n, nq))
    queries = (data[q_rows] + 0.03 * rng.standard_normal((nq, dim)).astype(f32)).astype(f32)
    want = oracle_for_every_query(lambda qi: oracle.canonical_topk(queries[qi], data, k, O.IP), nq)
    return build(L, data), queries, want, k


@pytest.mark.parametrize("nq", [256, 130])
def test_parity_with_the_oracle_and_with_the_sq8_scan(uniform_case, nq):
    idx, queries, want, k = uniform_case
    q = queries[:nq]
    r7 = search(idx, q, k, 1)
    p = r7[3]
    assert int(p["last_plan"]) & PLAN_SQ7 and int(p["last_plan"]) & PLAN_I8C, hex(int(p["last_plan"]))
    assert tiling(p) == 0x81 and p["fallback_queries"] == 0, p
    assert idx.sq7_state() == {"sq7_rows": len(idx), "sq7_strikes": 0}
    assert_exact(want[:nq], *r7[:3], ("sq7", nq))
    r8 = search(idx, q, k, 0)
    assert not (int(r8[3]["last_plan"]) & PLAN_SQ7) and tiling(r8[3]) == 0x81 and r8[3]["fallback_queries"] == 0, r8[3]
    assert_same(r7, r8, nq)
    print(f"SQ7 {nq} queries: rescored per query {p['pool_entries'] / nq:.1f} (SQ8: {r8[3]['pool_entries'] / nq:.1f})")
    # fewer than 129 queries, a small shard on auto: the copy is not read
    r_small = search(idx, queries[:100], k, 1)
    assert not (int(r_small[3]["last_plan"]) & PLAN_SQ7), r_small[3]
    r_auto = search(idx, q, k, None)
    assert not (int(r_auto[3]["last_plan"]) & PLAN_SQ7), r_auto[3]      # (auto starts at 10M rows)
    assert_same(r_auto, r8, ("auto", nq))


def test_ragged_end_and_append_with_a_new_maximum(L, oracle):
    n0, n1, dim, nq, k = 300_001, 10_000, 768, 130, 10
    rng = np.random.default_rng(2602)
    data = rng.random((n0 + n1, dim), dtype=f32)
    data[n0:] *= f32(1.5)                                  # the appended rows raise every dimension's maximum: a new fit, every code again
    q_rows = np.concatenate([np.sort(rng.integers(0, n0, nq - 30)), n0 + np.sort(rng.integers(0, n1, 30))])
    queries = (data[q_rows] + 0.03 * rng.standard_normal((nq, dim)).astype(f32)).astype(f32)
    idx = L.FlatIndex(None, dim)
    idx.write(data[:n0])
    idx.finalize()
    hbm_before = idx.hbm_bytes()
    r = search(idx, queries, k, 1)
    assert int(r[3]["last_plan"]) & PLAN_SQ7 and tiling(r[3]) == 0x81 and r[3]["fallback_queries"] == 0, r[3]
    assert idx.sq7_state()["sq7_rows"] == n0
    assert idx.hbm_bytes() >= hbm_before + 2 * n0 * dim          # the SQ8 codes and the SQ7 copy are both counted
    want0 = oracle_for_every_query(lambda qi: oracle.canonical_topk(queries[qi], data[:n0], k, O.IP), nq)
    assert_exact(want0, *r[:3], "before the append")
    idx.write(data[n0:])
    idx.finalize()
    r = search(idx, queries, k, 1)
    assert int(r[3]["last_plan"]) & PLAN_SQ7 and r[3]["fallback_queries"] == 0, r[3]
    assert idx.sq7_state()["sq7_rows"] == n0 + n1 and idx.coarse_state()["sq8_rows"] == n0 + n1
    want1 = oracle_for_every_query(lambda qi: oracle.canonical_topk(queries[qi], data, k, O.IP), nq)
    assert_exact(want1, *r[:3], "after the append")
    assert all(int(r[0][qi, 0]) == q_rows[qi] for qi in range(nq - 30, nq))      # the appended rows answer their own queries
    # rows inside the fitted ranges: only they are coded, the copy follows
    more = (rng.random((1_000, dim), dtype=f32) * f32(0.9)).astype(f32)
    idx.write(more)
    idx.finalize()
    r2 = search(idx, queries, k, 1)
    assert int(r2[3]["last_plan"]) & PLAN_SQ7 and idx.sq7_state()["sq7_rows"] == n0 + n1 + 1_000
    assert_same(r2, search(idx, queries, k, 0), "after the second append")


@pytest.mark.parametrize("dim", [256, 1024])
def test_other_widths(L, oracle, dim):
    """256 and 1024 columns, 200 queries, forced on.  EVERY stage of an SQ7 chunk reads the copy (the sample stage included, whichever
    kernel runs it: bit 26 describes the chunk), so the plan bit is asserted at both widths and the sample stage's kernel is only reported."""
    n, nq, k = 262_144, 200, 10
    rng = np.random.default_rng(2603 + dim)
    data = rng.random((n, dim), dtype=f32)
    q_rows = np.sort(rng.integers(0, n, nq))
    queries = (data[q_rows] + 0.03 * rng.standard_normal((nq, dim)).astype(f32)).astype(f32)
    idx = build(L, data)
    r7 = search(idx, queries, k, 1)
    lp = int(r7[3]["last_plan"])
    print(f"SQ7 {dim} columns: plan {hex(lp)}, sample stage on the query-stationary tiling: {bool(lp & PLAN_QS_SAMPLE)}, rescored per query {r7[3]['pool_entries'] / nq:.1f}")
    assert lp & PLAN_SQ7 and lp & PLAN_I8C and tiling(r7[3]) == 0x81 and r7[3]["fallback_queries"] == 0, r7[3]
    want = oracle_for_every_query(lambda qi: oracle.canonical_topk(queries[qi], data, k, O.IP), nq)
    assert_exact(want, *r7[:3], dim)
    assert_same(r7, search(idx, queries, k, 0), dim)


def test_mixed_sign_data_is_a_correctness_case(L, oracle):
    """Unit-Gaussian rows, mixed-sign queries: auto leaves the mode off and builds nothing, forced on the batch is answered BY the SQ7 scan
    (bit 26, no overflow) and is exact.  Not a speed case: the products are not non-negative.  The pool sizes are on record in the messages."""
    n, dim, nq, k = 300_000, 768, 256, 10
    rng = np.random.default_rng(2604)
    data = rng.standard_normal((n, dim)).astype(f32)
    queries = rng.standard_normal((nq, dim)).astype(f32)
    idx = build(L, data)
    r_auto = search(idx, queries, k, None)
    assert not (int(r_auto[3]["last_plan"]) & PLAN_SQ7) and idx.sq7_state()["sq7_rows"] == 0, r_auto[3]      # rows are not non-negative: auto leaves it off, nothing is built
    r7 = search(idx, queries, k, 1)
    p = r7[3]
    msg = f"mixed-sign SQ7: rescored per query {p['pool_entries'] / nq:.1f} (SQ8: {r_auto[3]['pool_entries'] / nq:.1f}), fallback queries {p['fallback_queries']}, plan {hex(int(p['last_plan']))}"
    print(msg)
    assert int(p["last_plan"]) & PLAN_SQ7 and int(p["last_plan"]) & PLAN_I8C, msg
    assert p["fallback_queries"] == 0 and idx.sq7_state() == {"sq7_rows": n, "sq7_strikes": 0}, msg
    want = oracle_for_every_query(lambda qi: oracle.canonical_topk(queries[qi], data, k, O.IP), nq)
    assert_exact(want, *r7[:3], msg)
    assert_same(r7, r_auto, msg)
    # back on auto the copy, which this shard will not scan, is freed again
    hbm = idx.hbm_bytes()
    search(idx, queries, k, None)
    assert idx.sq7_state()["sq7_rows"] == 0 and idx.hbm_bytes() <= hbm - n * dim, (hbm, idx.hbm_bytes())


def test_certificate_holds_on_a_constructed_worst_case(L):
    """Rows on code points plus residuals that are ALL on one side and parallel to the query's image (eps = 0.4999 u / 127), and a query whose
    own rounding residual is parallel to the largest code row (eta = 0.4999 c* / 127): both quantisation terms of
    q.v - coarse = s_q sum eta_d c_d + sum w_d eps_d are positive and near their Cauchy-Schwarz forms at the target pair.  With the mode's
    own coarse scores and E: |coarse - exact(f64)| <= E for every (row, query); the reached fraction is reported, not asserted."""
    rng = np.random.default_rng(2605)
    dim, n, nq, R = 256, 4096, 130, 16
    delta, s_q = 1.0 / 64.0, 2.0 ** -10
    anchors = np.full((R, dim), 64.0)
    for d in range(dim):
        anchors[d % R, d] = 0.0
        anchors[(d + R // 2) % R, d] = 127.0
    u = rng.integers(20, 127, dim).astype(np.float64)
    u[0] = 127.0                                                   # s_q = max w / 127 = 2^-10 exactly
    eps = 0.4999 * u / 127.0
    cstar = rng.integers(90, 128, dim).astype(np.float64)          # the largest code row
    cstar[0] = 0.0                                                 # (no residual on the element that fixes s_q)
    filler = rng.integers(20, 90, (n - R - 1, dim)).astype(np.float64) + eps
    data = (np.vstack([anchors, filler, cstar + eps]) * delta).astype(f32)
    q = rng.integers(40, 127, (nq, dim)) + rng.uniform(-0.49, 0.49, (nq, dim))
    q[0] = u + 0.4999 * cstar / 127.0
    q[:, 0] = 127.0
    queries = (q * s_q / delta).astype(f32)
    idx = build(L, data)
    os.environ["LYNSE_HIP_SQ7"] = "1"
    try:
        scores, bound, form = idx.coarse_scores_sq7(queries)
        s8, b8, form8 = idx.coarse_scores(queries, "ip", "i8")
    finally:
        del os.environ["LYNSE_HIP_SQ7"]
    assert form == FORM_I8 | FORM_SQ7 and form8 == FORM_I8 and scores.shape == (nq, n)
    exact = queries.astype(np.float64) @ data.astype(np.float64).T
    ratio = np.abs(scores.astype(np.float64) - exact) / bound.astype(np.float64)[:, None]
    worst = np.unravel_index(np.argmax(ratio), ratio.shape)
    r8 = np.abs(s8.astype(np.float64) - exact) / b8.astype(np.float64)[:, None]
    msg = (f"SQ7 certificate: max |coarse - exact| / E = {ratio.max():.4f} at (query, row) {worst}, E(q0) = {float(bound[0]):.4f}; "
           f"SQ8 on the same shard: {r8.max():.4f}, E(q0) = {float(b8[0]):.4f}")
    print(msg)
    assert ratio.max() <= 1.0, msg
    assert r8.max() <= 1.0, msg
    assert np.all(np.isfinite(bound)) and np.all(bound > 0), msg


@pytest.mark.parametrize("order,cap", [("score-ascending", 4096), ("insertion", 2048)])
def test_an_overflow_is_answered_on_the_sq8_codes_and_three_switch_sq7_off(L, oracle, order, cap):
    """Small candidate caps on unit-Gaussian rows (where the SQ7 margin leaves 3-4x the survivors of the SQ8 one), on a shard sorted by score
    (ascending along the rows) with a quarter of the default cap and on an unsorted one with an eighth: the SQ7 scan lets more rows through
    than the cap holds while the same plan level on the SQ8 codes fits.  Both pairs come from a sweep of the two scans over caps 256..8192 on
    these very shards (SQ8 0 overflowing queries, SQ7 9 and 201; one step smaller and SQ8 overflows too — the sorted shard at 2048, the
    unsorted one at 1024 —, one step larger and SQ7 fits; uniform rows have no such cap).  The batch is exact, the plan that answered is
    still the int8 pass, int8 takes no strike, and after three such batches the handle stops choosing SQ7."""
    n, dim, nq, k = 300_000, 768, 256, 10
    rng = np.random.default_rng(2607)
    data = rng.standard_normal((n, dim)).astype(f32)
    queries = rng.standard_normal((nq, dim)).astype(f32)
    if order == "score-ascending":
        data = np.ascontiguousarray(data[np.argsort(data.astype(np.float64) @ queries.astype(np.float64).mean(axis=0))])
    idx = build(L, data)
    idx.set_plan(stage0_rows=256, growth=8, cap=cap)
    r8 = search(idx, queries, k, 0)
    assert r8[3]["fallback_queries"] == 0 and int(r8[3]["last_plan"]) & PLAN_I8C, r8[3]      # the SQ8 scan fits these caps
    want = oracle_for_every_query(lambda qi: oracle.canonical_topk(queries[qi], data, k, O.IP), nq)
    assert_exact(want, *r8[:3], "sq8")
    for strike in (1, 2, 3):
        r7 = search(idx, queries, k, 1)
        p = r7[3]
        assert p["fallback_queries"] > 0, (strike, p)                                          # SQ7 overflowed ...
        assert int(p["last_plan"]) & PLAN_I8C and not (int(p["last_plan"]) & PLAN_SQ7), (strike, hex(int(p["last_plan"])))      # ... and the SQ8 codes answered
        assert_same(r7, r8, strike)
        assert idx.sq7_state()["sq7_strikes"] == strike and idx.coarse_state()["i8c_strikes"] == 0
    r = search(idx, queries, k, 1)
    assert not (int(r[3]["last_plan"]) & PLAN_SQ7) and r[3]["fallback_queries"] == 0, r[3]      # struck out: the batch starts on the SQ8 codes
    assert_same(r, r8, "struck out")
