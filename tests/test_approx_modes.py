"""Host side of the approximate flat search (`search(approx=True, eps=...)`): eps normalisation and rounding, the size policy against a
table kept as data (tests/golden/approx_policy.json), and the restatement the GPU tests compare against (tests/approx_ref/approx_ref.c)
checked on its own — against float64 and on the reference's own test cases.  No GPU."""
import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest

from approx_common import BRAY, CANB, CHEB, COS, IP, L1, L2, build_ref, f64_distances
from lynsedb_amd import _lib
from lynsedb_amd.core import APPROX_FLAT_METRICS, normalize_eps, round_distances_to_eps

f32 = np.float32
GOLDEN = Path(__file__).resolve().parent / "golden" / "approx_policy.json"


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return build_ref(tmp_path_factory.mktemp("approx_ref"))


def _bits(x):
    return np.asarray(x, f32).view(np.uint32)


def test_the_seven_metrics_and_the_abi():
    assert APPROX_FLAT_METRICS == (0, 1, 2, 7, 8, 9, 10)
    assert _lib.lib.lynse_hip_abi_version() == 1


def test_normalize_eps_known_answers(ref):
    # approx_search.rs:325-332
    for given, want in [(np.inf, 1e-4), (np.nan, 1e-4), (-1.0, 1e-4), (0.0, 1e-4), (1e-12, 1e-8), (-np.inf, 1e-4), (0.5, 0.5), (1e-8, 1e-8)]:
        assert f32(normalize_eps(given)) == f32(want), given
        assert f32(ref.lib.apx_normalize_eps(f32(given))) == f32(want), given
    assert f32(normalize_eps(None)) == f32(1e-4)


def test_round_to_eps_known_answers(ref):
    for rnd in (lambda v, e: round_distances_to_eps([v], e)[0], lambda v, e: ref.round([v], e)[0]):
        # approx_search.rs:288-294
        assert abs(rnd(1.234567, 1e-4) - f32(1.2346)) < 1e-6
        assert abs(rnd(1.23454, 1e-4) - f32(1.2345)) < 1e-6
        assert rnd(np.inf, 1e-4) == np.inf
        assert rnd(1e31, 1e-8) == f32(1e31)   # the quotient overflows: the value passes through
        # a half case: roundf goes away from zero, numpy's round to the even neighbour
        assert rnd(0.25, 0.5) == f32(0.5) and rnd(-0.25, 0.5) == f32(-0.5) and rnd(1.25, 0.5) == f32(1.5)
        assert np.round(f32(0.25) / f32(0.5)) * f32(0.5) == 0.0   # (what np.round would have given)
        assert rnd(-np.inf, 1e-4) == -np.inf and np.isnan(rnd(np.nan, 1e-4))
        assert rnd(3e38, 1e-3) == f32(3e38)                       # v / eps = inf
        assert rnd(0.9, 1.0) == 1.0 and rnd(0.6, 1.0) == 1.0 and rnd(0.4, 1.0) == 0.0
    # a whole array, in place semantics hidden behind the copy
    v = np.array([0.9, 0.6, np.inf, np.nan, 0.25], f32)
    assert np.array_equal(_bits(round_distances_to_eps(v, 0.5)), _bits(ref.round(v, 0.5)))
    assert v[0] == f32(0.9)   # the argument is left alone


def test_size_policy_against_the_table(ref):
    doc = json.loads(GOLDEN.read_text())
    lib = _lib.lib
    rows = doc["pools"]["rows"]
    assert {r[1] for r in rows} == {1, 10, 100} and {r[2] for r in rows} == {65537, 1000000, 10000000}
    for bits, k, n, ip_order, hyb_ip, hyb in rows:
        eps = np.array([bits], np.uint32).view(f32)[0]
        for mine in ((lib.lynse_hip_approx_ip_order_pool, lib.lynse_hip_approx_hybrid_ip_pool, lib.lynse_hip_approx_hybrid_pool),
                     (ref.lib.apx_ip_order_pool, ref.lib.apx_hybrid_ip_pool, ref.lib.apx_hybrid_pool)):
            assert (mine[0](k, n, eps), mine[1](k, n, eps), mine[2](k, n, eps)) == (ip_order, hyb_ip, hyb), (eps, k, n)
    srows = doc["samples"]["rows"]
    assert {r[1] for r in srows} == {17, 32, 33, 43, 128, 768}
    for bits, dim, s_ip, s_add, b_ip, b_add in srows:
        eps = np.array([bits], np.uint32).view(f32)[0]
        assert lib.lynse_hip_approx_hybrid_ip_sample_dims(dim, eps) == s_ip == ref.lib.apx_hybrid_ip_sample(dim, eps), (eps, dim)
        assert lib.lynse_hip_approx_hybrid_sample_dims(dim, eps) == s_add == ref.lib.apx_hybrid_sample(dim, eps), (eps, dim)
        for sample, want in ((s_ip, b_ip), (s_add, b_add)):
            st, ln = np.zeros(3, np.uint32), np.zeros(3, np.uint32)
            nb = lib.lynse_hip_approx_sampled_dim_blocks(dim, sample, st.ctypes.data_as(C.POINTER(C.c_uint32)), ln.ctypes.data_as(C.POINTER(C.c_uint32)))
            assert [[int(st[i]), int(ln[i])] for i in range(nb)] == want, (dim, sample)
            assert [list(b) for b in ref.blocks(dim, sample)] == want


def test_sampled_dim_blocks_known_answer(ref):
    assert ref.blocks(43, 32) == [(0, 11), (16, 11), (33, 10)]
    st, ln = np.zeros(3, np.uint32), np.zeros(3, np.uint32)
    p = C.POINTER(C.c_uint32)
    assert _lib.lib.lynse_hip_approx_sampled_dim_blocks(43, 32, st.ctypes.data_as(p), ln.ctypes.data_as(p)) == 3
    assert list(zip(st.tolist(), ln.tolist())) == [(0, 11), (16, 11), (33, 10)]
    assert ref.blocks(40, 40) == [(0, 40)] and ref.blocks(40, 1) == [(19, 1)] and ref.blocks(40, 2) == [(0, 1), (39, 1)]


@pytest.mark.parametrize("metric", [IP, L2, COS, L1, CHEB, CANB, BRAY])
@pytest.mark.parametrize("shape", [(300, 43), (4200, 40)])
def test_restatement_against_float64(ref, metric, shape):
    """paths 1 and 2 score every row: the distances agree with the metric's definition at the project's 1e-5 relative score contract
    (relative to the magnitude of the terms: an l2 distance from the norm expansion carries the rounding of |q|^2 + |v|^2)"""
    rng = np.random.default_rng(7 + metric)
    n, d = shape
    data = (rng.random((n, d), dtype=f32) - f32(0.25)).astype(f32)
    q = (rng.random(d, dtype=f32) - f32(0.25)).astype(f32)
    ans = ref.search(q, data, 10, metric, 1e-4)
    assert ans.info["path"] == (1 if metric in (L2, COS) else 2) and not ans.info["fell_back"]
    want = f64_distances(q, data, metric)
    mag = {IP: np.abs(data.astype(np.float64) * q).sum(1), L2: (data.astype(np.float64) ** 2).sum(1) + float((q.astype(np.float64) ** 2).sum()),
           COS: np.ones(n)}.get(metric, np.abs(want) + 1e-30)
    assert np.all(np.abs(ans.coarse - want) <= 1e-5 * mag)
    order = np.lexsort((np.arange(n), -ans.coarse if metric == IP else ans.coarse))[:10]
    assert np.array_equal(ans.rows, order.astype(np.uint64))
    assert np.array_equal(_bits(ans.dists), _bits(ans.coarse[order] + f32(0.0)))


def test_reference_case_raw_ranking_then_rounding(ref):
    # approx_search.rs:296-323
    ans = ref.search([1.0], np.array([[0.6], [0.9]], f32), 1, IP, 1.0)
    assert ans.rows.tolist() == [1] and abs(ans.dists[0] - 0.9) < 1e-6
    assert ref.round(ans.dists, 1.0).tolist() == [1.0]


def test_reference_case_tail_only_match(ref):
    # flat_mmap.rs:6162-6219: the whole signal in the last 32 of 128 dimensions, 4,096 rows
    for metric, idx, want in ((L2, 3000, 0.0), (IP, 3500, 32.0)):
        data = np.zeros((4096, 128), f32)
        q = np.zeros(128, f32)
        q[96:] = 1.0
        data[idx, 96:] = 1.0
        ans = ref.search(q, data, 1, metric, 1e-4)
        assert ans.rows.tolist() == [idx] and ans.dists.tolist() == [want]
        assert ans.info["path"] == (1 if metric == L2 else 2)


def test_reference_case_sum_orders_and_append(ref):
    # flat_mmap.rs:6222-6272
    n, d = 70000, 32
    data = np.zeros((n, d), f32)
    data[12345] = 1.0
    data[54321] = -2.0
    pos = ref.search(np.ones(d, f32), data, 1, IP, 1e-4)
    assert pos.rows.tolist() == [12345] and pos.dists.tolist() == [32.0]
    assert pos.info == {"path": 3, "ip_case": "sum_desc", "pool": 500, "sample_dims": 0, "fell_back": False}
    assert pos.pool.size == 500 and pos.pool[0] == 12345 and pos.pool[1:4].tolist() == [0, 1, 2]   # ties: row ascending
    neg = ref.search(-np.ones(d, f32), data, 1, IP, 1e-4)
    assert neg.rows.tolist() == [54321] and neg.dists.tolist() == [64.0] and neg.info["ip_case"] == "sum_asc"
    more = np.concatenate([data, np.full((1, d), 2.0, f32)])
    app = ref.search(np.ones(d, f32), more, 1, IP, 1e-4)
    assert app.rows.tolist() == [n] and app.dists.tolist() == [64.0]
    # a mixed query at dim 32: every dimension would be sampled, the exact search answers
    mixed = np.ones(d, f32)
    mixed[0] = -1.0
    mx = ref.search(mixed, data, 1, IP, 1e-4)
    assert mx.info["ip_case"] == "hybrid" and mx.info["fell_back"] and mx.rows.tolist() == [12345]


def test_reference_case_additive_hybrid_shortlists(ref):
    # approx_search.rs:444-473
    d, n = 32, 65537
    data = np.repeat((f32(1.0) + np.arange(n, dtype=f32) / f32(n))[:, None], d, axis=1).astype(f32)
    for metric in (L1, CHEB, CANB, BRAY):
        ans = ref.search(np.ones(d, f32), data, 5, metric, 1e-4)
        assert ans.rows.tolist() == [0, 1, 2, 3, 4], metric
        assert np.all(np.diff(ans.dists) >= 0)
        assert ans.info["path"] == 4 and ans.info["fell_back"]   # dim 32: sample_dims == dim


def test_restatement_paths_3_and_4_miss_what_the_pool_misses(ref):
    """the restatement is the approximate search, not the exact one: a best row outside the sampled blocks is missed"""
    rng = np.random.default_rng(3)
    n, d = 65537, 43
    data = rng.integers(-2, 3, (n, d)).astype(f32)
    q = rng.integers(-2, 3, d).astype(f32)
    q[q == 0] = 1.0
    blocks = ref.blocks(d, ref.lib.apx_hybrid_ip_sample(d, f32(1e-2)))
    outside = np.ones(d, bool)
    for s, ln in blocks:
        outside[s:s + ln] = False
    data[777] = 0.0
    data[777, outside] = 50.0 * np.sign(q[outside])   # the best inner product by far, nothing of it inside the blocks
    ans = ref.search(q, data, 1, IP, 1e-2)
    exact = int(np.argmax(data.astype(np.float64) @ q))
    assert exact == 777 and ans.info["ip_case"] == "hybrid" and not ans.info["fell_back"]
    assert ans.coarse[777] == 0.0 and 777 not in ans.pool and ans.rows.tolist() != [777]
