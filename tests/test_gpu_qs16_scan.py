"""`-m gpu` tests of the 16x16x64 form of the query-stationary int8 scan (scan_qs.h, M16): the plain threshold stages of
a batch of 129..256 queries over 256..768 code columns run v_mfma_i32_16x16x64_i8 at the wave tile of the 32x32x32 form — a lane then holds
two queries, four lanes share a query and each has a private segment of its own.  `LYNSE_HIP_QS_M16` = 1 / 0 forces / disables the form
and `last_plan` bit 27 (include/lynse_hip.h) tells which one ran.  The form only ever changes speed: every case is compared, ids and f32
distance bits, with the CPU oracle and with the same batch on the 32x32x32 form.
"""
import os

import numpy as np
import pytest

import oracle as O
from conftest import oracle_for_every_query

pytestmark = pytest.mark.gpu
f32 = np.float32

PLAN_I8C = 4
PLAN_SQ7 = 1 << 26
PLAN_M16 = 1 << 27
N_SHARD = 327_680 + 37      # the size at which tests/test_gpu_sq7_scan.py gets the int8 query-stationary plan, with a ragged last tile
K = 10


@pytest.fixture(scope="module")
def L():
    import lynsedb_amd as L_

    assert L_._lib.device_count() >= 1
    return L_


def tiling(p):
    return (int(p["last_plan"]) >> 16) & 0xff


def search(idx, queries, metric, m16, sq7=None):
    """One profiled blocking batch with LYNSE_HIP_QS_M16 = m16 (and LYNSE_HIP_SQ7 = sq7 if given) -> (rows, dists, counts, profile)."""
    want = {"LYNSE_HIP_QS_M16": str(m16)}
    if sq7 is not None:
        want["LYNSE_HIP_SQ7"] = str(sq7)
    old = {name: os.environ.get(name) for name in want}
    os.environ.update(want)
    try:
        idx.profile_enable(True)
        idx.profile_get(reset=True)
        r, d, c = idx.search_batch_arrays(queries, K, metric)
        return r, d, c, idx.profile_get(reset=True)
    finally:
        for name, v in old.items():
            if v is None:
                os.environ.pop(name, None)
            else:
                os.environ[name] = v


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


def make_rows(kind, dim, seed, n=N_SHARD):
    rng = np.random.default_rng(seed)
    data = rng.random((n, dim), dtype=f32) if kind == "nonneg" else rng.standard_normal((n, dim)).astype(f32)
    q_rows = np.sort(rng.integers(0, n, 256))
    noise = f32(0.03) if kind == "nonneg" else f32(0.3)
    queries = (data[q_rows] + noise * rng.standard_normal((256, dim)).astype(f32)).astype(f32)
    return data, queries


# ---- one shard per (operand kind, width); the oracle's answers per metric, computed once for all 256 queries and shared by the query counts
_cases = {}


def case(L, oracle, kind, dim):
    key = (kind, dim)
    if key not in _cases:
        data, queries = make_rows(kind, dim, 2701 + dim + (0 if kind == "nonneg" else 1))
        _cases[key] = {"data": data, "queries": queries, "idx": build(L, data), "want": {}}
    return _cases[key]


def wanted(oracle, cs, metric, nq):
    if metric not in cs["want"]:
        m = O.IP if metric == "ip" else O.COS
        nq_all = 256 if cs["data"].shape[1] == 768 else 200
        cs["want"][metric] = oracle_for_every_query(lambda qi: oracle.canonical_topk(cs["queries"][qi], cs["data"], K, m), nq_all)
    return cs["want"][metric][:nq]


def check_both_forms(cs, oracle, metric, nq, sq7, tag):
    q = cs["queries"][:nq]
    r16 = search(cs["idx"], q, metric, 1, sq7)
    lp = int(r16[3]["last_plan"])
    assert lp & PLAN_M16 and lp & PLAN_I8C and tiling(r16[3]) == 0x81 and r16[3]["fallback_queries"] == 0, (tag, hex(lp), r16[3])
    if sq7 is not None:
        assert bool(lp & PLAN_SQ7) == bool(sq7), (tag, hex(lp))
    assert_exact(wanted(oracle, cs, metric, nq), *r16[:3], tag)
    r32 = search(cs["idx"], q, metric, 0, sq7)
    lp32 = int(r32[3]["last_plan"])
    assert not (lp32 & PLAN_M16) and lp32 & PLAN_I8C and tiling(r32[3]) == 0x81 and r32[3]["fallback_queries"] == 0, (tag, hex(lp32))
    assert (lp32 ^ lp) == PLAN_M16, (tag, hex(lp), hex(lp32))      # the same plan otherwise
    assert_same(r16, r32, tag)
    assert r16[3]["pool_entries"] == r32[3]["pool_entries"], (tag, r16[3], r32[3])      # identical key sets: the same rows were rescored


# 256: every lane live; 200: wave 6 has one dead 16-query block, wave 7 is dead; 130: a block with two live lanes
@pytest.mark.parametrize("nq", [256, 200, 130])
@pytest.mark.parametrize("metric", ["ip", "cosine"])
@pytest.mark.parametrize("kind", ["nonneg", "gauss"])
def test_768_columns(L, oracle, kind, metric, nq):
    """Non-negative rows: the IP batch reads the SQ7 codes (forced: auto starts at 10M rows), the cosine batch the SQ8 codes.  Gaussian rows: SQ8."""
    sq7 = (1 if metric == "ip" else None) if kind == "nonneg" else 0
    check_both_forms(case(L, oracle, kind, 768), oracle, metric, nq, sq7, (kind, metric, nq))


@pytest.mark.parametrize("metric", ["ip", "cosine"])
@pytest.mark.parametrize("kind", ["nonneg", "gauss"])
def test_256_columns(L, oracle, kind, metric):
    """Two slabs: the narrowest tiling of the form (a tile's first MFMA of each accumulator takes C = 0, its fourth is the last)."""
    sq7 = (1 if metric == "ip" else None) if kind == "nonneg" else 0
    check_both_forms(case(L, oracle, kind, 256), oracle, metric, 200, sq7, (kind, metric, 256))


def test_massive_ties_overflow_a_private_segment(L, oracle):
    """One row, duplicated into 128-row windows one grid stride (workgroups x 64 rows) apart: whatever the stages' first rows are, every
    window holds a whole 64-row tile, the tiles of a stage's windows fall to ONE workgroup, and each of them gives every lane of the
    duplicate's query 16 passing keys — from the third window of a stage on a lane's private segment (32 keys at 1024 segments) is full and
    the keys go to the shared candidate buffer.  All duplicates tie at the best score: the answer is the ten lowest of their rows."""
    import torch

    stride = torch.cuda.get_device_properties(0).multi_processor_count * 64
    windows, dim, nq = 16, 768, 130
    n = windows * stride + 37
    rng = np.random.default_rng(2711)
    data = rng.standard_normal((n, dim)).astype(f32)
    dup = (f32(1.5) * rng.standard_normal(dim)).astype(f32)
    for w in range(windows):
        data[w * stride + 200: w * stride + 328] = dup
    queries = rng.standard_normal((nq, dim)).astype(f32)
    queries[7] = dup
    idx = build(L, data)
    r16 = search(idx, queries, "ip", 1, 0)
    lp = int(r16[3]["last_plan"])
    assert lp & PLAN_M16 and lp & PLAN_I8C and tiling(r16[3]) == 0x81 and r16[3]["fallback_queries"] == 0, (hex(lp), r16[3])
    want = oracle_for_every_query(lambda qi: oracle.canonical_topk(queries[qi], data, K, O.IP), nq)
    assert_exact(want, *r16[:3], "ties")
    assert [int(x) for x in r16[0][7]] == list(range(200, 210)), r16[0][7]
    assert_same(r16, search(idx, queries, "ip", 0, 0), "ties, 32x32x32")


def test_append_to_a_shard_that_has_answered(L, oracle):
    cs = case(L, oracle, "gauss", 768)
    data, queries, n0 = cs["data"], cs["queries"][:200], 300_001
    idx = L.FlatIndex(None, 768)
    idx.write(data[:n0])
    idx.finalize()
    r0 = search(idx, queries, "ip", 1, 0)
    assert int(r0[3]["last_plan"]) & PLAN_M16 and r0[3]["fallback_queries"] == 0, r0[3]
    assert_same(r0, search(idx, queries, "ip", 0, 0), "before the append")
    idx.write(data[n0:])
    idx.finalize()
    r1 = search(idx, queries, "ip", 1, 0)
    assert int(r1[3]["last_plan"]) & PLAN_M16 and r1[3]["fallback_queries"] == 0, r1[3]
    assert_exact(wanted(oracle, cs, "ip", 200), *r1[:3], "after the append")


def test_a_batch_in_flight_equals_the_blocking_call(L, oracle):
    import torch

    cs = case(L, oracle, "gauss", 768)
    idx, dev = cs["idx"], torch.device("cuda", 0)
    batches = [cs["queries"][:256], cs["queries"][56:256]]
    blocking = [search(idx, q, "ip", 1, 0) for q in batches]
    assert all(int(b[3]["last_plan"]) & PLAN_M16 for b in blocking)
    outs = [(torch.zeros((len(q), K), dtype=torch.int64, device=dev), torch.zeros((len(q), K), dtype=torch.float32, device=dev),
             torch.zeros(len(q), dtype=torch.int32, device=dev)) for q in batches]
    old = os.environ.get("LYNSE_HIP_QS_M16")
    os.environ["LYNSE_HIP_QS_M16"] = "1"
    try:
        tickets = [idx.search_submit(torch.as_tensor(q, device=dev), K, "ip", *o) for q, o in zip(batches, outs)]
        for t in tickets:
            t.wait()
    finally:
        if old is None:
            del os.environ["LYNSE_HIP_QS_M16"]
        else:
            os.environ["LYNSE_HIP_QS_M16"] = old
    for b, o in zip(blocking, outs):
        assert np.array_equal(o[0].cpu().numpy().astype(np.uint64), b[0].astype(np.uint64))
        assert np.array_equal(o[1].cpu().numpy().view(np.uint32), b[1].view(np.uint32))
        assert np.array_equal(o[2].cpu().numpy().astype(np.int64), np.asarray(b[2]).astype(np.int64))
