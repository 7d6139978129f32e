"""Row mutation on the GPU (the ROW MUTATION block of include/lynse_hip.h): lynse_hip_flat_update_rows_f32,
lynse_hip_flat_compact_rows, lynse_hip_flat_gather_rows and the Collection calls on top of them (upsert_items, update_items, compact,
read_vectors_by_ids).  Every comparison is exact — row bits, ids, f32 distance bits, counts — against three yardsticks: numpy models of
the row content, the CPU oracle for search answers, and a FRESH handle or collection given the final rows for everything a search, a
fit or a graph build produces."""
import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu
f32 = np.float32
METRICS = (("ip", O.IP), ("l2", O.L2), ("cosine", O.COS))


@pytest.fixture(scope="module")
def L():
    import lynsedb_amd as L_

    assert L_._lib.device_count() >= 1
    return L_


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same_search(a, b, tag):
    for x, y in zip(a, b):
        assert np.array_equal(bits(x) if x.dtype == f32 else x, bits(y) if y.dtype == f32 else y), tag


def assert_searches(L, orc, idx, model, tag, f16=False, queries=None, k=10):
    """ip / l2 / cosine over `idx` equal a fresh handle holding `model` and the oracle"""
    n, dim = model.shape
    rng = np.random.default_rng(77)
    q = rng.standard_normal((16, dim)).astype(f32) if queries is None else queries
    if n:
        q[0] = model[n // 2]
    fresh = L.FlatIndex(None, dim, dtype="f16" if f16 else "f32")
    if n:
        fresh.write(model)
    for name, m in METRICS:
        got, exp = idx.search_batch_arrays(q, k, name), fresh.search_batch_arrays(q, k, name)
        assert_same_search(got, exp, (tag, name))
        rows, dists, counts = got
        for qi in range(q.shape[0]):
            if n == 0:
                assert int(counts[qi]) == 0
                continue
            e_ids, e_d = orc.canonical_topk_f16(q[qi], model, k, m) if f16 else orc.canonical_topk(q[qi], model, k, m)
            assert int(counts[qi]) == len(e_ids) == min(k, n), (tag, name, qi)
            assert np.array_equal(rows[qi, :len(e_ids)].astype(np.uint32), e_ids), (tag, name, qi)
            assert np.array_equal(bits(dists[qi, :len(e_ids)]), bits(e_d)), (tag, name, qi)
    return fresh


def warm_up(idx, stored):
    """The lazy copies exist before the mutation: 16 queries of l2 and cosine run the staged pipeline (row statistics and norms, the f16
    shadow — an F16 shard's is an alias of its rows), a Hamming search packs the sign words.  Asserted from the profile not to be the fused
    single-launch search (last_plan bit 5), which reads the f32 rows alone."""
    q = stored[:16].copy()
    idx.profile_enable(True)
    for name in ("l2", "cosine"):
        idx.profile_get(reset=True)
        idx.search_batch_arrays(q, 5, name)
        p = idx.profile_get(reset=True)
        assert not int(p["last_plan"]) & 32 and p["scan_launches"] >= 1, (name, p)
    idx.search_batch_arrays(q, 5, "hamming")
    idx.profile_enable(False)


def compaction_case(L, orc, data, keep, window_rows, tag, f16=False, n_words=None, garbage=False):
    n, dim = data.shape
    idx = L.FlatIndex(None, dim, dtype="f16" if f16 else "f32")
    idx.write(data)
    stored = idx.read_rows(0, n)   # (an F16 shard: the decoded f16 values)
    warm_up(idx, stored)
    row_bytes = (-(-dim // 8) * 8 * 2) if f16 else (-(-dim // 4) * 4 * 4)
    if n_words is None:
        new_len = idx.compact(keep, window_rows)
    else:   # more words than needed, bits set beyond n
        b = np.concatenate([keep, np.full(n_words * 64 - n, garbage, bool)])
        new_len = idx.compact(L.BitSet(n_words * 64, np.packbits(b, bitorder="little").view(np.uint64)), window_rows)
    model = stored[keep]
    assert new_len == len(idx) == model.shape[0], tag
    assert np.array_equal(bits(idx.read_rows(0, new_len)), bits(model)), tag
    assert_searches(L, orc, idx, model, tag, f16=f16)
    assert idx.hbm_bytes() >= n * row_bytes, tag   # the capacity did not shrink: the row buffer still holds at least the old rows
    more = np.random.default_rng(5).standard_normal((100, dim)).astype(f32)
    idx.write(more)
    assert len(idx) == new_len + 100
    got = idx.read_rows(new_len, 100)
    assert np.array_equal(bits(got), bits(more.astype(np.float16).astype(f32) if f16 else more)), tag
    assert np.array_equal(bits(idx.read_rows(0, new_len)), bits(model)), tag
    return idx


@pytest.fixture(scope="module")
def small():   # n = 1001, dim 5 (pitch 8)
    return np.random.default_rng(1).standard_normal((1001, 5)).astype(f32)


@pytest.mark.parametrize("n,case", [(1000, "row0"), (1000, "clear_0_62"), (1000, "clear_0_63"), (1000, "clear_0_64"), (1000, "last"),
                                    (1001, "last"), (1001, "alternating")])
def test_compact_window_edges(L, oracle, small, n, case):
    """window_rows = 64: row 0 alone (every window staged, destination overlapping its own window by all but one row), shifts of W - 1
    (staged), W (the first direct window) and W + 1, the last row, a tail word of one bit, alternating rows"""
    idx = np.arange(n)
    keep = {"row0": idx != 0, "clear_0_62": idx > 62, "clear_0_63": idx > 63, "clear_0_64": idx > 64, "last": idx != n - 1,
            "alternating": idx % 2 == 0}[case]
    plan = L.FlatIndex.compact_plan(keep, n, 64)
    want = {"row0": {2}, "clear_0_62": {1, 2}, "clear_0_63": {1}, "clear_0_64": {1}, "last": {0, 2}, "alternating": {1, 2}}[case]
    assert set(plan["windows"][:, 3].tolist()) == want   # (the paths this case is here for)
    compaction_case(L, oracle, small[:n], keep, 64, (n, case))


def test_compact_everything_then_write(L, oracle, small):
    idx = L.FlatIndex(None, 5)
    idx.write(small)
    warm_up(idx, small)
    assert idx.compact(np.zeros(1001, bool), 64) == 0 and len(idx) == 0
    for name, _ in METRICS:
        rows, dists, counts = idx.search_batch_arrays(small[:4].copy(), 3, name)
        assert not counts.any()
    idx.write(small[:300])
    assert len(idx) == 300 and np.array_equal(bits(idx.read_rows(0, 300)), bits(small[:300]))
    assert_searches(L, oracle, idx, small[:300], "after emptying")


def test_compact_nothing_changes_nothing(L, oracle, small):
    idx = L.FlatIndex(None, 5)
    idx.write(small)
    idx.search_sq8_batch_arrays(small[:4].copy(), 5, "ip")   # SQ8 codes exist
    idx.build_hnsw("l2", 4, 16, 8)
    state, graph = idx.coarse_state(), idx.hnsw_params()
    assert state["sq8_rows"] == 1001 and graph["n"] == 1001
    assert idx.compact(np.ones(1001, bool), 64) == 1001 and idx.compact(L.BitSet.from_rows(np.arange(1001), 1001)) == 1001
    assert idx.coarse_state() == state
    after = idx.hnsw_params()
    assert after["n"] == 1001 and np.array_equal(after["adj0"], graph["adj0"])
    assert np.array_equal(bits(idx.read_rows(0, 1001)), bits(small))


@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
def test_compact_random_two_windows_per_path(L, oracle, p):
    """n = 5000, dim 128, window_rows = 128; n_words longer than needed with bits set beyond n"""
    rng = np.random.default_rng(int(p * 10))
    data = rng.standard_normal((5000, 128)).astype(f32)
    compaction_case(L, oracle, data, rng.random(5000) >= p, 128, ("random", p), n_words=5000 // 64 + 3, garbage=True)


def test_compact_default_window(L, oracle):
    rng = np.random.default_rng(8)
    data = rng.standard_normal((3000, 768)).astype(f32)
    compaction_case(L, oracle, data, rng.random(3000) >= 0.5, 0, "default window")


def test_compact_wide_rows(L, oracle):
    """n = 70, dim 20,000 (rows of 80 KB): one default window over both words, and the smallest window, 64 rows"""
    rng = np.random.default_rng(9)
    data = rng.standard_normal((70, 20000)).astype(f32)
    keep = np.ones(70, bool)
    keep[[0, 35]] = False
    assert L.FlatIndex.compact_plan(keep, 70, 0, 80000)["window_rows"] == 832   # (64 MiB / 80 KB; the clamp itself: test_mutation_modes)
    compaction_case(L, oracle, data, keep, 0, "wide rows")
    compaction_case(L, oracle, data, keep, 64, "wide rows, 64")


def test_compact_f16_shard_odd_half_pitch(L, oracle):
    rng = np.random.default_rng(10)
    data = rng.standard_normal((2000, 130)).astype(f32)
    compaction_case(L, oracle, data, rng.random(2000) >= 0.5, 128, "f16", f16=True)


# ---- update -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [5, 128])
def test_update_rows(L, oracle, dim):
    rng = np.random.default_rng(20 + dim)
    n = 2000
    data = rng.standard_normal((n, dim)).astype(f32)
    idx = L.FlatIndex(None, dim)
    idx.write(data)
    warm_up(idx, data)
    rows = np.concatenate([[0, 63, 64, n - 1], rng.choice(np.setdiff1d(np.arange(n), [0, 63, 64, n - 1]), 100, replace=False)])
    rng.shuffle(rows)
    new = rng.standard_normal((rows.size, dim)).astype(f32)
    idx.update_rows(rows, new)
    model = data.copy()
    model[rows] = new
    assert len(idx) == n and np.array_equal(bits(idx.read_rows(0, n)), bits(model))
    assert_searches(L, oracle, idx, model, ("update", dim))


def _int_batches(rng, dim):
    return rng.integers(0, 4, (256, dim)).astype(f32), rng.integers(0, 4, (8, dim)).astype(f32)


@pytest.mark.parametrize("direction", ["small_to_large", "large_to_small"])
def test_update_recomputes_the_accumulated_flags(L, oracle, direction):
    """Rows of integers in 0..3: rows_integer / rows_nonneg / amax / vmin only ever move one way under append.  One row becomes large,
    negative and fractional (and back): every answer must be the oracle's and the coarse state a fresh handle's."""
    rng = np.random.default_rng(31)
    n, dim = 70_000, 32   # (>= 64K rows: the certified int8 pass takes the 256-query batch)
    data = rng.integers(0, 4, (n, dim)).astype(f32)
    odd = (rng.standard_normal(dim) * 1000.0 - 500.37).astype(f32)
    odd[0] = -1234.5678
    plain = rng.integers(0, 4, dim).astype(f32)
    if direction == "large_to_small":
        data[4321] = odd
    q256, q8 = _int_batches(rng, dim)
    idx = L.FlatIndex(None, dim)
    idx.write(data)
    for q in (q256, q8):
        idx.search_batch_arrays(q, 10, "ip")   # every lazy copy exists
    new_row = odd if direction == "small_to_large" else plain
    idx.update_rows([4321], new_row.reshape(1, -1))
    model = data.copy()
    model[4321] = new_row
    fresh = L.FlatIndex(None, dim)
    fresh.write(model)
    for q in (q256, q8):
        got, exp = idx.search_batch_arrays(q, 10, "ip"), fresh.search_batch_arrays(q, 10, "ip")
        assert_same_search(got, exp, direction)
        rows, dists, counts = got
        for qi in range(q.shape[0]):
            e_ids, e_d = oracle.canonical_topk(q[qi], model, 10, O.IP)
            assert int(counts[qi]) == 10
            assert np.array_equal(rows[qi].astype(np.uint32), e_ids), (direction, qi)
            assert np.array_equal(bits(dists[qi]), bits(e_d)), (direction, qi)
    assert idx.coarse_state() == fresh.coarse_state()
    assert idx.sq7_state() == fresh.sq7_state()


def test_update_refits_sq8(L, oracle):
    rng = np.random.default_rng(40)
    n, dim = 3000, 24
    data = rng.random((n, dim), dtype=f32)
    q = rng.random((16, dim), dtype=f32)
    idx = L.FlatIndex(None, dim)
    idx.write(data)
    idx.search_sq8_batch_arrays(q, 10, "l2")
    new = data[[7, 1500]].copy()
    new[0, 3] = -5.0    # moves the minimum of column 3
    data_min_row = int(np.argmin(data[:, 9]))
    rows = [7, data_min_row] if data_min_row != 7 else [7, 1500]
    new[1] = data[rows[1]]
    new[1, 9] = 0.5     # the row that held the minimum of column 9 gives it up: the range SHRINKS (a merged table would keep it)
    idx.update_rows(rows, new)
    model = data.copy()
    model[rows] = new
    fresh = L.FlatIndex(None, dim)
    fresh.write(model)
    for name in ("ip", "l2", "cosine"):
        assert_same_search(idx.search_sq8_batch_arrays(q, 10, name), fresh.search_sq8_batch_arrays(q, 10, name), name)
    for a, b in zip(idx.sq8_params(), fresh.sq8_params()):
        assert np.array_equal(bits(a), bits(b))
    mins, _ = idx.sq8_params()
    assert mins[3] == f32(-5.0) and mins[9] == model[:, 9].min()


def test_update_zero_norm_cosine_and_packed_copy(L, oracle):
    rng = np.random.default_rng(41)
    n, dim = 1500, 70
    data = rng.random((n, dim), dtype=f32)
    idx = L.FlatIndex(None, dim)
    idx.write(data)
    q = rng.random((16, dim), dtype=f32)
    idx.search_batch_arrays(q, 10, "cosine")
    before = idx.search_batch_arrays(q, 10, "hamming")   # the packed copy exists
    new = np.zeros((2, dim), f32)
    new[1] = 1.0 - (data[900] > 0.5)   # every bit of row 900 flips
    idx.update_rows([11, 900], new)
    model = data.copy()
    model[[11, 900]] = new
    assert_searches(L, oracle, idx, model, "zero norm", queries=q)
    rows, dists, counts = idx.search_batch_arrays(q, 10, "hamming")
    for qi in range(16):
        e_ids, e_d = oracle.canonical_topk(q[qi], model, 10, O.HAMMING)
        assert np.array_equal(rows[qi].astype(np.uint32), e_ids) and np.array_equal(bits(dists[qi]), bits(e_d))
    fresh = L.FlatIndex(None, dim)
    fresh.write(model)
    assert np.array_equal(idx.read_packed(0, n), fresh.read_packed(0, n))
    assert before[0].shape == rows.shape


def test_update_f16_shard_rounds_like_append(L, oracle):
    rng = np.random.default_rng(42)
    n, dim = 1000, 130
    data = rng.standard_normal((n, dim)).astype(f32)
    idx = L.FlatIndex(None, dim, dtype="f16")
    idx.write(data)
    rows = rng.choice(n, 50, replace=False)
    new = (rng.standard_normal((50, dim)) * 3).astype(f32)
    new[0, :4] = [65504.0, 1e-7, 6.1e-5, -2049.0]   # the f16 maximum, a value that rounds to a subnormal, near the normal boundary, a tie
    idx.update_rows(rows, new)
    model = data.astype(np.float16).astype(f32)
    model[rows] = new.astype(np.float16).astype(f32)
    got = idx.read_rows(0, n)
    assert np.array_equal(got.astype(np.float16).view(np.uint16), model.astype(np.float16).view(np.uint16))
    assert np.array_equal(bits(got), bits(model))
    assert_searches(L, oracle, idx, model, "f16 update", f16=True)
    assert np.array_equal(bits(idx.gather_rows(rows[::-1])), bits(model[rows[::-1]]))


def test_update_across_a_staging_chunk(L):
    """dim 20,000 x 1000 rows = 80 MB of staged data: more than one 64 MiB chunk"""
    rng = np.random.default_rng(43)
    n, dim = 1000, 20000
    data = rng.standard_normal((n, dim)).astype(f32)
    idx = L.FlatIndex(None, dim)
    idx.write(data)
    rows = rng.permutation(n)
    new = rng.standard_normal((n, dim)).astype(f32)
    idx.update_rows(rows, new)
    model = np.empty_like(data)
    model[rows] = new
    assert np.array_equal(bits(idx.read_rows(0, n)), bits(model))
    pick = np.concatenate([rows[835:842], rows[:3], rows[-3:]])   # both sides of the chunk edge (838 rows per chunk)
    assert np.array_equal(bits(idx.gather_rows(pick)), bits(model[pick]))


def test_update_bad_arguments_leave_the_shard_unchanged(L):
    data = np.random.default_rng(44).standard_normal((200, 12)).astype(f32)
    idx = L.FlatIndex(None, 12)
    idx.write(data)
    new = np.ones((3, 12), f32)
    with pytest.raises(ValueError, match="named twice"):
        idx.update_rows([5, 9, 5], new)
    with pytest.raises(ValueError, match="out of bounds"):
        idx.update_rows([5, 200, 6], new)
    with pytest.raises(ValueError):
        idx.update_rows([5, 6], new)
    assert np.array_equal(bits(idx.read_rows(0, 200)), bits(data))
    idx.update_rows([], np.zeros((0, 12), f32))
    with pytest.raises(ValueError, match="ceil"):
        idx.compact(np.ones(100, bool))
    with pytest.raises(ValueError, match="multiple of 64"):
        idx.compact(np.ones(200, bool), 100)
    assert len(idx) == 200 and np.array_equal(bits(idx.read_rows(0, 200)), bits(data))


def test_update_and_compact_are_refused_in_flight(L):
    import torch

    dev = torch.device("cuda", 0)
    data = np.random.default_rng(45).standard_normal((30_000, 32)).astype(f32)   # (large enough that submit pipelines the batch)
    idx = L.FlatIndex(None, 32)
    idx.write(data)
    idx.finalize()
    idx.search_batch_arrays(data[:8].copy(), 5, "l2")
    idx.prepare("l2", 8)
    q = torch.as_tensor(data[:8].copy(), device=dev)
    out = (torch.zeros((8, 5), dtype=torch.int64, device=dev), torch.zeros((8, 5), dtype=torch.float32, device=dev),
           torch.zeros(8, dtype=torch.int32, device=dev))
    ticket = idx.search_submit(q, 5, "l2", *out)
    keep = np.arange(30_000) % 3 != 0
    try:
        with pytest.raises(ValueError, match="in flight"):
            idx.update_rows([1], np.zeros((1, 32), f32))
        with pytest.raises(ValueError, match="in flight"):
            idx.compact(keep)
    finally:
        ticket.wait()
    assert np.array_equal(out[0].cpu().numpy()[:, 0], np.arange(8))
    idx.update_rows([1], np.zeros((1, 32), f32))
    assert idx.compact(keep) == int(keep.sum())
    model = data.copy()
    model[1] = 0
    assert np.array_equal(bits(idx.read_rows(0, len(idx))), bits(model[keep]))


def test_other_refusals(L):
    packed = L.FlatIndex(None, 64)
    packed.write_packed(np.arange(10, dtype=np.uint64).reshape(10, 1))
    with pytest.raises(NotImplementedError):
        packed.update_rows([1], np.zeros((1, 64), f32))
    with pytest.raises(NotImplementedError):
        packed.compact(np.ones(10, bool))
    with pytest.raises(ValueError):
        packed.gather_rows([1])
    mapped = L.FlatIndex(None, 8)
    mapped.write(np.ones((100, 8), f32))
    mapped.set_row_map(2, 1)
    with pytest.raises(NotImplementedError, match="row-mapped"):
        mapped.compact(np.arange(100) % 2 == 0)
    assert len(mapped) == 100


def test_update_drops_the_auxiliary_indexes(L):
    data = np.random.default_rng(46).standard_normal((600, 32)).astype(f32)
    idx = L.FlatIndex(None, 32)
    idx.write(data)
    idx.build_pq(4, 16)
    idx.build_rabitq()
    idx.build_hnsw("l2", 4, 16, 8)
    idx.build_diskann("l2", 8, 16)
    assert idx.pq_params(False)["n"] == idx.rabitq_params(False)["n"] == idx.hnsw_params(False)["n"] == idx.diskann_params(False)["n"] == 600
    idx.update_rows([3], data[4:5])
    assert idx.pq_params(False)["n"] == idx.rabitq_params(False)["n"] == idx.hnsw_params(False)["n"] == idx.diskann_params(False)["n"] == 0
    idx.build_hnsw("l2", 4, 16, 8)
    idx.compact(np.arange(600) != 9)
    assert idx.hnsw_params(False)["n"] == 0


# ---- gather -----------------------------------------------------------------------------------------------------------------------
def test_gather_rows(L):
    rng = np.random.default_rng(50)
    data = rng.standard_normal((300, 21)).astype(f32)
    idx = L.FlatIndex(None, 21)
    idx.write(data)
    rows = np.array([299, 64, 63, 65, 64, 0, 0, 128, 127, 299], np.uint64)
    assert np.array_equal(bits(idx.gather_rows(rows)), bits(data[rows.astype(np.int64)]))
    assert np.array_equal(bits(idx.gather_rows(np.arange(299, -1, -1))), bits(data[::-1]))
    assert idx.gather_rows([]).shape == (0, 21)
    with pytest.raises(ValueError, match="out of bounds"):
        idx.gather_rows([3, 300])
    h = L.FlatIndex(None, 21, dtype="f16")
    h.write(data)
    assert np.array_equal(bits(h.gather_rows(rows)), bits(data.astype(np.float16).astype(f32)[rows.astype(np.int64)]))


# ---- Collection -------------------------------------------------------------------------------------------------------------------
DIM = 32


@pytest.fixture(scope="module")
def scenario():
    """600 rows (ids 1000...), 50 deleted, an upsert of 100 existing ids (5 of them tombstoned) and 30 new ones, a compaction"""
    rng = np.random.default_rng(60)
    base = rng.standard_normal((600, DIM)).astype(f32)
    ids = np.arange(1000, 1600, dtype=np.int64)
    perm = rng.permutation(600)
    dead = ids[perm[:50]]
    up_ids = np.concatenate([dead[:5], ids[perm[50:145]], np.arange(5000, 5030)])
    rng.shuffle(up_ids)
    up_vecs = rng.standard_normal((130, DIM)).astype(f32)
    rows, all_ids = np.concatenate([base, up_vecs[up_ids >= 5000]]), np.concatenate([ids, up_ids[up_ids >= 5000]])
    old = up_ids < 5000
    rows[up_ids[old] - 1000] = up_vecs[old]
    still_dead = dead[5:]
    live = ~np.isin(all_ids, still_dead)
    queries = rng.standard_normal((16, DIM)).astype(f32)
    queries[0] = rows[live][17]
    return {"base": base, "ids": ids, "dead": dead, "up_ids": up_ids, "up_vecs": up_vecs, "final_rows": rows[live], "final_ids": all_ids[live],
            "queries": queries}


def run_scenario(L, s, mode, params, fields=None, up_fields=None):
    c = L.Collection("mutated", DIM)
    c.add_items(s["base"], s["ids"].tolist(), fields)
    c.commit()
    c.build_index(mode, params)
    c.delete_items(s["dead"].tolist())
    c.upsert_items(s["up_vecs"], s["up_ids"].tolist(), up_fields)
    return c


def assert_same_results(a, b, tag):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.array_equal(x.ids(), y.ids()), tag
        assert np.array_equal(bits(x.distances()), bits(y.distances())), tag


@pytest.mark.parametrize("mode,params", [("FLAT-IP", None), ("FLAT-L2-SQ8", None), ("FLAT-COS-PQ", {"n_clusters": 16}), ("FLAT-IP-RABITQ", None),
                                         ("IVF-IP", {"n_clusters": 8}), ("SPANN-L2", {"n_clusters": 8}), ("HNSW-L2", None), ("DISKANN-L2", None)])
def test_collection_upsert_and_compact_equal_a_fresh_collection(L, scenario, mode, params):
    s = scenario
    c = run_scenario(L, s, mode, params)
    assert sorted(c.list_deleted_ids()) == sorted(s["dead"][5:].tolist()) and c.shape() == (630, DIM)
    assert c.compact() == 45
    fresh = L.Collection("fresh", DIM)
    fresh.add_items(s["final_rows"], s["final_ids"].tolist())
    fresh.commit()
    fresh.build_index(mode, params)
    assert c.shape() == fresh.shape() == (585, DIM)
    assert c.list_deleted_ids() == [] and c.compact() == 0
    assert_same_results(c.batch_search(s["queries"], 10), fresh.batch_search(s["queries"], 10), mode)
    assert_same_results([c.search(q, 7) for q in s["queries"][:3]], [fresh.search(q, 7) for q in s["queries"][:3]], mode)
    pick = s["final_ids"][::-7]
    assert np.array_equal(bits(c.read_vectors_by_ids(pick.tolist())), bits(s["final_rows"][::-7]))
    if mode.startswith("HNSW"):
        g, e = c._flat.hnsw_params(), fresh._flat.hnsw_params()
        assert g["n"] == 585 and all(np.array_equal(g[key], e[key]) for key in e if isinstance(e[key], np.ndarray))
        assert {key: v for key, v in g.items() if not isinstance(v, np.ndarray)} == {key: v for key, v in e.items() if not isinstance(v, np.ndarray)}
    if mode.startswith("DISKANN"):
        g, e = c._flat.diskann_params(), fresh._flat.diskann_params()
        assert g["n"] == 585 and np.array_equal(g["adj"], e["adj"]) and g["entry"] == e["entry"]
    if mode.endswith("PQ"):
        g, e = c._flat.pq_params(), fresh._flat.pq_params()
        assert g["n"] == 585 and g["K"] == e["K"] == 16   # (the cluster count of the build is kept for the rebuild)
        assert np.array_equal(g["codebooks"], e["codebooks"]) and np.array_equal(g["codes"], e["codes"])


def test_collection_sparse_and_text_follow(L, scenario):
    s = scenario
    words = ["alpha", "beta", "gamma", "delta", "epsilon", "zeta", "eta"]
    doc = lambda i, tag: {"body": f"{words[i % 7]} {words[(i * 3) % 7]} common {tag}", "n": i}   # noqa: E731
    sparse = lambda i: {int(i % 50): 1.0, int((i * 7) % 50 + 50): 0.5}   # noqa: E731
    fields = [doc(int(i), "old") for i in s["ids"]]
    up_fields = [doc(int(i), "new") for i in s["up_ids"]]
    c = L.Collection("mutated", DIM)
    c.add_items(s["base"], s["ids"].tolist(), fields)
    c.commit()
    c.add_sparse_vectors([sparse(i) for i in s["ids"]], s["ids"].tolist())
    c.build_index("FLAT-L2", None)
    c.search_sparse({3: 1.0}, 5)
    c.text_search("alpha common", None, 5)   # both device stores exist before the mutation
    c.delete_items(s["dead"].tolist())
    c.upsert_items(s["up_vecs"], s["up_ids"].tolist(), up_fields)
    assert c.compact() == 45
    final_fields = []
    up_at = {int(i): j for j, i in enumerate(s["up_ids"])}
    for i in s["final_ids"].tolist():
        final_fields.append(up_fields[up_at[i]] if i in up_at else doc(i, "old"))
    fresh = L.Collection("fresh", DIM)
    fresh.add_items(s["final_rows"], s["final_ids"].tolist(), final_fields)
    fresh.commit()
    had_sparse = s["final_ids"][s["final_ids"] < 5000]
    fresh.add_sparse_vectors([sparse(i) for i in had_sparse], had_sparse.tolist())
    fresh.build_index("FLAT-L2", None)
    assert c.sparse_len() == fresh.sparse_len() == had_sparse.size and c.text_len() == fresh.text_len() == 585
    q = s["queries"]
    for sv in ({3: 1.0, 57: 2.0}, {10: 0.5}, {49: 1.0, 99: 1.0}):
        assert_same_results([c.search_sparse(sv, 10)], [fresh.search_sparse(sv, 10)], "sparse")
    for text in ("alpha common", "new", "old gamma", "zeta eta new"):
        assert_same_results([c.text_search(text, None, 10)], [fresh.text_search(text, None, 10)], text)
        assert_same_results([c.hybrid_search(q[1], text, 10)], [fresh.hybrid_search(q[1], text, 10)], text)
    assert_same_results(c.batch_search(q, 10), fresh.batch_search(q, 10), "dense")


def test_collection_error_cases(L, scenario):
    s = scenario
    c = L.Collection("errors", DIM)
    c.add_items(s["base"][:100], s["ids"][:100].tolist())
    c.commit()
    before = c._flat.read_rows(0, 100)
    with pytest.raises(RuntimeError, match="id 77 does not exist; use upsert_items to insert missing IDs"):
        c.update_items(s["base"][:2], [1000, 77])
    with pytest.raises(RuntimeError, match="duplicate id 1003 within the same insert batch"):
        c.upsert_items(s["base"][:3], [1003, 1004, 1003])
    with pytest.raises(RuntimeError, match="duplicate id 1003 within the same insert batch"):
        c.update_items(s["base"][:3], [1003, 1004, 1003])
    with pytest.raises(RuntimeError, match="vector id 9 does not exist"):
        c.read_vectors_by_ids([1000, 9])
    with pytest.raises(RuntimeError, match="Dimension mismatch"):
        c.upsert_items(np.zeros((1, DIM + 1), f32), [1000])
    assert c.shape() == (100, DIM) and np.array_equal(bits(c._flat.read_rows(0, 100)), bits(before))
    assert c.compact() == 0 and c.shape() == (100, DIM)
    c.update_items(s["base"][200:202], [1001, 1000])
    assert np.array_equal(bits(c.read_vectors_by_ids([1000, 1001])), bits(s["base"][[201, 200]]))
    # pending rows are served from the buffer
    c.add_items(s["base"][300:303], [7000, 7001, 7002])
    assert c.pending_len() == 3
    assert np.array_equal(bits(c.read_vectors_by_ids([7001, 1000])), bits(s["base"][[301, 201]]))
    # this mirror's add_items accepts an id twice: the mutation calls name the id, compact removes every row of it
    c.add_items(s["base"][400:401], [1005])
    c.commit()
    for call in (lambda: c.upsert_items(s["base"][:1], [1005]), lambda: c.update_items(s["base"][:1], [1005]), lambda: c.read_vectors_by_ids([1005])):
        with pytest.raises(RuntimeError, match="id 1005 is stored in more than one row"):
            call()
    c.delete_items([1005, 424242])   # (an id without a row is simply forgotten)
    assert c.compact() == 2 and c.shape() == (102, DIM) and c.list_deleted_ids() == []
    with pytest.raises(RuntimeError, match="vector id 1005 does not exist"):
        c.read_vectors_by_ids([1005])
