"""`-m gpu`: update_rows / compact against every derived copy and every scan path that reads one (lynsedb_amd/csrc/mutate_host.inc,
reset_derived_locked).  tests/test_gpu_mutation.py checks the row bits, the plan and the Collection glue; here every case
  1. builds the copies its path reads BEFORE the mutation and asserts that they exist,
  2. mutates,
  3. searches, and asserts from the profile that the intended path answered.
A copy that survived the mutation does not crash: the coarse pass proposes candidates from rows that no longer sit where the copy says and the
exact rescoring returns a plausible, wrong top-k.  So every comparison is exact — ids, f32 distance bits, counts — against a FRESH handle given
the final rows and against the CPU oracle for every query of every batch, and the code sets are compared through sq8_params(), coarse_state()
and sq7_state().  The shards, the model of the final rows and the planted queries come from tests/mutation_common.py;
tests/test_mutation_paths_design.py proves on the CPU that the stale layout would answer them differently.

Observables (include/lynse_hip.h): `last_plan` bit 2 the certified int8 pass, bit 4 the <= 32-query kernel, bit 5 k_small_search, bits 16..23
the tiling (0x82 k_scan_qh, 0x24 / 0x42 the 256-query f16 tilings), bit 26 SQ7; coarse_state()["sq8_rows"] / ["bpm_rows"]; sq7_state();
hbm_bytes() (grows when an owned shadow is built).  Without an observable: n16 (the rows the shadow covers) and n_stats, the aliased shadow of an
F16 shard (no bytes of its own), the range scratch, and whether search_submit pipelined a batch or answered it inside the call — those cases
say so and rely on the searches that ran before the mutation."""
import os

import numpy as np
import pytest

import mutation_common as M
import oracle as O
from conftest import oracle_for_every_query

pytestmark = pytest.mark.gpu
f32 = np.float32
PLAN_I8C, PLAN_SMALL, PLAN_FUSED, PLAN_SQ7 = 4, 16, 32, 1 << 26
NQ_MFMA = 72   # the batch floor of Hamming on the matrix path (bin_mfma_minq)


@pytest.fixture(scope="module")
def L():
    import lynsedb_amd as L_

    assert L_._lib.device_count() >= 1
    return L_


def plan(p):
    return int(p["last_plan"])


def tiling(p):
    return (plan(p) >> 16) & 0xff


def on_int8(p, metric=None):
    return bool(plan(p) & PLAN_I8C) and p["fallback_queries"] == 0


def on_f16_256(p, metric):
    """the 256 x 256 tile of the f16 shadow: <2,4,4,2> for IP, <4,2,2,4> for L2 / cosine"""
    return not plan(p) & (PLAN_I8C | PLAN_SMALL | PLAN_FUSED) and tiling(p) == (0x24 if metric == "ip" else 0x42)


def on_small(p, metric=None):
    return bool(plan(p) & PLAN_SMALL) and not plan(p) & (PLAN_FUSED | PLAN_I8C)


def on_fused(p, metric=None):
    return bool(plan(p) & PLAN_FUSED)


def on_qh(p, metric=None):
    return tiling(p) == 0x82 and not plan(p) & PLAN_I8C and p["fallback_queries"] == 0


def on_sq7(p, metric=None):
    return bool(plan(p) & PLAN_SQ7) and bool(plan(p) & PLAN_I8C) and p["fallback_queries"] == 0


def index_of(L, rows, f16=False, reserve=0):
    idx = L.FlatIndex(None, rows.shape[1], dtype="f16" if f16 else "f32")
    if reserve:
        idx.reserve(reserve)
    idx.write(rows)
    idx.profile_enable(True)
    return idx


def profiled(idx, call):
    idx.profile_get(reset=True)
    out = call()
    return out, idx.profile_get(reset=True)


def search(idx, q, k, metric, sq7=False):
    """one profiled blocking batch (sq7: with LYNSE_HIP_SQ7=1 around the call) -> ((rows, dists, counts), profile)"""
    old = os.environ.pop("LYNSE_HIP_SQ7", None)
    if sq7:
        os.environ["LYNSE_HIP_SQ7"] = "1"
    try:
        return profiled(idx, lambda: idx.search_batch_arrays(q, k, metric))
    finally:
        os.environ.pop("LYNSE_HIP_SQ7", None)
        if old is not None:
            os.environ["LYNSE_HIP_SQ7"] = old


def gathered(call):
    """the call with LYNSE_HIP_FILTER_STRATEGY=1 (read per call): the subset filter gathers the listed shadow rows instead of masking the scan"""
    old = os.environ.pop("LYNSE_HIP_FILTER_STRATEGY", None)
    os.environ["LYNSE_HIP_FILTER_STRATEGY"] = "1"
    try:
        return call()
    finally:
        del os.environ["LYNSE_HIP_FILTER_STRATEGY"]
        if old is not None:
            os.environ["LYNSE_HIP_FILTER_STRATEGY"] = old


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same(a, b, tag):
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])), tag


def assert_exact(got, want, tag):
    rows, dists, counts = got
    for qi, (e_ids, e_d) in enumerate(want):
        c = int(counts[qi])
        assert c == len(e_ids), (tag, qi, c, len(e_ids))
        assert np.array_equal(rows[qi, :c].astype(np.uint64), e_ids.astype(np.uint64)), (tag, qi, rows[qi, :c], e_ids)
        assert np.array_equal(bits(dists[qi, :c]), bits(e_d)), (tag, qi, dists[qi, :c], e_d)


_wanted = {}


def wanted(oracle, key, rows, q, k, metric, f16=False):
    """the oracle's answer to every query of the batch; computed once per key (case, state, batch, k, metric) and shared"""
    if key not in _wanted:
        _wanted[key] = oracle_for_every_query(lambda i: M.oracle_topk(oracle, q[i], rows, k, metric, f16), q.shape[0])
    return _wanted[key]


def check(oracle, idx, fresh, rows, q, k, metric, path, key, f16=False, sq7=False):
    """the batch on `idx`: the path asserted from the profile, the answer equal to the fresh handle's and to the oracle's for every query"""
    got, p = search(idx, q, k, metric, sq7)
    assert path(p, metric), (key, metric, hex(plan(p)), p)
    exp, _ = search(fresh, q, k, metric, sq7)
    assert_same(got, exp, (key, metric, "fresh handle"))
    assert_exact(got, wanted(oracle, key + (q.shape[0], k, metric), rows, q, k, metric, f16), (key, metric))
    return got


def assert_code_sets_equal(idx, fresh, tag, params=True):
    assert idx.coarse_state() == fresh.coarse_state(), (tag, idx.coarse_state(), fresh.coarse_state())
    assert idx.sq7_state() == fresh.sq7_state(), (tag, idx.sq7_state(), fresh.sq7_state())
    if params:
        for a, b in zip(idx.sq8_params(), fresh.sq8_params()):
            assert np.array_equal(bits(a), bits(b)), tag


def assert_planted(c, got, final, tag):
    """(c) queries find their appended rows; (b) queries no longer find the content that was deleted or overwritten"""
    rows = got[0]
    for j, qi in enumerate(c.slots("c")):
        assert int(rows[qi, 0]) == int(c.src_c[j]), (tag, "c", qi, rows[qi, :3])
    for j, qi in enumerate(c.slots("b")):
        assert not np.array_equal(final[int(rows[qi, 0])], c.q_b[j]), (tag, "b", qi, rows[qi, :3])


APPENDS = [("compact", "inside"), ("compact", "regrow"), ("update", "inside"), ("update", "regrow")]


def append_plan(c, kind, append):
    """-> (rows to reserve up front, rows appended after the mutation): an update leaves no free capacity, so its short append needs a reserve"""
    s = c.spec
    n_app = s.n_inside if append == "inside" else s.n_append
    return (s.n0 + s.n_inside if (kind == "update" and append == "inside") else 0), n_app


# ---- 1. int8 IP: a compaction that stays above the threshold of the pass, one that falls below it; an update -----------------------
@pytest.mark.parametrize("kind,append", APPENDS)
def test_int8_ip_codes_follow_the_mutation(L, oracle, kind, append):
    """72,000 x 32 (ld16 = 32: k_scan_qh does not take the batch), 256 and 40 queries.  Pins the SQ8 codes (sq8_rows, sq8_params, the fit
    counters through coarse_state) and `last_plan` bit 2 before the mutation, after it on freshly fitted codes, after an append (inside the old
    capacity / across a regrow: the merge of new rows into rebuilt codes); then a compaction to ~40,000 rows: the 256-query f16 tiling (bits 2 and 4
    clear, tiling 0x24) answers and sq8_rows is 0.  The f16 shadow the last step reads has no observable of its row count (n16)."""
    c = M.case(f"ip32_{kind}")
    s = c.spec
    reserve, n_app = append_plan(c, kind, append)
    idx = index_of(L, c.base, reserve=reserve)
    batches = [c.batch(256), c.batch(40)]
    for q in batches:
        _, p = search(idx, q, 10, "ip")
        assert on_int8(p), hex(plan(p))
    assert idx.coarse_state()["sq8_rows"] == s.n0
    assert c.mutate(idx) == c.after.shape[0] == len(idx)
    assert idx.coarse_state()["sq8_rows"] == 0
    fresh = index_of(L, c.after)
    for q in batches:
        check(oracle, idx, fresh, c.after, q, 10, "ip", on_int8, (s.name, "after"))
    assert idx.coarse_state()["sq8_rows"] == len(idx)
    assert_code_sets_equal(idx, fresh, (s.name, "after"))
    # mutate -> search -> append -> search
    final = c.final(n_app)
    idx.write(c.more[:n_app])
    fresh = index_of(L, final)
    for q in batches:
        got = check(oracle, idx, fresh, final, q, 10, "ip", on_int8, (s.name, "appended", n_app))
        assert_planted(c, got, final, (s.name, append))
    assert idx.coarse_state()["sq8_rows"] == final.shape[0] == len(idx)
    assert_code_sets_equal(idx, fresh, (s.name, "appended", append))
    # below 65,536 rows: the f16 shadow, no codes
    keep = np.random.default_rng(s.seed + 5).random(final.shape[0]) < 0.55
    keep[0] = False
    assert idx.compact(keep) == int(keep.sum()) < 65_536
    below = final[keep]
    fresh = index_of(L, below)
    for q in batches:
        check(oracle, idx, fresh, below, q, 10, "ip", on_f16_256 if q.shape[0] > 64 else (lambda p, m: not plan(p) & (PLAN_I8C | PLAN_FUSED)),
              (s.name, "below", append))
    assert idx.coarse_state()["sq8_rows"] == 0
    assert_code_sets_equal(idx, fresh, (s.name, "below"), params=False)


# ---- 2. plain-L2 codes + exact norms, unit-row cosine codes, SQ7 ---------------------------------------------------------------------
@pytest.mark.parametrize("kind,append", [("compact", "inside"), ("update", "regrow")])
def test_int8_l2_cosine_and_sq7_codes_follow_the_mutation(L, oracle, kind, append):
    """72,000 x 256, 256 and 40 queries of l2 and cosine (bit 2: the codes of the rows with the exact row norms, the codes of the unit rows),
    then IP with 256 queries under LYNSE_HIP_SQ7=1 (bit 26).  The update overwrites the rows of largest and smallest norm, so vmax / vmin (and
    eps2 of the unit-row codes) move; the compaction keeps each row with probability 0.92.  The augmented L2 codes are pinned by the masked scan
    of test_filters_and_large_k_after_a_compaction.  (Rows of both signs: an SQ7 copy is freed by the next batch that does not force it — it is
    compared right after its own search.)"""
    c = M.case(f"d256_{kind}")
    s = c.spec
    reserve, n_app = append_plan(c, kind, append)
    idx = index_of(L, c.base, reserve=reserve)
    q256, q40 = c.batch(256), c.batch(40)

    def all_paths(idx, fresh, rows, state):
        for metric in ("l2", "cosine"):
            for q in (q256, q40):
                got = check(oracle, idx, fresh, rows, q, 10, metric, on_int8, (s.name, state))
                if state != "after":
                    assert_planted(c, got, rows, (s.name, state, metric))
        assert_code_sets_equal(idx, fresh, (s.name, state))
        check(oracle, idx, fresh, rows, q256, 10, "ip", on_sq7, (s.name, state), sq7=True)
        assert idx.sq7_state() == {"sq7_rows": rows.shape[0], "sq7_strikes": 0}
        assert_code_sets_equal(idx, fresh, (s.name, state, "sq7"))

    for metric in ("l2", "cosine"):
        for q in (q256, q40):
            _, p = search(idx, q, 10, metric)
            assert on_int8(p), (metric, hex(plan(p)))
    _, p = search(idx, q256, 10, "ip", sq7=True)
    assert on_sq7(p), hex(plan(p))
    assert idx.coarse_state()["sq8_rows"] == s.n0 and idx.sq7_state()["sq7_rows"] == s.n0
    assert c.mutate(idx) == c.after.shape[0]
    assert idx.coarse_state()["sq8_rows"] == 0 and idx.sq7_state()["sq7_rows"] == 0
    all_paths(idx, index_of(L, c.after), c.after, "after")
    final = c.final(n_app)
    idx.write(c.more[:n_app])
    all_paths(idx, index_of(L, final), final, ("appended", n_app))


# ---- 3. batched Hamming on the FP4 copy -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,append", [("compact", "inside"), ("update", "regrow"), ("compact", "regrow")])
def test_fp4_hamming_copy_follows_the_mutation(L, oracle, kind, append):
    """72,000 x 256 rows uniform in [0, 1) (a bit is set where x > 0.5), 72 queries = bin_mfma_minq(): bpm_rows is n0 before the mutation, 0
    after it and the new n after the search; the packed words equal a fresh handle's."""
    c = M.case(f"ham256_{kind}")
    s = c.spec
    reserve, n_app = append_plan(c, kind, append)
    idx = index_of(L, c.base, reserve=reserve)
    q = c.batch(NQ_MFMA)
    search(idx, q, 10, "hamming")
    assert idx.coarse_state()["bpm_rows"] == s.n0
    assert c.mutate(idx) == c.after.shape[0]
    assert idx.coarse_state()["bpm_rows"] == 0
    for rows, state in ((c.after, "after"), (None, "appended")):
        if rows is None:
            rows = c.final(n_app)
            idx.write(c.more[:n_app])
        fresh = index_of(L, rows)
        got = check(oracle, idx, fresh, rows, q, 10, "hamming", lambda p, m: bool(plan(p) & PLAN_I8C), (s.name, state, n_app if state == "appended" else 0))
        n = rows.shape[0]
        assert idx.coarse_state()["bpm_rows"] == n == len(idx) and fresh.coarse_state()["bpm_rows"] == n
        assert np.array_equal(idx.read_packed(0, n), fresh.read_packed(0, n)), (s.name, state)
        if state == "appended":
            assert_planted(c, got, rows, (s.name, append))


# ---- 4. k_scan_qh over the f16 shadow ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["qh64_compact", "qh100_compact", "qh100_f16_compact"])
def test_qh_shadow_follows_a_compaction_and_an_update(L, oracle, name):
    """20,000 x 64 and 20,000 x 100 (ld16 = 128, padded), IP, 64 queries: tiling 0x82 before, after the compaction and after an update of the
    compacted shard.  The f32 shards own their shadow (hbm_bytes grows by it); the F16 shard's shadow is an alias of its rows (no bytes, no
    observable): there the padded half-pitch goes through k_compact_rows and k_scatter_rows<_Float16>."""
    c = M.case(name)
    s = c.spec
    idx = index_of(L, c.base, f16=s.f16)
    q = c.batch(64)
    before = idx.hbm_bytes()
    _, p = search(idx, q, 10, "ip")
    assert on_qh(p), hex(plan(p))
    ld16 = -(-s.dim // 64) * 64
    if not s.f16:
        assert idx.hbm_bytes() >= before + s.n0 * ld16 * 2
    assert c.mutate(idx) == c.after.shape[0]
    fresh = index_of(L, c.after, f16=s.f16)
    check(oracle, idx, fresh, c.after, q, 10, "ip", on_qh, (name, "after"), f16=s.f16)
    rng = np.random.default_rng(s.seed + 9)
    model = M.RowModel(s.dim, s.f16)
    model.rows = c.after
    rows = rng.choice(len(model), 150, replace=False)
    new = M.centred(rng, 150, s.dim)
    new[:4] = c.q_a * f32(1.25)       # the (a) queries now have a better row under IP than the one they copy
    model.update(rows, new)
    idx.update_rows(rows, new)
    assert np.array_equal(bits(idx.read_rows(0, len(model))), bits(model.rows))
    fresh = index_of(L, model.rows, f16=s.f16)
    got = check(oracle, idx, fresh, model.rows, q, 10, "ip", on_qh, (name, "updated"), f16=s.f16)
    assert sorted(int(r) for r in got[0][:4, 0]) == sorted(int(r) for r in rows[:4])


# ---- 5. the <= 32-query tiling over an owned shadow that existed before the mutation -------------------------------------------------
@pytest.mark.parametrize("fused", [True, False], ids=["fused_on", "fused_off"])
@pytest.mark.parametrize("kind,append", APPENDS)
def test_small_batch_tiling_with_a_shadow_built_before(L, oracle, kind, append, fused):
    """5,000 x 128 f32, 16 queries: bit 4 set and bit 5 clear for l2 / ip / cosine, the owned shadow built before the mutation (hbm_bytes grew by
    n x ld16 halves).  With the fused search on, a 3-query batch is answered by k_small_search (bit 5), which reads the f32 rows only."""
    c = M.case(f"small128_{kind}")
    s = c.spec
    reserve, n_app = append_plan(c, kind, append)
    idx = index_of(L, c.base, reserve=reserve)
    idx.set_fused_search(fused)
    q = c.batch(16)
    before = idx.hbm_bytes()
    for metric in s.metrics:
        _, p = search(idx, q, 10, metric)
        assert on_small(p), (metric, hex(plan(p)))
    assert idx.hbm_bytes() >= before + s.n0 * 128 * 2
    assert c.mutate(idx) == c.after.shape[0]
    for rows, state in ((c.after, "after"), (None, "appended")):
        if rows is None:
            rows = c.final(n_app)
            idx.write(c.more[:n_app])
        fresh = index_of(L, rows)
        fresh.set_fused_search(fused)
        for metric in s.metrics:
            got = check(oracle, idx, fresh, rows, q, 10, metric, on_small, (s.name, state, n_app if state == "appended" else 0))
            if state == "appended":
                assert_planted(c, got, rows, (s.name, append, metric))
        check(oracle, idx, fresh, rows, q[:3], 5, "l2", on_fused if fused else on_small, (s.name, state, "q3", n_app if state == "appended" else 0))


# ---- 6. filters and a large k after a compaction --------------------------------------------------------------------------------------
def filtered_want(oracle, rows, q, k, metric, subset):
    return oracle_for_every_query(lambda i: oracle.canonical_topk_filtered(q[i], rows, k, M.METRIC_IDS[metric], subset), q.shape[0])


def test_filters_and_large_k_after_a_compaction(L, oracle):
    """The 72,000 x 256 shard, >= 65,536 rows after the compaction.  A BitSet over half of the rows with 40 queries: the masked int8 scan (bit 2;
    l2 reads the augmented codes, cosine the unit-row codes, ip the plain ones).  A subset of 300 rows: at this size the cost model still masks the
    scan, so the gathered rows are reached with LYNSE_HIP_FILTER_STRATEGY=1 (bit 2 clear, fewer rows scanned than the shard holds), and the
    subset is also sent without it.  k = 4,200 > cap / 4: search_large_k, one inner search per range of cap = 16,384 rows (profile `searches`).  All three before
    and after, the subsets in the new numbering."""
    c = M.case("d256_compact")
    s = c.spec
    idx = index_of(L, c.base)
    q = c.batch(40)
    rng = np.random.default_rng(s.seed + 11)

    def run_all(idx, rows, fresh, state):
        n = rows.shape[0]
        half = np.sort(rng.choice(n, n // 2, replace=False))
        half = np.union1d(half, np.arange(n - 70, n))          # the last rows of the shard are in: beyond them the kept buffers hold old rows
        words = L.BitSet.from_rows(half, n).words
        few = np.sort(np.concatenate([rng.choice(n - 300, 290, replace=False), np.arange(n - 10, n)]))
        for metric in ("ip", "l2", "cosine"):
            got, p = profiled(idx, lambda: idx.search_filtered_bitset_batch_arrays(q, 10, metric, words))
            assert on_int8(p), (state, metric, hex(plan(p)))
            assert_exact(got, filtered_want(oracle, rows, q, 10, metric, half), (state, "bitset", metric))
            got2, p = gathered(lambda: profiled(idx, lambda: idx.search_filtered_batch_arrays(q, 10, metric, few)))
            assert not plan(p) & PLAN_I8C and 0 < p["scan_rows"] < n, (state, metric, hex(plan(p)), p)
            want_few = filtered_want(oracle, rows, q, 10, metric, few)
            assert_exact(got2, want_few, (state, "gathered", metric))
            got3, p = profiled(idx, lambda: idx.search_filtered_batch_arrays(q, 10, metric, few))     # (the strategy the cost model picks)
            assert_exact(got3, want_few, (state, "short subset", metric, hex(plan(p))))
            if fresh is not None:
                assert_same(got, fresh.search_filtered_bitset_batch_arrays(q, 10, metric, words), (state, "bitset", metric))
                assert_same(got2, gathered(lambda: fresh.search_filtered_batch_arrays(q, 10, metric, few)), (state, "gathered", metric))
        got, p = profiled(idx, lambda: idx.search_batch_arrays(q[:3], 4_200, "l2"))
        assert p["searches"] == -(-n // 16_384), p
        assert_exact(got, wanted(oracle, (s.name, state, "large k"), rows, q[:3], 4_200, "l2"), (state, "large k"))
        if fresh is not None:
            assert_same(got, fresh.search_batch_arrays(q[:3], 4_200, "l2"), (state, "large k"))

    run_all(idx, c.before, None, "before")
    assert idx.coarse_state()["sq8_rows"] == s.n0
    assert c.mutate(idx) == c.after.shape[0] >= 65_536
    run_all(idx, c.after, index_of(L, c.after), "after")


# ---- 7. range search and the additive metrics ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def additive_ref(tmp_path_factory):
    from additive_common import build_ref

    return build_ref(tmp_path_factory.mktemp("additive_ref"))


@pytest.mark.parametrize("name", ["range27_compact", "range27_update", "range27_f16_compact", "range27_f16_update"])
def test_range_search_and_additive_metrics_after_a_mutation(L, oracle, additive_ref, name):
    """3,000 x 27, f32 and F16.  The range scratch (sized for the old length; no observable) and the additive scan existed before the mutation.
    After it: range search under ip / l2 / cosine against the oracle's distances to every row, under L1 and Canberra against tests/additive_ref,
    and on the f32 shard the top-k of the four additive metrics (an F16 shard refuses it) — each also against a fresh handle."""
    import test_gpu_additive_metrics as A
    import test_gpu_range_search as R
    from additive_common import BRAY, CANB, CHEB, L1, NAME

    c = M.case(name)
    s = c.spec
    idx = index_of(L, c.base, f16=s.f16)
    q = c.batch(12)
    first = idx.search_range_batch_arrays(q, np.full(12, 1.0, f32), 50, "l2")
    idx.search_range_batch_arrays(q, np.full(12, 5.0, f32), 50, "l1")
    if not s.f16:
        idx.search_batch_arrays(q, 10, "l1")
    assert int(first[3].max()) >= 1                                 # the scan ran over the old rows: the planted copies pass at distance 0
    assert c.mutate(idx) == c.after.shape[0]
    rows = c.after
    fresh = index_of(L, rows, f16=s.f16)
    n = rows.shape[0]
    for metric in (O.IP, O.L2, O.COS):
        case = R.Case(q, R.all_dists(oracle, q, rows, metric), metric)
        thr = np.array([case.D[i][case.order[i]][[0, 3, 40, 400, n - 1, 7][i % 6]] for i in range(12)], f32)
        for cap in (25, n + 5):
            got = idx.search_range_batch_arrays(q, thr, cap, R.NAME[metric])
            R.check(got, case, thr, cap)
            exp = fresh.search_range_batch_arrays(q, thr, cap, R.NAME[metric])
            assert all(np.array_equal(bits(a) if a.dtype == f32 else a, bits(b) if b.dtype == f32 else b) for a, b in zip(got, exp)), (name, metric, cap)
    for m in (L1, CANB):
        raw = additive_ref.raw_dists(m, q, rows)
        thr = np.array([np.sort(raw[i])[[0, 3, 40, 400, n - 1, 7][i % 6]] for i in range(12)], f32)
        for cap in (25, n + 5):
            got = idx.search_range_batch_arrays(q, thr, cap, NAME[m])
            A.check_range(got, raw, thr, cap)
            exp = fresh.search_range_batch_arrays(q, thr, cap, NAME[m])
            assert all(np.array_equal(bits(a) if a.dtype == f32 else a, bits(b) if b.dtype == f32 else b) for a, b in zip(got, exp)), (name, m, cap)
    if not s.f16:
        for m in (L1, CHEB, CANB, BRAY):
            got = idx.search_batch_arrays(q, 10, NAME[m])
            A.check_batch(got, additive_ref.dists(m, q, rows), 10, what=(name, m))
            assert_same(got, fresh.search_batch_arrays(q, 10, NAME[m]), (name, m))


# ---- 8. search_submit on a handle prepared and searched before the mutation ----------------------------------------------------------
@pytest.mark.parametrize("prepare_again", [False, True], ids=["no_prepare", "prepare"])
@pytest.mark.parametrize("kind", ["compact", "update"])
def test_search_submit_after_a_mutation(L, oracle, kind, prepare_again):
    """30,000 x 32, 8 queries of l2 (large enough that submit pipelines the batch: test_gpu_mutation.py).  The handle was prepared, searched and
    had a ticket answered before the mutation; afterwards a ticket — without and with a new prepare — equals the blocking search of a fresh
    handle and the oracle.  Whether submit pipelined the batch or answered it inside the call has no observable; bit 4 tells the tiling."""
    import torch

    dev = torch.device("cuda", 0)
    c = M.case(f"submit_{kind}")
    s = c.spec
    idx = index_of(L, c.base)
    q = c.batch(8)
    dq = torch.as_tensor(q, device=dev)

    def submit():
        out = (torch.zeros((8, 10), dtype=torch.int64, device=dev), torch.zeros((8, 10), dtype=torch.float32, device=dev),
               torch.zeros(8, dtype=torch.int32, device=dev))
        (_, p) = profiled(idx, lambda: idx.search_submit(dq, 10, "l2", *out).wait())
        torch.cuda.synchronize()
        return (out[0].cpu().numpy().astype(np.uint64), out[1].cpu().numpy(), out[2].cpu().numpy().astype(np.uint32)), p

    idx.finalize()
    idx.search_batch_arrays(q, 10, "l2")
    idx.prepare("l2", 8)
    got, p = submit()
    assert on_small(p) and p["searches"] == 1, p
    assert_exact(got, wanted(oracle, (s.name, "before", 8, 10, "l2"), c.before, q, 10, "l2"), (s.name, "before"))
    assert c.mutate(idx) == c.after.shape[0]
    if prepare_again:
        idx.prepare("l2", 8)
    got, p = submit()
    assert on_small(p) and p["searches"] == 1, p
    fresh = index_of(L, c.after)
    assert_same(got, tuple(x.astype(t) for x, t in zip(fresh.search_batch_arrays(q, 10, "l2"), (np.uint64, f32, np.uint32))), (s.name, "fresh"))
    assert_exact(got, wanted(oracle, (s.name, "after", 8, 10, "l2"), c.after, q, 10, "l2"), (s.name, "after"))
    got2, _ = submit()       # and once more, now on derived data the first ticket left behind
    assert_same(got, got2, (s.name, "second ticket"))


# ---- 10. F16 shard: the shadow between an alias of the rows and a buffer of its own ---------------------------------------------------
def test_f16_alias_transitions(L, oracle):
    """2,000 x 130 on an F16 shard, 16 queries, l2 / ip / cosine after each step (bit 4: the <= 32-query kernel; F16 shards never take the fused
    one).  1: a row gets a 40,000, so sv leaves 1 and the shadow becomes an owned buffer (hbm_bytes grows by it); 2: a compaction in that state;
    3: the row goes back to a small value, the shadow is an alias again (hbm_bytes falls back); 4: a compaction in the aliased state."""
    rng = np.random.default_rng(9301)
    n, dim = 2_000, 130
    model = M.RowModel(dim, f16=True)
    base = M.centred(rng, n, dim)
    model.write(base)
    idx = index_of(L, base, f16=True)
    big = 777

    def step(tag):
        q = (model.rows[rng.integers(0, len(model), 16)] + f32(0.02) * rng.standard_normal((16, dim)).astype(f32)).astype(f32)
        q[0] = model.rows[len(model) - 1]
        q[1] = model.rows[1]
        assert len(idx) == len(model) and np.array_equal(bits(idx.read_rows(0, len(model))), bits(model.rows)), tag
        fresh = index_of(L, model.rows, f16=True)
        for metric in ("l2", "ip", "cosine"):
            check(oracle, idx, fresh, model.rows, q, 10, metric, on_small, ("alias", tag), f16=True)
        return idx.hbm_bytes()

    aliased = step("written")
    new = model.rows[big:big + 1].copy()
    new[0, 5] = 40_000.0
    model.update([big], new)
    idx.update_rows([big], new)
    owned = step("1: owned after the update")
    assert owned >= aliased + n * 136 * 2                           # (an F16 shard's pitch: round_up(130, 8) halves per row)
    keep = rng.random(n) < 0.7
    keep[[0, 1]] = False, True
    keep[big] = True
    at = int(keep[:big].sum())
    model.compact(keep)
    assert idx.compact(keep, 128) == len(model)
    assert step("2: compacted while owned") >= aliased + len(model) * 136 * 2
    assert model.rows[at, 5] == 40_000.0
    small = M.centred(rng, 1, dim)
    model.update([at], small)
    idx.update_rows([at], small)
    assert step("3: aliased again after the update") <= aliased
    keep = rng.random(len(model)) < 0.7
    keep[[0, 1]] = False, True
    model.compact(keep)
    assert idx.compact(keep, 128) == len(model)
    assert step("4: compacted while aliased") <= aliased


# ---- 11. seeded operation sequences --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(M.SEQ_SHAPES))
@pytest.mark.parametrize("seed", M.SEQ_SEEDS)
def test_seeded_operation_sequence(L, oracle, seed, shape):
    """A dozen steps of write / update / compact / search (3, 16 or 40 queries of ip, l2, cosine or hamming) / filtered search / range search /
    build_pq or build_hnsw + search (f32 shards).  After every step the rows equal the model's, and every read equals a fresh handle holding the
    model rows and the oracle.  The operation list is printed when a step fails."""
    import test_gpu_range_search as R

    n0, dim, f16 = M.SEQ_SHAPES[shape]
    first, ops = M.draw_ops(seed, n0, dim, f16)
    model = M.RowModel(dim, f16)
    model.write(first)
    idx = index_of(L, first, f16=f16)
    done = []
    try:
        for step, op in enumerate(ops):
            done.append(op)
            tag = (seed, shape, step, op[0])
            if op[0] == "write":
                model.write(op[1])
                idx.write(op[1])
            elif op[0] == "update":
                model.update(op[1], op[2])
                idx.update_rows(op[1], op[2])
            elif op[0] == "compact":
                model.compact(op[1])
                assert idx.compact(op[1], 64 * (1 + step % 3)) == len(model), tag
            rows = model.rows
            n = len(model)
            assert len(idx) == n and np.array_equal(bits(idx.read_rows(0, n)), bits(rows)), tag
            if op[0] in ("write", "update", "compact"):
                continue
            fresh = index_of(L, rows, f16=f16)
            q = op[1]
            if op[0] == "search":
                got = idx.search_batch_arrays(q, 10, op[2])
                assert_same(got, fresh.search_batch_arrays(q, 10, op[2]), tag)
                assert_exact(got, [M.oracle_topk(oracle, q[i], rows, 10, op[2], f16) for i in range(q.shape[0])], tag)
            elif op[0] == "filtered":
                got = idx.search_filtered_batch_arrays(q, 10, op[2], op[3])
                assert_same(got, fresh.search_filtered_batch_arrays(q, 10, op[2], op[3]), tag)
                if not f16:
                    assert_exact(got, filtered_want(oracle, rows, q, 10, op[2], op[3]), tag)
            elif op[0] == "range":
                case = R.Case(q, R.all_dists(oracle, q, rows, O.L2), O.L2)
                thr = np.array([case.D[i][case.order[i]][min(op[2], n - 1)] for i in range(q.shape[0])], f32)
                got = idx.search_range_batch_arrays(q, thr, 100, "l2")
                R.check(got, case, thr, 100)
                exp = fresh.search_range_batch_arrays(q, thr, 100, "l2")
                assert all(np.array_equal(bits(a) if a.dtype == f32 else a, bits(b) if b.dtype == f32 else b) for a, b in zip(got, exp)), tag
            elif op[2] == "pq":
                for h in (idx, fresh):
                    h.build_pq(4, 16)
                assert_same(idx.search_pq_batch_arrays(q, 10, "l2"), fresh.search_pq_batch_arrays(q, 10, "l2"), tag)
                g, e = idx.pq_params(), fresh.pq_params()
                assert g["n"] == n and np.array_equal(g["codebooks"], e["codebooks"]) and np.array_equal(g["codes"], e["codes"]), tag
            else:
                for h in (idx, fresh):
                    h.build_hnsw("l2", 4, 16, 8)
                assert_same(idx.search_hnsw_batch_arrays(q, 10, "l2"), fresh.search_hnsw_batch_arrays(q, 10, "l2"), tag)
                g, e = idx.hnsw_params(), fresh.hnsw_params()
                assert g["n"] == n and np.array_equal(g["adj0"], e["adj0"]), tag
    except Exception:
        print(f"seed {seed} {shape}, failed at step {len(done) - 1}: {M.describe(done)}")
        raise
