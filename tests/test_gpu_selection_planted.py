"""GPU tests of the code every score-matrix search ends in — the radix selection k_pq_hist / k_pq_find / k_pq_emit driven by
ScoreCut::cut, the LDS sort k_pool_select<256|1024> and the order-and-pad code of range_cut_and_order — on one-column shards, where
the score image of every row is an input of the test: at dim = 1 IP with the query [1.0] returns 0 + 1 * v and L1 with the query [0.0]
returns 0 + |0 - v| (tests/selection_common.py has the datasets; tests/test_selection_planted_design.py shows, without a GPU, which
selection digit each of them reaches).  Expected distances come from the oracle (all_distances, IPFORM_SINGLE) and the additive
restatement (tests/additive_ref/additive_ref.c), once per distinct query value, and are asserted bit-equal to the planted values.
Rows, counts, `passed`, f32 distance bits and the padding are compared exactly; there are no tolerances.

Left out on purpose: the 256 MiB pool bound of ScoreCut::chunk.  It needs a cap above 131,072, which costs about 400 MB of host
output and a few hundred host sorts per call — too slow for this suite."""
import numpy as np
import pytest

import oracle as O
import selection_common as S
from additive_common import L1, build_ref
from selection_common import Column, check_range, check_topk

pytestmark = pytest.mark.gpu
f32, u32, u64 = np.float32, np.uint32, np.uint64


@pytest.fixture(scope="module")
def L():
    import lynsedb_amd as L_

    assert L_._lib.device_count() >= 1
    return L_


class Bank:
    """the datasets, their one-column shards and the reference's columns, each made once for the module"""

    def __init__(self, L, oracle, ref):
        self.L, self.oracle, self.ref = L, oracle, ref
        self.ds, self.idx, self.cols = {}, {}, {}

    def dataset(self, name, asc):
        if (name, asc) not in self.ds:
            self.ds[name, asc] = S.DATASETS[name](asc)
        return self.ds[name, asc]

    def index_of(self, values):
        idx = self.L.FlatIndex(None, 1, device=0)
        idx.write(np.ascontiguousarray(values, f32).reshape(-1, 1))
        return idx

    def index(self, name, asc, negated=False):
        if (name, asc, negated) not in self.idx:
            v = self.dataset(name, asc).values
            self.idx[name, asc, negated] = self.index_of(-v if negated else v)
        return self.idx[name, asc, negated]

    def ip_column(self, stored, scale):
        """the oracle's IP scores of the query [scale]; the premise: they are scale * stored, bit for bit (NaN rows apart)"""
        d = self.oracle.all_distances(np.array([scale], f32), np.ascontiguousarray(stored, f32).reshape(-1, 1), O.IP, O.IPFORM_SINGLE)
        planted = f32(scale) * stored
        assert np.array_equal(np.isnan(d), np.isnan(planted))
        ok = ~np.isnan(planted)
        assert np.array_equal(d[ok].view(u32), (planted[ok] + f32(0.0)).view(u32))
        return Column(d, False)

    def l1_column(self, stored, nan_as_inf=False):
        """the restatement's L1 distances of the query [0]; the premise: they are |stored|"""
        d = self.ref.raw_dists(L1, np.zeros((1, 1), f32), np.ascontiguousarray(stored, f32).reshape(-1, 1))[0]
        assert np.array_equal(np.isnan(d), np.isnan(stored))
        ok = ~np.isnan(stored)
        assert np.array_equal(d[ok].view(u32), np.abs(stored[ok]).view(u32))
        if nan_as_inf:
            d[np.isnan(d)] = np.inf
        return Column(d, True)

    def column(self, name, metric, scale=1.0, negated=False):
        """metric "ip": the query [scale] (negated: on the negated column); "l1": the query [0]; "l1_topk": the same, a NaN reported as +inf"""
        if (name, metric, scale, negated) not in self.cols:
            v = self.dataset(name, metric != "ip").values
            if metric == "ip":
                col = self.ip_column(-v if negated else v, scale)
            else:
                col = self.l1_column(v, metric == "l1_topk")
            self.cols[name, metric, scale, negated] = col
        return self.cols[name, metric, scale, negated]


@pytest.fixture(scope="module")
def bank(L, oracle, tmp_path_factory):
    return Bank(L, oracle, build_ref(tmp_path_factory.mktemp("additive_ref")))


def queries_of(scales):
    return np.array(scales, f32).reshape(-1, 1)


# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["ip", "l1"])
@pytest.mark.parametrize("name", list(S.DATASETS))
def test_cut_in_every_digit(bank, name, metric):
    asc = metric == "l1"
    ds, idx = bank.dataset(name, asc), bank.index(name, asc)
    if asc:     # three copies of the query [0]; the middle one admits every row
        queries, cols, scale = np.zeros((3, 1), f32), [bank.column(name, "l1")] * 3, (1.0, 1.0, 1.0)
    else:       # [1], [2], [0.5]: the same order at three exponents
        queries, cols, scale = queries_of(S.IP_SCALES), [bank.column(name, "ip", s) for s in S.IP_SCALES], S.IP_SCALES
    for cut in ds.cuts:
        thr = np.array([cut.thr * f32(s) for s in scale], f32)
        if asc:
            thr[1] = np.inf
        got = idx.search_range_batch_arrays(queries, thr, cut.cap, metric)
        print(f"\n{name}[{metric}] {cut}: passed {got[3].tolist()}, counts {got[2].tolist()}, last row kept {got[0][:, cut.cap - 1].tolist()}")
        check_range(got, cols, thr, cut.cap, what=(name, metric, cut))
        assert (got[3] > cut.cap).all() and (got[2] == cut.cap).all()      # every query had to select, as the design test says
        for q in range(3):   # the cut fell inside a planted group: its last row is one of the group's, and the group is not exhausted
            group = next(g for g in ds.groups.values() if int(got[0][q, cut.cap - 1]) in set(g.tolist()))
            assert 0 < np.isin(group, got[0][q].astype(np.int64)).sum() < group.size
    if not asc:   # once more with the query [-1] on the negated column: the same scores from negative stored values
        nidx, col = bank.index(name, asc, negated=True), bank.column(name, "ip", -1.0, negated=True)
        assert np.array_equal(col.order, bank.column(name, "ip", 1.0).order)
        for cut in ds.cuts:
            thr = np.array([cut.thr, -np.inf, cut.thr], f32)
            got = nidx.search_range_batch_arrays(queries_of([-1.0] * 3), thr, cut.cap, "ip")
            check_range(got, [col] * 3, thr, cut.cap, what=(name, "negated", cut))
            assert (got[3] > cut.cap).all()


@pytest.mark.parametrize("metric", ["ip", "l1"])
@pytest.mark.parametrize("name", ["digit3", "rows_512"])
def test_mixed_states_in_one_chunk(bank, name, metric):
    asc = metric == "l1"
    ds, idx = bank.dataset(name, asc), bank.index(name, asc)
    n, N = ds.n, {"digit3": ds.cuts[1].cap, "rows_512": ds.cuts[2].cap}[name]      # a cap inside the cluster / the run
    assert 3 * N < n
    nq = 40
    # IP: [1], [2], [0.5] and [-1], which reverses the order: its N-th key lies among distinct scores and is found in an earlier pass
    scales = [0.0 if asc else (S.IP_SCALES + (-1.0,))[(q + q // 8) % 4] for q in range(nq)]
    cols = [bank.column(name, "l1") if asc else bank.column(name, "ip", s) for s in scales]

    def thresholds(counts):
        """the threshold under which `count` rows of each query pass (None: a NaN threshold; a tie group goes in whole)"""
        thr = np.empty(nq, f32)
        for q, c in enumerate(counts):
            col = cols[q]
            thr[q] = np.nan if c is None else (np.nextafter(col.threshold_for(1), col.fail_thr) if c == 0 else col.threshold_for(c))
        return thr

    # one chunk in which queries start done, select (and finish in different passes), pass nothing and carry a NaN threshold, interleaved
    kinds = [0, 1, N - 1, N, N + 1, 3 * N, n, None]
    thr = thresholds([kinds[q % 8] for q in range(nq)])
    passed = [cols[q].passed(thr[q]) for q in range(nq)]
    got = idx.search_range_batch_arrays(queries_of(scales), thr, N, metric)
    print(f"\nmixed {name}[{metric}]: cap {N}, passed of queries 0..7 {got[3][:8].tolist()} (expected {passed[:8]}), largest count {int(got[2].max())}")
    check_range(got, cols, thr, N, what=(name, metric, "mixed"))
    assert {0, n} <= set(passed) and any(0 < p <= N for p in passed) and any(N < p < n for p in passed)   # done, selecting, empty
    assert np.isnan(thr[7::8]).all() and (got[3][7::8] == 0).all()
    if name != "digit3":      # (the equal values of rows_512 pass as a whole: the counts below need distinct scores)
        return
    assert passed == [0 if k is None else k for k in (kinds[q % 8] for q in range(nq))]
    # every count below the cap and all of them different: the device's output stride is the largest count, not the cap
    counts = np.random.default_rng(8).permutation(np.unique(np.linspace(0, N - 100, nq).astype(int))).tolist()
    assert len(counts) == nq
    thr = thresholds(counts)
    got = idx.search_range_batch_arrays(queries_of(scales), thr, N, metric)
    print(f"stride {name}[{metric}]: cap {N}, largest count {int(got[2].max())}, distinct counts {len(set(got[2].tolist()))} of {nq}")
    check_range(got, cols, thr, N, what=(name, metric, "stride"))
    assert len(set(got[2].tolist())) > nq // 2 and int(got[2].max()) < N and (got[2] == got[3]).all()


@pytest.mark.parametrize("metric", ["ip", "l1"])
def test_sort_sizes(bank, metric):
    asc = metric == "l1"
    v, cum = S.sort_sizes(asc)
    idx = bank.index_of(v)
    if asc:
        scales, cols = [0.0, 0.0], [bank.l1_column(v)] * 2
    else:
        scales, cols = [1.0, 2.0], [bank.ip_column(v, 1.0), bank.ip_column(v, 2.0)]
    n = v.size

    def run(cap, counts):
        thr = np.array([cols[q].threshold_for(c) for q, c in enumerate(counts)], f32)
        assert [cols[q].passed(thr[q]) for q in range(2)] == list(counts)       # the tie groups end where the counts say
        got = idx.search_range_batch_arrays(queries_of(scales), thr, cap, metric)
        print(f"\nsort[{metric}] cap {cap}: wanted {list(counts)}, passed {got[3].tolist()}, counts {got[2].tolist()}")
        check_range(got, cols, thr, cap, what=(metric, cap, counts))
        assert got[3].tolist() == list(counts)

    assert set(S.SORT_COUNTS) == {1, 2, 3, 1024, 1025, 2048, 2049, 16383, 16384}
    # the device sort: p2 = 2, 2 | 4, 1024 | 2048 (k_pool_select<256> -> <1024>), 2048 | 4096, 16384 (128 KiB of LDS)
    for counts in [(1, 1), (1, 2), (3, 1024), (1025, 1024), (1025, 2048), (2049, 16383), (16384, 1), (n, 16383), (16388, 16384)]:
        run(16384, counts)
    # the host sort: N = 16385 (the cut inside a tie group of 4) and 20000, counts on both sides of the cap
    for cap, pairs in [(16385, [(16384, n), (20000, 16388)]), (20000, [(16384, n), (20004, 19996)])]:
        for counts in pairs:
            run(cap, counts)
    tied = np.nonzero(cols[0].d == cols[0].d[cols[0].order[16384]])[0]
    assert tied.size == 4 and np.array_equal(cols[0].order[16384:16388], tied)   # the group the cap 16385 cuts, lowest row kept


@pytest.mark.parametrize("metric", ["ip", "l1"])
def test_score_matrix_bound_chunks(bank, metric):
    asc = metric == "l1"
    ds, idx = bank.dataset("rows_2p20", asc), bank.index("rows_2p20", asc)
    n, nq, cap = ds.n, 130, 64
    assert min(256, (512 << 20) // (n * 4), (256 << 20) // (cap * 8)) == 127 == (1 << 27) // n     # ScoreCut::chunk: 127 + 3 queries
    scales = [0.0 if asc else S.IP_SCALES[q % 3] for q in range(nq)]
    cols = [bank.column("rows_2p20", "l1") if asc else bank.column("rows_2p20", "ip", s) for s in scales]
    thr = np.array([cols[q].threshold_for(600) for q in range(nq)], f32)                            # the group of 600, cut at 64
    # distinct answers on both sides of the chunk boundary: nothing, the group, the group and 4,400 more rows, every row, a NaN threshold
    thr[125] = np.nextafter(cols[125].threshold_for(1), cols[125].fail_thr)
    thr[127] = cols[127].threshold_for(5000)
    thr[128] = ds.all_thr
    thr[129] = np.nan
    thr[3] = thr[128]
    got = idx.search_range_batch_arrays(queries_of(scales), thr, cap, metric)
    print(f"\nchunks[{metric}]: n {n}, queries per chunk {(1 << 27) // n}, passed[124:] {got[3][124:].tolist()}, counts[124:] {got[2][124:].tolist()}, "
          f"first rows of query 126 {got[0][126, :3].tolist()}")
    check_range(got, cols, thr, cap, what=("rows_2p20", metric, "chunks"))
    assert got[3][124:].tolist() == [600, 0, 600, 5000, n, 0] and got[2][124:].tolist() == [64, 0, 64, 64, 64, 0]


@pytest.mark.parametrize("name", ["digit3", "rows_512", "all_equal"])
def test_additive_topk_shares_the_cut(bank, L, name):
    ds, idx, col = bank.dataset(name, True), bank.index(name, True), bank.column(name, "l1_topk")
    n = ds.n
    ks = ([7, 513] if name == "all_equal" else [c.cap for c in ds.cuts]) + [n - 1, n, n + 5]      # k inside the tie clusters, k = n, k > n
    for nq in (3, 1):
        for k in ks:
            check_topk(idx.search_batch_arrays(np.zeros((nq, 1), f32), k, "l1"), col, nq, k, what=(name, nq, k))
    # half of every planted group masked out: those rows carry RANGE_FAIL and the cut falls among the rows that stay
    live = np.ones(n, bool)
    for g in ds.groups.values():
        live[g[1::2]] = False
    words = L.BitSet.from_rows(np.nonzero(live)[0], n).words
    n_live = int(live.sum())
    kept = {gn: int(live[g].sum()) for gn, g in ds.groups.items()}
    first = next(iter(kept.values()))
    ks = [900 + first // 2] if name == "digit3" else [7, first // 2, sum(kept.values()) - first // 2]
    ks += [n_live - 1, n_live, n_live + 3, n + 5]
    for nq in (3, 1):
        for k in ks:
            got = idx.search_filtered_bitset_batch_arrays(np.zeros((nq, 1), f32), k, "l1", words)
            print(f"\ntop-k {name} masked, {nq} queries, k {k} of {n_live} live: counts {got[2].tolist()}, last row {int(got[0][0, int(got[2][0]) - 1])}")
            check_topk(got, col, nq, k, live, what=(name, "masked", nq, k))
            assert live[got[0][0, :int(got[2][0])].astype(np.int64)].all()


@pytest.mark.parametrize("metric", ["ip", "l1"])
def test_non_finite_images(bank, metric):
    asc = metric == "l1"
    v = S.non_finite()
    n = v.size
    idx = bank.index_of(v)
    col = bank.l1_column(v) if asc else bank.ip_column(v, 1.0)
    q = queries_of([0.0 if asc else 1.0] * 2)
    d = col.d
    assert np.isnan(d).sum() == 3 and np.isinf(d).sum() == 4 and ((d != 0) & (np.abs(d) < S.FLT_MIN)).sum() == 5    # NaN, ±inf, denormals
    every = n - 3                                        # a NaN row never passes
    bound = S.FLT_MAX if asc else -S.FLT_MAX             # the finite side of the infinities that sort last
    finite = col.passed(bound)
    assert finite == (every - 4 if asc else every - 2)   # L1: |±inf| sort last; IP: the two -inf rows do
    ds_all = np.inf if asc else -np.inf
    for thr_v, p in ((ds_all, every), (bound, finite)):
        for cap in sorted({p - 1, p, p + 1, finite - 1, finite, finite + 1}):
            thr = np.array([thr_v, thr_v], f32)
            got = idx.search_range_batch_arrays(q, thr, cap, metric)
            print(f"\nnon-finite[{metric}] threshold {float(thr_v)} cap {cap}: passed {got[3].tolist()} (expected {p}), counts {got[2].tolist()}, "
                  f"last distance kept {got[1][0, min(cap, p) - 1]}")
            check_range(got, [col] * 2, thr, cap, what=(metric, float(thr_v), cap))
            assert (got[3] == p).all() and not np.isnan(got[1]).any()
            assert not np.isin(got[0], np.array([0, 500, n - 1], u64)).any()     # no NaN row, at the cut or elsewhere
    # thresholds at the denormals and at zero pass exactly what the reference says; a NaN threshold passes nothing
    for t in (0.0, 1e-45, -1e-45, 5e-39, float(S.FLT_MIN), np.nan):
        thr = np.array([t, ds_all], f32)
        check_range(idx.search_range_batch_arrays(q, thr, 50, metric), [col] * 2, thr, 50, what=(metric, t))
