"""The grow-on-demand device scratch of a handle across a grow / shrink / grow sequence of calls.

A handle keeps its search scratch between calls and regrows a buffer only when a call needs more than the buffer holds, so a call may
run on buffers that an earlier, larger call left behind.  Each case runs the same sequence of calls twice over the same data: on ONE
long-lived handle, and on a FRESH handle per step (whose scratch is sized by that step alone).  Rows, distances and counts of the two
must be bit-equal at every step; no tolerance is involved.

Sequence: 4,096 rows of 64 dimensions; 4, 300, 4 and 520 queries (300 and 520 cross the 256-query chunk); subsets of 100, 3,000, 100
and again 3,000 ids where the search takes one."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
f32 = np.float32
N, DIM, K, NLIST = 4096, 64, 10, 16
STEPS = [(4, 100), (300, 3000), (4, 100), (520, 3000)]   # (queries, subset ids)


@pytest.fixture(scope="module")
def L():
    import lynsedb_amd as L_

    assert L_._lib.device_count() >= 1
    return L_


@pytest.fixture(scope="module")
def corpus():
    rng = np.random.default_rng(20261)
    data = rng.standard_normal((N, DIM)).astype(f32)
    queries = rng.standard_normal((520, DIM)).astype(f32)
    subset = rng.permutation(N)[:3000].astype(np.uint64)   # unordered: the gathered-rows strategy sorts it
    cen = data[rng.permutation(N)[:NLIST]].copy()
    d2 = (data.astype(np.float64) ** 2).sum(1)[:, None] - 2.0 * data.astype(np.float64) @ cen.astype(np.float64).T + (cen.astype(np.float64) ** 2).sum(1)[None]
    asg = np.argmin(d2, axis=1).astype(np.uint32)
    for a in (data, queries, subset, cen, asg):
        a.setflags(write=False)
    return {"data": data, "queries": queries, "subset": subset, "cen": cen, "asg": asg}


def words_of(rows):
    w = np.zeros(N // 64, np.uint64)
    for r in rows:
        w[int(r) // 64] |= np.uint64(1) << np.uint64(int(r) % 64)
    return w


def flat_of(L, corpus):
    h = L.FlatIndex(None, DIM)
    h.write(corpus["data"])
    h.finalize()
    return h


def assert_same_at_every_step(make, call):
    """make() -> a handle; call(handle, nq, ns) -> arrays.  The long-lived handle against a fresh one per step."""
    long_lived = make()
    for step, (nq, ns) in enumerate(STEPS):
        kept = call(long_lived, nq, ns)
        fresh = call(make(), nq, ns)
        assert len(kept) == len(fresh)
        assert int(np.asarray(kept[2]).sum()) > 0   # (the counts: the comparison is of results, not of two empty answers)
        for i, (a, b) in enumerate(zip(kept, fresh)):
            a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
            assert a.dtype == b.dtype and a.shape == b.shape
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"step {step} (nq {nq}, subset {ns}): output {i} differs"


@pytest.mark.parametrize("strategy", ["1", "2"])   # the gathered rows, the masked scan
def test_flat_ip_list_subset(L, corpus, monkeypatch, strategy):
    monkeypatch.setenv("LYNSE_HIP_FILTER_STRATEGY", strategy)
    assert_same_at_every_step(lambda: flat_of(L, corpus),
                              lambda h, nq, ns: h.search_filtered_batch_arrays(corpus["queries"][:nq], K, "ip", corpus["subset"][:ns]))


def test_flat_l2_bitset(L, corpus):
    words = {ns: words_of(corpus["subset"][:ns]) for ns in (100, 3000)}
    assert_same_at_every_step(lambda: flat_of(L, corpus),
                              lambda h, nq, ns: h.search_filtered_bitset_batch_arrays(corpus["queries"][:nq], K, "l2", words[ns]))


def test_ivf_ip_filtered(L, corpus):
    assert_same_at_every_step(lambda: L.IvfFlatIndex.load(corpus["data"], corpus["cen"], corpus["asg"], "ip"),
                              lambda h, nq, ns: h.search_filtered_batch_arrays(corpus["queries"][:nq], K, 4, corpus["subset"][:ns]))


def test_ivf_l2_sq8(L, corpus):
    mn = corpus["data"].min(0).astype(f32)
    sc = ((corpus["data"].max(0) - mn) / f32(255)).astype(f32)
    assert_same_at_every_step(lambda: L.IvfFlatIndex.load_sq8(corpus["data"], corpus["cen"], corpus["asg"], mn, sc, "l2"),
                              lambda h, nq, ns: h.search_batch_arrays(corpus["queries"][:nq], K, 4))


def test_spann_ip(L, corpus):
    order = np.argsort(corpus["asg"], kind="stable")   # every row in its one list, ascending rows inside a list
    off = np.concatenate([[0], np.cumsum(np.bincount(corpus["asg"], minlength=NLIST))]).astype(np.uint64)
    assert_same_at_every_step(lambda: L.SpannIndex.load(corpus["data"], corpus["cen"], off, order.astype(np.uint64), 2, "ip"),
                              lambda h, nq, ns: h.search_batch_arrays(corpus["queries"][:nq], K, 4))


def test_flat_ip_pq(L, corpus):
    trained = flat_of(L, corpus)
    trained.build_pq(8, 16)
    p = trained.pq_params()   # one training: every handle of the case loads the same quantiser

    def make():
        h = flat_of(L, corpus)
        h.load_pq(p["codebooks"], p["codes"])
        return h

    assert_same_at_every_step(make, lambda h, nq, ns: h.search_pq_batch_arrays(corpus["queries"][:nq], K, "ip"))


def test_range_search(L, corpus):
    thr = np.full(520, 4.0, f32)   # an inner product of 4 against rows of norm ~8: a few per cent of the rows pass
    assert_same_at_every_step(lambda: flat_of(L, corpus),
                              lambda h, nq, ns: h.search_range_batch_arrays(corpus["queries"][:nq], thr[:nq], 16 if nq == 4 else 200, "ip"))
