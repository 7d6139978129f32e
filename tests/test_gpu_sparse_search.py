"""GPU parity tests for sparse-vector search (include/lynse_hip.h, SPARSE VECTORS) through the C ABI, SparseIndex and the Collection,
against the restatement of the reference's arithmetic (tests/sparse_ref/sparse_ref.c, checked on its own in tests/test_sparse_modes.py).
Expected per query: the rows with score != 0, by (score descending with NaN as -inf, row ascending), the first k.  Rows, counts, passer
counts and f32 score bits are compared exactly; there are no tolerances."""
import numpy as np
import pytest

import sparse_common as sc
from sparse_common import Csr, f32, u32, u64

pytestmark = pytest.mark.gpu
G = 16          # lanes of a row group in k_sparse_scan (SPARSE_G)
ROW_TILE = 128  # rows of a tile (SPARSE_ROWS)
MAX_NNZ = 4096  # entries of one query (SPARSE_MAX_NNZ)


@pytest.fixture(scope="module")
def L():
    import lynsedb_amd as L_

    assert L_._lib.device_count() >= 1
    return L_


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return sc.build_ref(tmp_path_factory.mktemp("sparse_ref"))


def index_of(L, rows: Csr):
    idx = L.SparseIndex(device=0)
    idx.set_rows(*rows.arrays())
    assert len(idx) == len(rows) and idx.nnz == rows.indices.size
    return idx


def search(idx, queries: Csr, k, words=None):
    return idx.search_batch_arrays(*queries.arrays(), k, words)


def live_of(words, n, n_words=None):
    w = np.asarray(words, u64)[:n_words]
    bits = np.unpackbits(w.view(np.uint8), bitorder="little").astype(bool)
    live = np.zeros(n, bool)
    m = min(n, bits.size)
    live[:m] = bits[:m]
    return live


# ---- 1. parity on the three configurations ---------------------------------------------------------------------------------------------
N_PARITY, NQ_MAX = 20011, 300
_cfg_cache = {}


@pytest.fixture(scope="module")
def cfg(L, ref):
    def get(name):
        if name not in _cfg_cache:
            vocab, lo, hi, qnnz = sc.CONFIGS[name]
            rng = np.random.default_rng(ord(name))
            rows = sc.gen_vectors(rng, N_PARITY, vocab, lo, hi)
            queries = sc.gen_vectors(rng, NQ_MAX, vocab, qnnz, qnnz)
            smat = ref.scores(queries, rows)
            rev = ref.scores(queries, rows, reversed_=True) if name in "AB" else None
            orders = [sc.order_of(smat[i]) for i in range(NQ_MAX)]
            _cfg_cache[name] = (rows, queries, smat, rev, orders, index_of(L, rows))
        return _cfg_cache[name]

    yield get
    _cfg_cache.clear()


@pytest.mark.parametrize("nq", [1, 7, 33, 300])
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_parity_through_the_c_abi(cfg, name, nq):
    rows, queries, smat, rev, orders, idx = cfg(name)
    if rev is not None:   # the data can tell a wrong summation order: a fifth of these pairs change bits when summed in reverse
        frac = float(np.mean(smat[:nq].view(u32) != rev[:nq].view(u32)))
        assert frac >= 0.2, (name, nq, frac)
    if name == "C":       # most pairs share no index
        assert float(np.mean(smat == 0)) > 0.5 and not np.isnan(smat).any()
    for k in (1, 10, 100):
        sc.check_batch(search(idx, queries.head(nq), k), smat[:nq], k, what=(name, nq, k), orders=orders)


# ---- 2. row lengths --------------------------------------------------------------------------------------------------------------------
def test_row_length_edges(L, ref):
    rng = np.random.default_rng(2)
    vocab = 40000
    lens = [0, 1, 2, G - 1, G, G + 1, 2 * G - 1, 2 * G, 2 * G + 1, 63, 64, 65, 127, 128, 129, 1000, 0, 3, 20000, 5, 0]
    lens += [int(x) for x in rng.integers(0, 12, 3 * ROW_TILE + 37 - len(lens))]   # n = 421: the last tile is partial
    assert len(lens) % ROW_TILE != 0
    vecs = []
    for m in lens:
        ind = np.sort(rng.choice(vocab, m, replace=False)).astype(u32)
        vecs.append((ind, sc.gen_values(rng, m)))
    rows = Csr.of(vecs)
    # queries dense enough to meet the short rows: a tenth of the vocabulary each, so every step width of the long rows has hits and misses
    queries = Csr.of([(np.sort(rng.choice(vocab, 4000, replace=False)).astype(u32), sc.gen_values(rng, 4000)) for _ in range(5)])
    smat = ref.scores(queries, rows)
    assert np.all(smat[:, [0, 16, 20]] == 0) and (smat[:, 18] != 0).all() and (smat[:, :16] != 0).any()
    idx = index_of(L, rows)
    for k in (1, 7, len(lens), len(lens) + 5):
        sc.check_batch(search(idx, queries, k), smat, k, what=("row lengths", k))
    # (those tiles shrink to one query each); narrower queries share a tile
    narrow = Csr.of([(np.sort(rng.choice(vocab, 300, replace=False)).astype(u32), sc.gen_values(rng, 300)) for _ in range(7)])
    sc.check_batch(search(idx, narrow, 9), ref.scores(narrow, rows), 9, what="row lengths, one tile")


# ---- 3. index extremes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["full_u32", "mod_2_15", "mod_2_16", "mod_2_20"])
def test_index_extremes_and_collisions(L, ref, kind):
    rng = np.random.default_rng(3)
    if kind == "full_u32":
        vocab = np.unique(np.concatenate([[0, 0xFFFFFFFF, 1, 0xFFFFFFFE, 0x80000000, 0x7FFFFFFF], rng.integers(0, 1 << 32, 3000, dtype=np.uint64)])).astype(u32)
    else:
        step = {"mod_2_15": 1 << 15, "mod_2_16": 1 << 16, "mod_2_20": 1 << 20}[kind]
        # every index of a residue class collides in the prefilter (and, for the larger steps, in the table's home slots); two classes
        vocab = np.unique(np.concatenate([5 + step * np.arange(min(2000, (1 << 32) // step), dtype=np.uint64),
                                          77 + step * np.arange(min(500, (1 << 32) // step), dtype=np.uint64)])).astype(u32)

    def vec(m):
        ind = np.sort(rng.choice(vocab, m, replace=False))
        return ind, sc.gen_values(rng, m)

    assert kind != "full_u32" or (vocab[0] == 0 and vocab[-1] == 0xFFFFFFFF)
    rows = Csr.of([vec(int(m)) for m in rng.integers(1, 120, 700)] + [(vocab[[0, -1]], [1.5, -2.5])])
    queries = Csr.of([vec(60) for _ in range(18)] + [(vocab[[0, -1]], [2.0, 3.0]), (vocab[[0]], [1.0]), (vocab[[-1]], [1.0])])
    smat = ref.scores(queries, rows)
    assert smat[-3, -1] == f32(1.5 * 2.0 - 2.5 * 3.0) and smat[-2, -1] == 1.5 and smat[-1, -1] == -2.5
    assert float(np.mean(smat != 0)) > 0.05
    sc.check_batch(search(index_of(L, rows), queries, 50), smat, 50, what=kind)


# ---- 4. query shapes -------------------------------------------------------------------------------------------------------------------
def test_query_shapes(L, ref):
    rng = np.random.default_rng(4)
    vocab = 9000
    rows = sc.gen_vectors(rng, 1500, vocab, 1, 300)
    idx = index_of(L, rows)

    def q(m):
        return np.sort(rng.choice(vocab, m, replace=False)).astype(u32), sc.gen_values(rng, m)

    shared = np.sort(rng.choice(vocab, 50, replace=False)).astype(u32)
    disjoint = rng.permutation(vocab)[:16 * 40].reshape(16, 40)
    batches = {
        "nnz 1 and 4096": [q(1), q(MAX_NNZ), q(1)],
        "4096 alone": [q(MAX_NNZ)],
        "4096 twice and small": [q(MAX_NNZ), q(3), q(MAX_NNZ), q(2000)],
        "an empty query inside": [q(30), ([], []), q(30), ([], [])],
        "one tile sharing every index": [(shared, sc.gen_values(rng, 50)) for _ in range(16)],
        "one tile sharing none": [(np.sort(disjoint[i]).astype(u32), sc.gen_values(rng, 40)) for i in range(16)],
        "both tiles in one batch": [(shared, sc.gen_values(rng, 50)) for _ in range(16)] + [(np.sort(disjoint[i]).astype(u32), sc.gen_values(rng, 40)) for i in range(16)],
    }
    for what, vecs in batches.items():
        queries = Csr.of(vecs)
        smat = ref.scores(queries, rows)
        got = search(idx, queries, 20)
        sc.check_batch(got, smat, 20, what=what)
        if what == "an empty query inside":
            assert list(got[2][[1, 3]]) == [0, 0] and list(got[3][[1, 3]]) == [0, 0]
    # over the documented cap: refused before any launch
    idx.profile_enable(True)
    idx.profile_get(reset=True)
    with pytest.raises(L._lib.LynseUnsupportedError, match="4096"):
        search(idx, Csr.of([q(5), q(MAX_NNZ + 1)]), 5)
    assert idx.profile_get()["scan_launches"] == 0
    search(idx, Csr.of([q(5)]), 5)
    p = idx.profile_get()
    assert p["scan_launches"] == 1 and p["scan_rows"] == len(rows) and p["scan_bytes"] == rows.indices.size * 8 + (len(rows) + 1) * 8 and p["scan_us"] > 0
    idx.profile_enable(False)
    # queries are validated like rows
    for bad in [([5, 3], [1.0, 1.0]), ([3, 3], [1.0, 1.0]), ([3, 5], [1.0, 0.0]), ([3], [np.nan]), ([3], [np.inf])]:
        with pytest.raises(ValueError):
            search(idx, Csr.of([([1], [1.0]), bad]), 5)
    for bad in [([5, 3], [1.0, 1.0]), ([3, 5], [1.0, 0.0]), ([3], [-np.inf])]:
        with pytest.raises(ValueError):
            L.SparseIndex(device=0).set_rows(*Csr.of([bad]).arrays())
    with pytest.raises(ValueError):
        L.SparseIndex(device=0).set_rows(np.array([1, 2], u64), np.array([1, 2], u32), np.array([1, 2], f32))   # indptr[0] != 0
    with pytest.raises(ValueError):
        L.SparseIndex(device=0).set_rows(np.array([0, 2, 1], u64), np.array([1, 2], u32), np.array([1, 2], f32))   # decreasing


# ---- 5. the != 0 rule ------------------------------------------------------------------------------------------------------------------
def test_zero_scores_nan_and_infinities(L, ref):
    a, b, c = 10, 20, 30
    big = f32(3e38)
    rows = Csr.of([
        {a: 2.5, b: -2.5},        # 0: cancels exactly against {a: 1, b: 1}
        {a: 1.0},                 # 1: 1.0
        {c: 7.0},                 # 2: no common index
        {a: big, b: big},         # 3: with q2 = {a: big, b: -big}: +inf - inf = NaN -> kept, -inf, last
        {a: big},                 # 4: with q2: +inf, first
        {a: -0.75, b: 0.75},      # 5: cancels
        {b: 4.0},                 # 6
        {},                       # 7: empty
        {a: -big},                # 8: with q2: -inf, an ordinary value: ties with the NaN row, by row
    ])
    queries = Csr.of([{a: 1.0, b: 1.0}, {a: big, b: -big}, {c + 1: 1.0}])
    smat = ref.scores(queries, rows)
    assert list(smat[0][[0, 5, 2, 7]]) == [0, 0, 0, 0] and np.isnan(smat[1, 3]) and smat[1, 4] == np.inf and smat[1, 8] == -np.inf
    idx = index_of(L, rows)
    for k in (1, 3, 5, 9, 20):
        got = search(idx, queries, k)
        sc.check_batch(got, smat, k, what=("rule", k))
    r, s, cnt, passed = search(idx, queries, 20)
    assert list(r[0, :cnt[0]]) == [3, 4, 6, 1, 8] and list(passed) == [5, 7, 0]   # k above the passer count: exactly the passers
    # +inf first (rows 0 and 4 tie, by row), the NaN of row 3 reported as -inf among the -inf rows, by row
    assert list(r[1, :cnt[1]]) == [0, 4, 1, 3, 5, 6, 8] and list(s[1, :2]) == [np.inf, np.inf] and np.all(np.isneginf(s[1, 3:7]))
    assert cnt[2] == 0   # a query nothing matches
    r, s, cnt, passed = search(idx, Csr.of([{c + 1: 1.0}, {c + 2: 2.0}]), 4)   # a whole chunk in which nothing passes
    assert list(cnt) == [0, 0] and list(passed) == [0, 0] and np.all(r == u64(0xFFFFFFFFFFFFFFFF))
    # k == 0 and an all-empty batch touch nothing
    r, s, cnt, passed = search(idx, queries, 0)
    assert r.shape == (3, 0) and list(cnt) == [0, 0, 0]
    r, s, cnt, passed = search(idx, Csr.of([{}, {}]), 3)
    assert list(cnt) == [0, 0] and list(passed) == [0, 0]


# ---- 6. ties ---------------------------------------------------------------------------------------------------------------------------
def test_ties_are_cut_by_ascending_row(L, ref):
    rng = np.random.default_rng(6)
    n, vocab = 3000, 12
    vecs = []
    for _ in range(n):
        m = int(rng.integers(1, 5))
        vecs.append((np.sort(rng.choice(vocab, m, replace=False)).astype(u32), rng.integers(1, 3, m).astype(f32)))
    rows = Csr.of(vecs)
    queries = Csr.of([(np.arange(vocab, dtype=u32), np.ones(vocab, f32)), ([0, 3, 7], [1.0, 2.0, 1.0]), ([1], [1.0])])
    smat = ref.scores(queries, rows)
    vals, counts = np.unique(smat[0], return_counts=True)
    assert vals.size <= 10 and counts.max() > 300
    idx = index_of(L, rows)
    order = sc.order_of(smat[0])
    inside = [k for k in (10, 100, 257, 1000) if smat[0][order[k - 1]] == smat[0][order[k]]]   # the cut falls inside a tie group
    assert len(inside) >= 2
    for k in (10, 100, 257, 1000):
        sc.check_batch(search(idx, queries, k), smat, k, what=("ties", k))


# ---- 7. masks --------------------------------------------------------------------------------------------------------------------------
def test_masks(L, ref):
    rng = np.random.default_rng(7)
    n = 1000 + 37   # a partial last word
    rows = sc.gen_vectors(rng, n, 200, 1, 80)
    queries = sc.gen_vectors(rng, 5, 200, 30, 30)
    smat = ref.scores(queries, rows)
    idx = index_of(L, rows)
    nw = (n + 63) // 64
    random_words = rng.integers(0, 1 << 63, nw, dtype=np.uint64) | (rng.integers(0, 2, nw, dtype=np.uint64) << u64(63))
    beyond = random_words.copy()
    beyond[-1] |= ~u64(0) << u64(n % 64)   # bits at or beyond n are ignored
    longer = np.concatenate([random_words, np.full(3, ~u64(0), u64)])
    few = np.zeros(nw, u64)
    few[3] = u64(0b1011) << u64(17)   # three live rows: fewer than k
    few[-1] = u64(1) << u64((n - 1) % 64)   # ... and the last row
    cases = [("random", random_words), ("bits beyond n", beyond), ("more words than rows", longer), ("all zero", np.zeros(nw, u64)),
             ("short of the rows", random_words[:nw - 5]), ("one word", random_words[:1]), ("no words", np.zeros(0, u64)),
             ("fewer live rows than k", few), ("all ones", np.full(nw, ~u64(0), u64))]
    for what, words in cases:
        live = live_of(words, n)
        for k in (1, 10, 64):
            sc.check_batch(search(idx, queries, k, words), smat, k, live=live, what=(what, k))
    assert live_of(few, n).sum() == 4


# ---- 8. beyond the LDS sort ------------------------------------------------------------------------------------------------------------
def test_large_k_takes_the_host_sort(L, ref):
    rng = np.random.default_rng(8)
    n = 30000
    rows = sc.gen_vectors(rng, n, 200, 1, 80)
    queries = sc.gen_vectors(rng, 3, 200, 30, 30)
    smat = ref.scores(queries, rows)
    idx = index_of(L, rows)
    assert min(int((smat[i] != 0).sum()) for i in range(3)) > 20000   # more passers than k: the radix selection, then the host sort
    sc.check_batch(search(idx, queries, 20000), smat, 20000, what="k = 20000")
    sc.check_batch(search(idx, queries, n + 10000), smat, n + 10000, what="k > n")
    sc.check_batch(search(idx, queries, 16385), smat, 16385, what="k = 16385")
    sc.check_batch(search(idx, queries, 16384), smat, 16384, what="k = 16384")


# ---- 9. the store is replaced whole ----------------------------------------------------------------------------------------------------
def test_set_rows_replaces_the_store(L, ref):
    rng = np.random.default_rng(9)
    queries = sc.gen_vectors(rng, 4, 300, 25, 25)
    idx = L.SparseIndex(device=0)
    assert len(idx) == 0 and idx.nnz == 0
    got = search(idx, queries, 5)   # a store never filled
    assert list(got[2]) == [0] * 4
    for n, hi in [(700, 60), (90, 200), (1300, 30)]:
        rows = sc.gen_vectors(rng, n, 300, 0, hi)
        idx.set_rows(*rows.arrays())
        assert len(idx) == n and idx.nnz == rows.indices.size and idx.hbm_bytes() >= rows.indices.size * 8 + (n + 1) * 8
        sc.check_batch(search(idx, queries, 12), ref.scores(queries, rows), 12, what=("set_rows", n))
    idx.set_rows(np.zeros(1, u64), np.zeros(0, u32), np.zeros(0, f32))
    assert len(idx) == 0 and idx.nnz == 0
    r, s, cnt, passed = search(idx, queries, 5)
    assert list(cnt) == [0] * 4 and list(passed) == [0] * 4 and np.all(r == u64(0xFFFFFFFFFFFFFFFF)) and np.all(np.isneginf(s))


# ---- 10. Collection ----------------------------------------------------------------------------------------------------------------------
def coll_of(L, ids, path=None, dim=4):
    c = L.Collection("c", dim, device=0, path=path)
    c.add_items(np.arange(len(ids) * dim, dtype=f32).reshape(len(ids), dim), ids)
    c.commit()
    return c


def pairs(res):
    return [int(x) for x in res.ids()], [float(x) for x in res.distances()]


def test_collection_known_answer_and_id_order(L):
    c = coll_of(L, [10, 20, 30])
    c.add_sparse_vectors([{1: 1.0, 5: 0.5}, {2: 2.0, 5: 1.0}, {2: 0.5, 7: 1.0}], [10, 20, 30])
    res = c.search_sparse({2: 1.0}, k=2)
    assert pairs(res) == ([20, 30], [2.0, 0.5]) and res.index_mode() == "SPARSE-FLAT-IP" and res._dim == 0 and res._k == 2
    assert pairs(c.search_sparse([(5, 1.0)])) == ([20, 10], [1.0, 0.5]) and c.search_sparse({5: 1.0})._k == 10   # k=None means 10
    assert pairs(c.search_sparse({2: 1.0}, k=0)) == ([], []) and pairs(c.search_sparse({}, k=3)) == ([], [])
    assert pairs(c.search_sparse([(3, 0.0), (2, 0.5), (2, 0.5)], k=1)) == ([20], [2.0])
    with pytest.raises(NotImplementedError):
        c.search_sparse({2: 1.0}, where_expr="a > 1")
    # equal scores come back in id order, not insertion order
    c2 = coll_of(L, [30, 10, 20])
    c2.add_sparse_vectors([{4: 1.0}, {4: 1.0}, {4: 1.0, 9: 3.0}], [30, 10, 20])
    assert pairs(c2.search_sparse({4: 2.0})) == ([10, 20, 30], [2.0, 2.0, 2.0])
    assert pairs(c2.search_sparse({4: 2.0}, k=2)) == ([10, 20], [2.0, 2.0])
    # replace an id, remove one with a vector that normalises to empty
    c2.add_sparse_vectors([{4: 5.0}], [20])
    assert pairs(c2.search_sparse({4: 2.0})) == ([20, 10, 30], [10.0, 2.0, 2.0]) and pairs(c2.search_sparse({9: 1.0})) == ([], [])
    c2.add_sparse_vectors([[(4, 1.0), (4, -1.0)], {}], [10, 30])
    assert pairs(c2.search_sparse({4: 2.0})) == ([20], [10.0]) and c2.sparse_len() == 1


def test_collection_errors_leave_the_store_unchanged(L):
    c = coll_of(L, [1, 2, 3])
    c.add_sparse_vectors([{1: 1.0}, {1: 2.0}], [1, 2])
    before = pairs(c.search_sparse({1: 1.0}))
    assert before == ([2, 1], [2.0, 1.0])
    for vectors, ids, msg in [
        ([{1: 9.0}], [1, 2], r"Invalid argument: ids length \(2\) must match sparse vector count \(1\)"),
        ([{1: 9.0}, {1: 9.0}], [3, 3], "Invalid argument: duplicate id 3 within sparse vector batch"),
        ([{1: 9.0}, {1: 9.0}], [3, 99], "Invalid argument: cannot add sparse vector for unknown id 99"),
        ([{1: 9.0}, {1: 9.0}], [99, 99], "Invalid argument: cannot add sparse vector for unknown id 99"),   # unknown comes before its duplicate
        ([{1: 9.0}, {1: float("nan")}], [3, 1], "Invalid argument: sparse vector values must be finite"),
        ([{1: 9.0}, {1: float("inf")}], [3, 1], "Invalid argument: sparse vector values must be finite"),
    ]:
        with pytest.raises(RuntimeError, match=msg):
            c.add_sparse_vectors(vectors, ids)
        assert pairs(c.search_sparse({1: 1.0})) == before and c.sparse_len() == 2
    with pytest.raises(RuntimeError, match="sparse vector values must be finite"):
        c.search_sparse({1: float("nan")})
    # an id that is only pending is accepted
    c.add_items(np.ones((1, 4), f32), [50])
    assert c.pending_len() == 1
    c.add_sparse_vectors([{1: 4.0}], [50])
    assert pairs(c.search_sparse({1: 1.0})) == ([50, 2, 1], [4.0, 2.0, 1.0])


def test_collection_tombstones_subsets_and_batches(L, ref):
    rng = np.random.default_rng(10)
    n = 300
    ids = [int(x) for x in rng.permutation(n) * 3 + 7]   # dense row r holds user id ids[r]
    c = coll_of(L, ids)
    vecs = sc.gen_vectors(rng, n, 60, 1, 20)
    c.add_sparse_vectors([dict(zip(*[x.tolist() for x in vecs.row(r)])) for r in range(n)], ids)
    queries = sc.gen_vectors(rng, 6, 60, 10, 10)
    qd = [dict(zip(*[x.tolist() for x in queries.row(i)])) for i in range(6)]
    by_id = np.argsort(ids)   # sparse row s holds the vector of dense row by_id[s]
    sorted_ids = np.array(ids)[by_id]
    smat = ref.scores(queries, Csr.of([vecs.row(int(r)) for r in by_id]))

    def want(qi, k, live=None):
        o = sc.order_of(smat[qi], live)[:k]
        return [int(x) for x in sorted_ids[o]], [float(x) for x in sc.reported(smat[qi], o)]

    batch = c.batch_search_sparse(qd, k=15)
    for qi in range(6):
        assert pairs(batch[qi]) == want(qi, 15) == pairs(c.search_sparse(qd[qi], k=15))
    assert len(c.batch_search_sparse(qd)[0]) == 10
    # tombstones leave before the cut; restore brings them back
    dead = [x for x in want(0, 15)[0][:4]]
    c.delete_items(dead)
    live = ~np.isin(sorted_ids, dead)
    assert pairs(c.search_sparse(qd[0], k=15)) == want(0, 15, live) and not set(dead) & set(pairs(c.search_sparse(qd[0], k=15))[0])
    c.restore_items(dead[:2])
    assert pairs(c.search_sparse(qd[0], k=15)) == want(0, 15, ~np.isin(sorted_ids, dead[2:]))
    c.restore_items(dead)
    # subset= in dense rows: a BitSet and an array of row indices
    sub_rows = np.sort(rng.choice(n, 40, replace=False))
    live = np.isin(sorted_ids, np.array(ids)[sub_rows])
    for subset in (L.BitSet.from_rows(sub_rows, n), sub_rows, list(sub_rows) + [n + 5]):
        assert pairs(c.search_sparse(qd[1], k=50, subset=subset)) == want(1, 50, live)
        assert [pairs(r) for r in c.batch_search_sparse(qd, k=50, subset=subset)] == [want(i, 50, live) for i in range(6)]
    assert pairs(c.search_sparse(qd[1], k=5, subset=np.zeros(0, np.uint64))) == ([], [])


def test_collection_persists_and_reloads(L, tmp_path):
    c = coll_of(L, [10, 20, 30], path=tmp_path)
    c.add_sparse_vectors([{1: 1.0, 5: 0.5}, {2: 2.0, 5: 1.0}, {2: 0.5, 7: 1e-30}], [10, 20, 30])
    c.add_sparse_vectors([{}], [10])
    text = (tmp_path / "sparse_vectors.jsonl").read_text()
    assert text == '{"id":20,"indices":[2,5],"values":[2.0,1.0]}\n{"id":30,"indices":[2,7],"values":[0.5,1e-30]}\n'
    d = coll_of(L, [10, 20, 30], path=tmp_path)
    assert pairs(d.search_sparse({2: 1.0})) == ([], []) and d.try_load_sparse() and d.sparse_len() == 2
    for q in ({2: 1.0}, {5: 1.0}, {7: 1.0}):
        assert pairs(d.search_sparse(q)) == pairs(c.search_sparse(q))
    assert pairs(d.search_sparse({2: 1.0})) == ([20, 30], [2.0, 0.5])
    assert not coll_of(L, [1]).try_load_sparse() and not coll_of(L, [1], path=tmp_path / "none").try_load_sparse()
