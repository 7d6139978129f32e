"""BM25 text search on the GPU (include/lynse_hip.h, TEXT SEARCH) against the plain-C restatement of its rules
(tests/text_ref/text_ref.c): rows, counts, passer counts and f32 score bits equal, for every query of every batch."""
import numpy as np
import pytest

import text_common as tc
from text_common import Corpus, Queries, f32, u32, u64

pytestmark = pytest.mark.gpu

N, VOCAB = 20011, 2000
R = 4096                      # TEXT_ROWS of csrc/text.h: N spans five tiles, the middle one starts at row 8192
CAP = 256                     # TEXT_MAX_TERMS
BASE = 2 * R
# planted terms, appended to the vocabulary
T_EDGE, T_EVERY, T_LAST, T_RARE, T_FREQ, T_EVERY2 = VOCAB, VOCAB + 1, VOCAB + 2, VOCAB + 3, VOCAB + 4, VOCAB + 5
V_ALL = VOCAB + 6
EDGE_ROWS = [BASE - 1, BASE, BASE + R - 1, BASE + R]
COPIES = [50, 51, 4095, 4096, 15000]   # identical documents: equal scores, ordered by row


@pytest.fixture(scope="module")
def L():
    import lynsedb_amd as L_

    return L_


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return tc.build_ref(tmp_path_factory.mktemp("text_ref"))


@pytest.fixture(scope="module")
def world():
    """the main corpus with its planted terms, and where they were planted"""
    rng = np.random.default_rng(2024)
    docs = tc.gen_corpus(rng, N, VOCAB).docs()
    for r in COPIES[1:]:
        docs[r] = dict(docs[COPIES[0]])
    free = np.setdiff1d(np.arange(N), COPIES)   # (the copies stay identical: nothing is planted in one of them alone)
    rare = np.sort(rng.choice(free, 10, replace=False))
    freq = np.sort(rng.choice(free, 5000, replace=False))
    for r in EDGE_ROWS:
        docs[r][T_EDGE] = 2
    for r in range(N):
        docs[r][T_EVERY] = 1 if r in COPIES else 1 + r % 3
        docs[r][T_EVERY2] = 2
    docs[N - 1][T_LAST] = 3
    for r in rare:
        docs[int(r)][T_RARE] = 1
    for r in freq:
        docs[int(r)][T_FREQ] = 1
    return dict(corpus=Corpus.of(docs, V_ALL), rare=rare, freq=freq, rng=rng)


@pytest.fixture(scope="module")
def idx(L, world):
    c = world["corpus"]
    i = L.TextIndex(device=0)
    i.set(c.doc_len, *c.csc())
    assert (len(i), i.terms, i.nnz) == (c.n, V_ALL, c.doc_term.size) and i.hbm_bytes() >= 4 * (c.n + 2 * c.doc_term.size)
    return i


@pytest.fixture(scope="module")
def main_queries(world):
    return tc.gen_queries(np.random.default_rng(7), 300, VOCAB)


@pytest.fixture(scope="module")
def main_refs(ref, world, main_queries):
    return ref.batch(world["corpus"], main_queries, 10)


def words_of(live):
    return np.packbits(np.asarray(live, bool), bitorder="little").tobytes().ljust((len(live) + 63) // 64 * 8, b"\0")


def mask_words(live):
    return np.frombuffer(words_of(live), u64).copy()


def search(idx, q: Queries, k, words=None):
    return idx.search_batch_arrays(*q.arrays(), k, words)


def compare(idx, ref, corpus, q: Queries, k, live=None, what=None, refs=None):
    refs = ref.batch(corpus, q, k, live) if refs is None else refs
    tc.check_batch(search(idx, q, k, None if live is None else mask_words(live)), refs, k, what)
    return refs


# ---- the main corpus -----------------------------------------------------------------------------------------------------------------
def test_restatement_is_order_sensitive_on_the_main_corpus(ref, world, main_queries, main_refs):
    """What keeps the comparison below from passing on an order-blind kernel: among the (query, document) pairs that match three or
    more query terms — a sum of two terms commutes — at least a fifth change bits when summed in reverse slot order."""
    rev = ref.batch(world["corpus"], main_queries, 10, reversed_=True)
    pairs = changed = 0
    for a, b in zip(main_refs, rev):
        m = a["matched"] >= 3
        pairs += int(m.sum())
        changed += int((a["score"][m].view(u32) != b["score"][m].view(u32)).sum())
        assert np.allclose(a["score"], b["score"], rtol=1e-5)
    assert pairs >= 1000, pairs
    assert changed * 5 >= pairs, (changed, pairs)


@pytest.mark.parametrize("nq", [1, 16, 300])
def test_main_corpus_batches(idx, main_queries, main_refs, nq):
    q = Queries(main_queries.lists[:nq])
    tc.check_batch(search(idx, q, 10), main_refs[:nq], 10, f"batch of {nq}")
    assert N > 2 * R


def test_tile_edges(idx, ref, world):
    c = world["corpus"]
    q = Queries([([T_EDGE], [1]), ([T_EDGE, 3, 0], [1, 2, 1]), ([0, T_EDGE], [1, 1]), ([T_EVERY], [1]), ([5, T_EVERY, T_RARE], [1, 1, 1]),
                 ([T_LAST], [2]), ([T_LAST, 1], [1, 1]), ([T_EDGE, T_LAST, T_EVERY2], [1, 1, 1])])
    refs = compare(idx, ref, c, q, 50, what="tile edges")
    assert list(tc.order_of(refs[0])) == sorted(EDGE_ROWS, key=lambda r: (-float(refs[0]["score"][r]), r)) and refs[0]["passed"] == 4
    assert refs[3]["passed"] == N and list(refs[5]["result"].nonzero()[0]) == [N - 1]
    compare(idx, ref, c, q, N, what="tile edges, every row asked for")


# ---- the candidate rule --------------------------------------------------------------------------------------------------------------
def test_candidate_rule(idx, ref, world):
    c = world["corpus"]
    q = Queries([([T_RARE, T_FREQ], [1, 1])])
    only_freq = np.setdiff1d(world["freq"], world["rare"])
    at10 = ref.batch(c, q, 10)[0]
    assert list(at10["df"]) == [10, 5000] and list(at10["cand"]) == [1, 0]                 # cutoff max(40, 80)
    assert (at10["score"][only_freq] > 0).all() and not at10["result"][only_freq].any() and at10["passed"] == 10
    at1000 = ref.batch(c, q, 1000)[0]
    assert list(at1000["cand"]) == [1, 1] and at1000["result"][only_freq].all()            # cutoff max(40, 8000)
    assert at1000["passed"] == np.union1d(world["freq"], world["rare"]).size
    tc.check_batch(search(idx, q, 10), [at10], 10, "k = 10")
    tc.check_batch(search(idx, q, 1000), [at1000], 1000, "k = 1000")
    # terms of every row only: no term qualifies, every term is a candidate term
    q = Queries([([T_EVERY], [1]), ([T_EVERY2, T_EVERY], [1, 2])])
    refs = compare(idx, ref, c, q, 25, what="all-terms fallback")
    assert all(list(r["cand"]) == [1] * len(r["cand"]) and r["passed"] == N for r in refs)
    # a term of every row next to a selective one is never a candidate term: the rows of the selective term alone come back
    q = Queries([([T_EVERY, T_RARE], [1, 1]), ([T_RARE, T_EVERY2, T_EVERY], [1, 1, 1])])
    refs = compare(idx, ref, c, q, 25, what="every-row term next to a selective one")
    assert all(list(r["result"].nonzero()[0]) == list(world["rare"]) for r in refs) and list(refs[0]["cand"]) == [0, 1]


# ---- masks ---------------------------------------------------------------------------------------------------------------------------
def test_masks(idx, ref, world, main_queries, main_refs):
    c = world["corpus"]
    rng = np.random.default_rng(99)
    live = rng.random(N) < 0.6
    live[rng.choice(N, 300, replace=False)] = False           # "tombstones" on top of the subset
    q = Queries(main_queries.lists[:24] + [([T_RARE, T_FREQ], [1, 1]), ([T_EVERY, 4], [1, 1]), ([T_EDGE, T_LAST], [1, 1])])
    refs = compare(idx, ref, c, q, 10, live, "subset and tombstones")
    plain = main_refs[:24]
    assert all(r["docs"] == int(live.sum()) < N and r["total"] == int(c.doc_len[live].sum()) for r in refs)
    assert any(not np.array_equal(a["df"], b["df"]) for a, b in zip(refs, plain))
    assert any(not np.array_equal(a["w"].view(u32), b["w"].view(u32)) for a, b in zip(refs, plain))
    # a mask that turns a selective term into the term of every live row changes the candidate terms
    few = np.zeros(N, bool)
    few[world["rare"]] = True
    few[world["freq"][:40]] = True
    q2 = Queries([([T_RARE, T_FREQ], [1, 1]), ([T_FREQ, T_EVERY], [1, 1])])
    r2 = compare(idx, ref, c, q2, 10, few, "a small subset")
    assert r2[0]["docs"] == int(few.sum()) and list(r2[0]["cand"]) == [1, 1] and list(ref.batch(c, q2, 10)[0]["cand"]) == [1, 0]
    # a mask that empties a term: the term is ignored, the rest of the query answers
    gone = np.ones(N, bool)
    gone[world["rare"]] = False
    r3 = compare(idx, ref, c, Queries([([T_RARE, 7], [1, 1]), ([T_RARE], [1])]), 10, gone, "a term emptied")
    assert r3[0]["df"][0] == 0 and r3[0]["passed"] > 0 and r3[1]["passed"] == 0
    # a mask that empties the corpus, as zero words and as no words at all
    compare(idx, ref, c, q, 10, np.zeros(N, bool), "an empty corpus")
    got = search(idx, q, 10, np.zeros(0, u64))
    assert not got[2].any() and not got[3].any() and (got[0] == tc.NO_ROW).all()
    # words that cover only the first rows: the rest is out
    short = np.zeros(N, bool)
    short[:640] = True
    tc.check_batch(search(idx, q, 10, mask_words(short)[:10]), ref.batch(c, q, 10, short), 10, "short words")
    # ... and the unmasked search still answers as before
    tc.check_batch(search(idx, Queries(main_queries.lists[:24]), 10), plain, 10, "after the masks")


def test_masked_batch_whose_first_chunk_is_empty(idx, ref, world, main_queries):
    """A batch goes in chunks of at most 256 queries.  Under a mask the live corpus totals are counted by the first chunk that reaches
    the device — not by chunk 0, which launches nothing when its queries are all empty."""
    c = world["corpus"]
    rng = np.random.default_rng(123)
    live = rng.random(N) < 0.5
    empty = [([], [])] * 256
    for lead, tail in [(empty, main_queries.lists[:9] + [([T_EVERY, T_RARE], [1, 1])]),
                       (empty + empty, [([], [])] * 3 + main_queries.lists[9:14]),
                       (main_queries.lists[:2] + empty[2:], empty[:255] + main_queries.lists[2:5])]:
        q = Queries(lead + tail)
        refs = compare(idx, ref, c, q, 10, live, "leading empty chunk")
        assert all(r["docs"] == int(live.sum()) for r in refs) and sum(r["passed"] for r in refs[len(lead):]) > 0
        compare(idx, ref, c, q, 10, what="leading empty chunk, no mask")
    # a mask that leaves no row is found out by that later chunk too
    q = Queries(empty + main_queries.lists[:3])
    got = search(idx, q, 10, mask_words(np.zeros(N, bool)))
    assert not got[2].any() and not got[3].any() and (got[0] == tc.NO_ROW).all() and np.isneginf(got[1]).all()


# ---- the cut and the order -----------------------------------------------------------------------------------------------------------
def test_cut_and_order(idx, ref, world):
    c = world["corpus"]
    own = [t for t in sorted(c.docs()[COPIES[0]]) if t < VOCAB][-2:]   # the two rarest terms of the copied document
    q = Queries([(own, [1] * len(own)), ([T_EVERY], [1]), ([T_RARE], [1]), ([T_EDGE, T_RARE], [1, 1])])
    refs = compare(idx, ref, c, q, 3000, what="k above most passers")
    order = list(tc.order_of(refs[0]))
    at = [order.index(r) for r in COPIES]
    assert at == list(range(at[0], at[0] + len(COPIES))), at      # the identical documents tie and come back in row order
    assert refs[2]["passed"] == 10 < 3000
    refs = compare(idx, ref, c, q, 20000, what="k beyond the LDS sort")
    assert refs[1]["passed"] == N > 16384
    got = search(idx, q, 0)
    assert got[0].shape == (4, 0) and not got[2].any() and not got[3].any()
    compare(idx, ref, c, q, 1, what="k = 1")


# ---- limits and refusals -------------------------------------------------------------------------------------------------------------
def test_limits_and_refusals(L, idx, ref, world):
    c = world["corpus"]
    rng = np.random.default_rng(5)
    wide = rng.choice(VOCAB, CAP + 1, replace=False)
    ok = Queries([(wide[:CAP], np.ones(CAP)), ([3], [1])])
    compare(idx, ref, c, ok, 10, what="the cap")
    idx.profile_enable(True)
    idx.profile_get(reset=True)
    with pytest.raises(L._lib.LynseUnsupportedError, match="256"):
        search(idx, Queries([([3], [1]), (wide, np.ones(CAP + 1))]), 10)
    assert idx.profile_get()["scan_launches"] == 0
    compare(idx, ref, c, ok, 10, what="after the refusal")
    p = idx.profile_get()
    idx.profile_enable(False)
    assert p["scan_launches"] == 1 and p["scan_rows"] == 2 * N and p["scan_bytes"] > 0 and p["searches"] == 1
    for bad in [([3, 5, 3], [1, 1, 1]), ([V_ALL], [1]), ([3, 0xFFFFFFFF], [1, 1]), ([3], [0])]:
        with pytest.raises(ValueError):
            search(idx, Queries([([1], [1]), bad]), 10)
    compare(idx, ref, c, Queries([([3, 5], [1, 1])]), 10, what="after the invalid queries")
    # bad stores are refused before any device work; the store they were meant for stays empty and answers nothing
    small = Corpus.of([{0: 1, 1: 2}, {1: 1}, {0: 2, 2: 1}], 3)
    ptr, row, tf = small.csc()
    t = L.TextIndex(device=0)
    assert len(t) == 0 and not search(t, Queries([([], [])]), 5)[2].any()
    with pytest.raises(ValueError):
        search(t, Queries([([0], [1])]), 5)          # an empty store knows no term
    bads = [(small.doc_len, ptr + u64(1), row, tf), (small.doc_len, ptr[[0, 2, 1, 3]], row, tf),
            (small.doc_len, ptr, np.where(row == 2, 3, row), tf), (small.doc_len, ptr, row[[1, 0, 2, 3, 4]], tf),
            (small.doc_len + u32(1), ptr, row, tf), (small.doc_len, ptr, row, np.where(tf == 2, 0, tf)),
            (np.array([3, 1, 0], u32), ptr, row, tf)]
    for bad in bads:
        with pytest.raises(ValueError):
            t.set(*bad)
        assert len(t) == 0
    t.set(small.doc_len, ptr, row, tf)
    assert (len(t), t.terms, t.nnz) == (3, 3, 5)
    compare(t, ref, small, Queries([([1, 0], [1, 2]), ([2], [1]), ([], [])]), 5, what="a small store")
    t.set(np.zeros(0, u32), np.zeros(1, u64), np.zeros(0, u32), np.zeros(0, u32))
    assert len(t) == 0 and t.terms == 0


# ---- Collection ----------------------------------------------------------------------------------------------------------------------
WORDS = ["red", "green", "blue", "wine", "sky", "sea", "deep", "old", "new", "tower", "bridge", "river"]


def make_collection(L, rng, n=400, dim=8, pending=0):
    c = L.Collection("text", dim, device=0)
    docs = []
    for i in range(n):
        title = " ".join(rng.choice(WORDS, int(rng.integers(1, 6))))
        body = [" ".join(rng.choice(WORDS, int(rng.integers(0, 9)))), {"note": "Old TOWER" if i % 7 == 0 else None, "n": i}]
        docs.append({"title": title, "body": body, "year": 1990 + i % 30, "flag": i % 2 == 0})
    ids = [3 * i + 1 for i in range(n)]
    vec = rng.random((n, dim), dtype=np.float32)
    c.add_items(vec[:n - pending], ids[:n - pending], fields=docs[:n - pending])
    c.commit()
    if pending:
        c.add_items(vec[n - pending:], ids[n - pending:], fields=docs[n - pending:])
        assert c.pending_len() == pending
    return c, ids, docs, vec


def expected_text(L, ref, ids, docs, text, text_fields, k, dead=(), allowed=None):
    """the restatement over the documents as the Python mirror indexes them -> (ids, scores)"""
    from lynsedb_amd.core import index_text_document

    sel = set(text_fields or [])
    rows, vocab, kept = [], {}, []
    for i, d in sorted(zip(ids, docs)):
        tf = {}
        for name, counts in index_text_document(d).items():
            if not sel or name in sel:
                for t, n_ in counts.items():
                    tid = vocab.setdefault(t, len(vocab))
                    tf[tid] = tf.get(tid, 0) + n_
        if tf:
            rows.append(tf)
            kept.append(i)
    corpus = Corpus.of(rows, len(vocab))
    counts = {}
    for t in L.tokenize_text(text):
        if t in vocab:
            counts[vocab[t]] = counts.get(vocab[t], 0) + 1
    kept = np.array(kept, np.int64)
    live = ~np.isin(kept, list(dead)) if allowed is None else (np.isin(kept, list(allowed)) & ~np.isin(kept, list(dead)))
    r = ref.search(corpus, list(counts), list(counts.values()), k, live)
    order = tc.order_of(r)[:k]
    return kept[order], r["score"][order]


def same_result(res, exp, mode="BM25-INVERTED"):
    assert res.index_mode() == mode
    assert np.array_equal(res.ids(), exp[0]), (res.ids()[:10], exp[0][:10])
    assert np.array_equal(res.distances().view(u32), exp[1].view(u32)), (res.distances()[:10], exp[1][:10])


def test_collection_field_selections_pending_rows_and_deletes(L, ref):
    rng = np.random.default_rng(31)
    c, ids, docs, _ = make_collection(L, rng, pending=60)
    assert c.text_len() == 400
    for text, fields in [("red wine", None), ("Old tower, old BRIDGE", []), ("red wine", ["title"]), ("old tower", ["body"]),
                         ("deep blue sea river", ["title", "body"]), ("tower", ["body", "nothing"]), ("sky", ["year"]), ("zzz sky", ["title"])]:
        for k in (5, 1000):
            res = c.text_search(text, fields, k)
            same_result(res, expected_text(L, ref, ids, docs, text, fields, k))
            assert res._dim == 8 and res._k == k
    assert len(c.text_search("sky", ["year"])) == 0 and len(c.text_search("", None)) == 0 and len(c.text_search("red", None, 0)) == 0
    batch = c.batch_text_search(["red wine", "", "old old tower"], ["title"], 7)
    for res, text in zip(batch, ["red wine", "", "old old tower"]):
        same_result(res, expected_text(L, ref, ids, docs, text, ["title"], 7))
    # the last rows are still pending and are found
    pend = set(ids[-60:])
    assert pend & set(c.text_search("red wine old tower sea", None, 1000).ids().tolist())
    # deleting ids takes them out of the statistics too; restoring brings them back
    first = c.text_search("red wine", None, 10)
    dead = [int(x) for x in first.ids()[:3]] + ids[100:160]
    c.delete_items(dead)
    same_result(c.text_search("red wine", None, 10), expected_text(L, ref, ids, docs, "red wine", None, 10, dead=dead))
    c.restore_items(dead)
    same_result(c.text_search("red wine", None, 10), (first.ids(), first.distances()))
    # subset= takes dense rows
    rows = np.arange(0, 400, 3)
    allowed = [ids[r] for r in rows]
    same_result(c.text_search("blue sea", ["title"], 20, subset=rows), expected_text(L, ref, ids, docs, "blue sea", ["title"], 20, allowed=allowed))
    # documents added later are searched
    c.add_items(rng.random((1, 8), dtype=np.float32), [5000], fields=[{"title": "zzz unique sky"}])
    assert list(c.text_search("zzz", None, 3).ids()) == [5000]
    # a re-added id replaces its document, also by one that holds no text
    c.add_items(rng.random((1, 8), dtype=np.float32), [5000], fields=[{"title": "other words"}])
    assert len(c.text_search("zzz", None, 3)) == 0 and list(c.text_search("other", None, 3).ids()) == [5000] and c.text_len() == 401
    c.add_items(rng.random((1, 8), dtype=np.float32), [5000], fields=[{"title": "", "year": 7}])
    assert len(c.text_search("other", None, 3)) == 0 and c.text_len() == 400
    with pytest.raises(OverflowError):
        c.text_search("red", None, -1)
    with pytest.raises(NotImplementedError):
        c.text_search("red", where_expr="year > 2000")
    with pytest.raises(RuntimeError, match=r"Invalid argument: ids length \(1\) must match field count \(2\)"):
        c.add_items(rng.random((1, 8), dtype=np.float32), [6000], fields=[{}, {}])


def test_collection_without_text_reports_the_scan_mode(L):
    c = L.Collection("plain", 8, device=0)
    c.add_items(np.ones((3, 8), np.float32), [1, 2, 3], fields=[{"n": 1}, {"ok": True}, {"t": ""}])
    res = c.text_search("anything", None, 5)
    assert res.index_mode() == "BM25-SCAN" and len(res) == 0 and c.text_len() == 0


def test_reference_api_cases(L):
    """The reference's public-API cases on its fixture, restated as data: 20 rows of dimension 8 with tag = "item_<i>"."""
    rng = np.random.default_rng(42)
    vec = rng.random((20, 8), dtype=np.float32)
    c = L.Collection("api", 8, device=0)
    c.add_items(vec, list(range(20)), fields=[{"tag": f"item_{i}", "value": i} for i in range(20)])
    c.commit()
    res = c.text_search("item_3", text_fields=["tag"], k=3)
    assert 3 in res.ids().tolist() and res.index_mode() == "BM25-INVERTED"
    assert res.ids().tolist() == [3]            # "item" is in every row and never a candidate term next to "3"
    res = c.hybrid_search(vec[3], "item_3", text_fields=["tag"], k=5)
    assert len(res) == 5 and np.isfinite(res.distances()).all() and res.index_mode() == "HYBRID-RRF"
    assert res.ids()[0] == 3
    assert len(c.text_search("alpha", k=1, text_fields=["tag"])) == 0
    assert len(c.hybrid_search(vector=vec[0], text="alpha", k=2)) == 2


@pytest.mark.parametrize("mode", ["FLAT-IP", "FLAT-L2"])
def test_hybrid_search_is_the_cpu_fusion_of_its_legs(L, mode):
    from lynsedb_amd.core import hybrid_fuse

    rng = np.random.default_rng(77)
    c, ids, docs, vec = make_collection(L, rng, n=300)
    c.build_index(mode)
    asc = mode == "FLAT-L2"
    qv = vec[17] + f32(0.01)
    for fusion, kw in [("rrf", {}), ("RRF", dict(rrf_k=10.0, vector_weight=2.0)), ("weighted", {}), ("Weighted", dict(vector_weight=0.3, text_weight=1.7)),
                       ("weighted", dict(text_weight=-1.0)), ("rrf", dict(candidate_limit=7))]:
        k = 6
        limit = max(kw.get("candidate_limit") or 4 * k, k, 1)
        v = c.search(qv, limit)
        t = c.text_search("old tower river", ["title", "body"], limit)
        e_ids, e_s = hybrid_fuse((v.ids(), v.distances()), (t.ids(), t.distances()), k, fusion, kw.get("vector_weight", 1.0), kw.get("text_weight", 1.0),
                                 kw.get("rrf_k", 60.0), asc)
        res = c.hybrid_search(qv, "old tower river", k, text_fields=["title", "body"], fusion=fusion, **kw)
        assert res.index_mode() == ("HYBRID-WEIGHTED" if fusion.lower() == "weighted" else "HYBRID-RRF")
        assert np.array_equal(res.ids(), e_ids) and np.array_equal(res.distances().view(u32), e_s.view(u32)), (fusion, kw)
        assert len(res) == k and len(t) > 0
    # one leg alone: a blank text with a vector is the vector leg, no vector is the text leg
    v = c.search(qv, 24)
    res = c.hybrid_search(qv, "  ", 6)
    assert np.array_equal(res.ids(), hybrid_fuse((v.ids(), v.distances()), None, 6, ascending=asc)[0])
    t = c.text_search("old tower", None, 24)
    res = c.hybrid_search(None, "old tower", 6)
    assert np.array_equal(res.ids(), hybrid_fuse(None, (t.ids(), t.distances()), 6)[0])
    sub = np.arange(0, 300, 2)
    res = c.hybrid_search(qv, "old tower", 6, subset=sub)
    assert set(res.ids().tolist()) <= {ids[r] for r in sub}
    with pytest.raises(RuntimeError, match="hybrid_search requires a vector, text, or both"):
        c.hybrid_search(None, " ")
