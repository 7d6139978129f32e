"""Text search without a GPU: the tokenizer and the document indexing of the Python mirror, the restatement the GPU tests compare
against (tests/text_ref/text_ref.c) checked on its own, the host-only weights step of the C ABI, the fusion of hybrid_search and the
entry points' argument checks.  No GPU."""
import ctypes as C
import math
import re
from pathlib import Path

import numpy as np
import pytest

import text_common as tc
from text_common import Corpus, f32, u32, u64

HERE = Path(__file__).resolve().parent
INVALID, DEVICE = 1, 6
_vp = C.c_void_p
TEXT_ENTRY_POINTS = ["lynse_hip_text_create", "lynse_hip_text_destroy", "lynse_hip_text_set", "lynse_hip_text_len", "lynse_hip_text_hbm_bytes",
                     "lynse_hip_text_search", "lynse_hip_text_weights", "lynse_hip_text_profile_enable", "lynse_hip_text_profile_get"]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return tc.build_ref(tmp_path_factory.mktemp("text_ref"))


@pytest.fixture(scope="module")
def L():
    import lynsedb_amd as L_

    return L_


# ---- the tokenizer and the documents -------------------------------------------------------------------------------------------------
def test_tokenizer(L):
    tok = L.tokenize_text
    assert tok("hello world") == ["hello", "world"]
    assert tok("Hello, WORLD!  MiXed") == ["hello", "world", "mixed"]
    assert tok("item_3") == ["item", "3"]
    assert tok("abc123 4x4 v2.0") == ["abc123", "4x4", "v2", "0"]
    assert tok("") == [] and tok("  ,;--__  ") == []
    assert tok("a--b__c") == ["a", "b", "c"]                      # empty pieces dropped
    assert tok("Ärger über Öl") == ["ärger", "über", "öl"]        # non-ASCII letters split nothing and are lower-cased
    assert tok("naïve CAFÉ") == ["naïve", "café"]
    assert tok("ПРИВЕТ мир") == ["привет", "мир"]
    assert tok("東京 tower") == ["東京", "tower"]
    assert tok("x\ty\nz") == ["x", "y", "z"]


def test_document_indexing(L):
    from lynsedb_amd.core import index_text_document, text_term_counts

    assert text_term_counts("a b a") == {"a": 2, "b": 1}
    assert text_term_counts(["x y", ["y", {"k": "Z z"}], 3, 1.5, True, None]) == {"x": 1, "y": 2, "z": 2}
    assert text_term_counts({"p": "one", "q": {"r": ["two", "one"]}}) == {"one": 2, "two": 1}
    for nothing in (None, True, False, 7, 2.5, [], {}, [1, [2, None]], "", " ,. "):
        assert text_term_counts(nothing) == {}
    doc = index_text_document({"title": "Red red wine", "tags": ["wine", "drink"], "year": 1983, "ok": True, "blank": " - ", "none": None,
                               "nested": {"a": {"b": "deep Wine"}}})
    assert doc == {"title": {"red": 2, "wine": 1}, "tags": {"wine": 1, "drink": 1}, "nested": {"deep": 1, "wine": 1}}
    assert index_text_document({"year": 3, "flag": False, "empty": ""}) == {}      # no field left: not indexed


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
FIVE = [{0: 1, 1: 1}, {0: 2}, {1: 1, 2: 3}, {2: 1}, {0: 1, 1: 1, 2: 1}]   # lengths 2, 2, 4, 1, 3: total 12, avg 2.4


def test_restatement_on_five_documents_worked_by_hand(ref):
    """Query: term 0 once, term 2 twice.  df = 3 for both, idf = ln(2.5 / 3.5 + 1) = 0.5389965; every term is a candidate (3 < 5 and
    3 <= max(12, 80)).  Row 0: 0.5389965 * 2.2 / (1 + 1.2 * (0.25 + 0.75 * 2 / 2.4)) = 1.1857923 / 2.05 = 0.5784353, and so on."""
    c = Corpus.of(FIVE, 4)
    r = ref.search(c, [0, 2], [1, 2], 10)
    assert (r["docs"], r["total"], list(r["df"])) == (5, 12, [3, 3]) and list(r["cand"]) == [1, 1]
    assert np.allclose(r["w"], [0.5389965, 1.077993], rtol=1e-6)
    expect = [0.5784352690789815, 0.7775687223684669, 1.4822403770148898, 1.4158714049097456, 1.4669595483858704]
    assert np.allclose(r["score"], expect, rtol=1e-6) and r["result"].all() and r["passed"] == 5
    assert list(tc.order_of(r)) == [2, 4, 3, 1, 0]
    assert list(r["matched"]) == [1, 1, 1, 1, 2]
    # a mask changes the statistics: without rows 2 and 3 term 2 lives in row 4 alone
    r = ref.search(c, [0, 2], [1, 2], 10, live=[1, 1, 0, 0, 1])
    assert (r["docs"], r["total"], list(r["df"])) == (3, 7, [3, 1])
    assert list(r["cand"]) == [0, 1]                     # df 3 == docs: never a candidate next to a selective term
    assert list(r["result"]) == [False, False, False, False, True] and r["score"][0] > 0
    # a term nobody holds is ignored, a query of such terms has no result, k == 0 neither
    r = ref.search(c, [3, 0], [1, 1], 10)
    assert list(r["df"]) == [0, 3] and r["w"][0] == 0 and r["passed"] == 3
    assert ref.search(c, [3], [1], 10)["passed"] == 0 and ref.search(c, [0], [1], 0)["passed"] == 0
    # the term in every row alone: no term qualifies, so every term is a candidate term
    every = Corpus.of([{0: 1}, {0: 2, 1: 1}, {0: 1}], 2)
    r = ref.search(every, [0], [1], 10)
    assert list(r["cand"]) == [1] and r["passed"] == 3


def test_restatement_against_float64(ref):
    rng = np.random.default_rng(11)
    c = tc.gen_corpus(rng, 300, 60)
    q = tc.gen_queries(rng, 8, 60)
    docs = c.docs()
    total = int(c.doc_len.sum())
    avg = max(total / c.n, 1.0)
    checked = 0
    for (terms, counts), r in zip(q.lists, ref.batch(c, q, 10)):
        for d in range(c.n):
            s = 0.0
            for t, cnt in zip(terms, counts):
                tf = docs[d].get(int(t), 0)
                if tf:
                    df = sum(1 for x in docs if int(t) in x)
                    idf = math.log((c.n - df + 0.5) / (df + 0.5) + 1.0)
                    s += cnt * idf * (tf * 2.2) / (tf + 1.2 * (0.25 + 0.75 * float(c.doc_len[d]) / avg))
            assert abs(float(r["score"][d]) - s) <= 1e-5 * max(abs(s), 1e-30), (d, r["score"][d], s)
            checked += s > 0
    assert checked > 500


# ---- lynse_hip_text_weights ----------------------------------------------------------------------------------------------------------
def same_weights(L, ref, docs, total, df, count, k):
    from lynsedb_amd.core import text_weights

    a, w, c = text_weights(docs, total, df, count, k)
    ea, ew, ec = ref.weights(docs, total, df, count, k)
    assert np.array_equal(np.asarray([a]).view(u32), np.asarray([ea]).view(u32)), (a, ea)
    assert np.array_equal(w.view(u32), ew.view(u32)) and np.array_equal(c, ec), (df, w, ew, c, ec)
    return a, w, c


def test_weights_match_the_restatement_bit_for_bit(L, ref):
    rng = np.random.default_rng(3)
    for _ in range(200):
        docs = int(rng.integers(1, 5_000_000))
        total = int(rng.integers(0, 200)) * docs + int(rng.integers(0, docs + 1))
        T = int(rng.integers(1, 40))
        df = np.minimum(rng.integers(0, docs + 1, T) // rng.choice([1, 1, 10, 1000], T), docs).astype(u64)
        count = rng.integers(1, 5, T).astype(u32)
        same_weights(L, ref, docs, total, df, count, int(rng.choice([1, 10, 1000, 100000])))
    same_weights(L, ref, 7, 3, [], [], 10)                                    # no term
    a, w, c = same_weights(L, ref, 0, 0, [0, 0], [1, 2], 10)                  # no live row
    assert a == 1 and not w.any() and not c.any()
    a, _, _ = same_weights(L, ref, 10, 4, [1], [1], 10)                       # avg is never below 1
    assert a == 1


def test_weights_candidate_rule(L, ref):
    # df 10 next to df 5,000 of 20,000: the cutoff is max(40, 8k)
    _, _, c = same_weights(L, ref, 20000, 800000, [10, 5000], [1, 1], 10)
    assert list(c) == [1, 0]
    _, _, c = same_weights(L, ref, 20000, 800000, [10, 5000], [1, 1], 1000)
    assert list(c) == [1, 1]
    # frequent terms only: min_df * 4 admits the rarer one; both beyond every cutoff cannot happen (min_df <= 4 * min_df), so the
    # all-terms fallback is reached through df == docs alone
    _, _, c = same_weights(L, ref, 20000, 800000, [6000, 5000], [1, 1], 10)
    assert list(c) == [1, 1]
    _, _, c = same_weights(L, ref, 20000, 800000, [6000, 1000], [1, 1], 10)
    assert list(c) == [0, 1]
    _, w, c = same_weights(L, ref, 500, 9000, [500, 500], [2, 1], 10)         # df == docs everywhere: every term is a candidate term
    assert list(c) == [1, 1] and (w > 0).all()
    _, _, c = same_weights(L, ref, 500, 9000, [500, 0, 20], [1, 1, 1], 10)    # df == docs is no candidate next to a selective term, df 0 never
    assert list(c) == [0, 0, 1]
    _, w, c = same_weights(L, ref, 500, 9000, [500, 0], [1, 1], 10)           # ... and the fallback leaves df 0 out
    assert list(c) == [1, 0] and w[1] == 0
    # saturation: min_df * 4 beyond 2^64 stays the largest value instead of wrapping to a small one
    # (wrapped, the cutoff would be max(20, 80): no term would qualify and the fallback would flag the df == docs term too)
    big = (1 << 62) + 5
    _, _, c = same_weights(L, ref, 1 << 63, 1 << 63, [big, big + 1, 1 << 63], [1, 1, 1], 10)
    assert list(c) == [1, 1, 0]
    _, _, c = same_weights(L, ref, 1 << 40, 1 << 41, [100, 1 << 35], [1, 1], 0xFFFFFFFF)   # k * 8 does not wrap in 64 bits
    assert list(c) == [1, 0]
    _, _, c = same_weights(L, ref, 1 << 40, 1 << 41, [100, (1 << 35) - 8], [1, 1], 0xFFFFFFFF)
    assert list(c) == [1, 1]


# ---- the fusion ----------------------------------------------------------------------------------------------------------------------
def test_fusion_rrf_worked_by_hand(L):
    from lynsedb_amd.core import hybrid_fuse

    one = f32(1)
    r = lambda rank: f32(one / f32(f32(f32(60) + f32(rank)) + one))   # noqa: E731
    ids, s = hybrid_fuse(([1, 2, 3], [0.9, 0.5, 0.1]), ([3, 1], [4.0, 2.0]), 10)
    assert list(ids) == [1, 3, 2]
    assert np.array_equal(s, np.array([f32(r(0) + r(1)), f32(r(2) + r(0)), r(1)], f32))
    assert abs(float(s[0]) - (1 / 61 + 1 / 62)) < 1e-8
    ids, s = hybrid_fuse(([5, 2], [1.0, 0.5]), ([2, 5], [3.0, 1.0]), 10)           # equal sums: the lower id first
    assert list(ids) == [2, 5] and s[0] == s[1]
    ids, s = hybrid_fuse(([1, 2, 3], [0.9, 0.5, 0.1]), ([3, 1], [4.0, 2.0]), 2)    # cut at k
    assert list(ids) == [1, 3]
    ids, s = hybrid_fuse(([1, 2], [1.0, 0.5]), ([2, 9], [3.0, 1.0]), 10, text_weight=-3.0)   # a negative weight adds nothing
    assert list(ids) == [1, 2, 9] and np.array_equal(s, np.array([r(0), r(1), 0], f32))
    ids, s = hybrid_fuse(([1, 2], [1.0, 0.5]), None, 10, rrf_k=0.25)               # rrf_k is at least 1
    assert np.array_equal(s, np.array([f32(one / f32(f32(one + f32(0)) + one)), f32(one / f32(f32(one + one) + one))], f32))
    ids, s = hybrid_fuse(None, ([4, 6], [2.0, 1.0]), 10, vector_weight=5.0, text_weight=0.5)
    assert list(ids) == [4, 6] and np.array_equal(s, np.array([f32(f32(0.5) / f32(61)), f32(f32(0.5) / f32(62))], f32))


def test_fusion_weighted_worked_by_hand(L):
    from lynsedb_amd.core import hybrid_fuse, normalize_scores

    # vector leg (ip): [1, 0.5, 0] stays; text leg [4, 2] -> [1, 0]; id 1: 0.5 * 1 + 2 * 0, id 2: 0.5 * 0.5, id 3: 0.5 * 0 + 2 * 1
    ids, s = hybrid_fuse(([1, 2, 3], [1.0, 0.5, 0.0]), ([3, 1], [4.0, 2.0]), 10, "WeighTed", 0.5, 2.0)
    assert list(ids) == [3, 1, 2] and list(s) == [2.0, 0.5, 0.25]
    # the same distances under an ascending metric: 1 - x
    ids, s = hybrid_fuse(([1, 2, 3], [0.0, 0.5, 1.0]), ([3, 1], [4.0, 2.0]), 10, "weighted", 0.5, 2.0, ascending=True)
    assert list(ids) == [3, 1, 2] and list(s) == [2.0, 0.5, 0.25]
    ids, s = hybrid_fuse(([1, 2, 3], [1.0, 0.5, 0.0]), None, 10, "weighted", ascending=True)
    assert list(ids) == [3, 2, 1] and list(s) == [1.0, 0.5, 0.0]
    # a leg of equal scores normalises to 1.0, ascending or not; so does a span within FLT_EPSILON and a leg with no finite score
    for asc in (False, True):
        assert list(normalize_scores([3.0, 3.0, 3.0], asc)) == [1.0, 1.0, 1.0]
        assert list(normalize_scores([1.0, 1.0 + 2.0 ** -23], asc)) == [1.0, 1.0]
        assert list(normalize_scores([np.inf, -np.inf], asc)) == [1.0, 1.0]
    assert list(normalize_scores([2.0, np.inf, 1.0, -np.inf], False)) == [1.0, 1.0, 0.0, 0.0]   # clamped
    assert normalize_scores([], False).size == 0
    ids, s = hybrid_fuse(([7, 8], [3.0, 3.0]), ([8], [1.5]), 10, "weighted")
    assert list(ids) == [8, 7] and list(s) == [2.0, 1.0]
    ids, s = hybrid_fuse(([7, 8], [3.0, 1.0]), ([8, 7], [1.5, 0.5]), 10, "weighted", 1.0, -1.0)   # clamped to 0
    assert list(ids) == [7, 8] and list(s) == [1.0, 0.0]
    # anything but "weighted" is reciprocal rank
    assert np.array_equal(hybrid_fuse(([1], [1.0]), None, 5, "whatever")[1], hybrid_fuse(([1], [1.0]), None, 5, "RRF")[1])


def test_hybrid_search_needs_a_vector_or_a_text(L):
    c = L.Collection.__new__(L.Collection)   # (the check comes before anything of the collection is touched: no device needed)
    for text in (None, "", "  \t\n"):
        with pytest.raises(RuntimeError, match="^Invalid argument: hybrid_search requires a vector, text, or both$"):
            c.hybrid_search(None, text)
    with pytest.raises(OverflowError):
        c.hybrid_search(None, "x", k=-1)
    with pytest.raises(NotImplementedError):
        c.hybrid_search(None, "x", where_expr="a > 1")
    with pytest.raises(NotImplementedError):
        c.text_search("x", where_expr="a > 1")


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_text_entry_points_declared_exported_and_bound(L):
    header = (HERE.parent / "include" / "lynse_hip.h").read_text()
    assert "TEXT SEARCH" in header and "SLOT ORDER" in header
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = C.CDLL(str(L._lib.LIB_PATH))
    for name in TEXT_ENTRY_POINTS:
        assert re.search(rf"\b{name}\s*\(", code), name
        assert hasattr(raw, name), name
        assert name in L._lib.SIGNATURES, name
    assert L._lib.lib.lynse_hip_abi_version() == 1
    assert L.TextIndex and L.tokenize_text


def test_null_arguments_are_invalid(L):
    lib = L._lib.lib
    z = np.zeros(4, u64)
    p = L._lib.Profile()
    assert lib.lynse_hip_text_set(None, tc._p(z), 0, tc._p(z), 0, tc._p(z), tc._p(z)) == INVALID
    assert lib.lynse_hip_text_len(None, None, None, None) == INVALID and L._lib.last_error() == "handle is NULL"
    assert lib.lynse_hip_text_search(None, tc._p(z), tc._p(z), tc._p(z), 1, 1, None, 0, tc._p(z), tc._p(z), tc._p(z), None) == INVALID
    assert lib.lynse_hip_text_profile_enable(None, 1) == INVALID
    assert lib.lynse_hip_text_profile_get(None, C.byref(p), 0) == INVALID
    assert lib.lynse_hip_text_create(0, None) == INVALID
    assert lib.lynse_hip_text_hbm_bytes(None) == 0
    assert lib.lynse_hip_text_destroy(None) == 0
    assert lib.lynse_hip_text_weights(5, 5, tc._p(z), tc._p(z), 2, 10, None, tc._p(z), tc._p(z)) == INVALID
    assert lib.lynse_hip_text_weights(5, 5, None, tc._p(z), 2, 10, C.byref(C.c_float()), tc._p(z), tc._p(z)) == INVALID


def test_create_without_a_device_is_a_device_error(L):
    if L._lib.device_count() >= 1:
        pytest.skip("a HIP device is present: tests/test_gpu_text_search.py creates handles")
    h = _vp()
    assert L._lib.lib.lynse_hip_text_create(0, C.byref(h)) == DEVICE and not h
    with pytest.raises(L._lib.LynseHipError):
        L.TextIndex(device=0)


def test_text_kernels_have_no_scratch():
    import lynsedb_amd

    rep = Path(lynsedb_amd.__file__).parent / "csrc" / "resource_usage.txt"
    assert rep.exists(), "the build writes csrc/resource_usage.txt"
    blocks = re.findall(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", rep.read_text(), flags=re.S)
    for kernel in ("k_text_scan", "k_text_stats"):
        mine = [(n, int(s)) for n, s in blocks if kernel in n]
        assert mine and all(s == 0 for _, s in mine), (kernel, mine)
