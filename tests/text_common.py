"""Shared by tests/test_text_modes.py and tests/test_gpu_text_search.py: the compiled restatement (tests/text_ref/text_ref.c), the
corpus and query generators of the text tests and the expected result of a search.  TEST INFRASTRUCTURE."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np

from conftest import oracle_for_every_query

HERE = Path(__file__).resolve().parent
f32, u8, u32, u64 = np.float32, np.uint8, np.uint32, np.uint64
_vp = C.c_void_p
NO_ROW = u64(0xFFFFFFFFFFFFFFFF)


def _p(a):
    return a.ctypes.data_as(_vp)


class Corpus:
    """n documents, document-major: doc_ptr u64[n + 1], doc_term u32 ascending within a document, doc_tf u32; doc_len = the tf sums"""

    def __init__(self, doc_ptr, doc_term, doc_tf, vocab):
        self.doc_ptr = np.ascontiguousarray(doc_ptr, u64)
        self.doc_term = np.ascontiguousarray(doc_term, u32)
        self.doc_tf = np.ascontiguousarray(doc_tf, u32)
        self.vocab = int(vocab)
        self.n = self.doc_ptr.size - 1
        self.doc_len = np.add.reduceat(np.append(self.doc_tf, 0).astype(np.int64), self.doc_ptr[:-1].astype(np.int64)).astype(u32) \
            if self.n else np.zeros(0, u32)
        assert int(self.doc_ptr[-1]) == self.doc_term.size == self.doc_tf.size and (self.n == 0 or self.doc_len.min() >= 1)

    @staticmethod
    def of(docs, vocab):
        """[{term id: tf}] -> Corpus"""
        ptr = np.zeros(len(docs) + 1, u64)
        ptr[1:] = np.cumsum([len(d) for d in docs])
        terms = [t for d in docs for t in sorted(d)]
        tfs = [d[t] for d in docs for t in sorted(d)]
        return Corpus(ptr, terms, tfs, vocab)

    def docs(self):
        return [{int(t): int(c) for t, c in zip(self.doc_term[int(a):int(b)], self.doc_tf[int(a):int(b)])}
                for a, b in zip(self.doc_ptr[:-1], self.doc_ptr[1:])]

    def csc(self):
        """-> (term_ptr u64[V + 1], post_row u32 ascending within a term, post_tf u32): what lynse_hip_text_set takes"""
        row = np.repeat(np.arange(self.n, dtype=np.int64), np.diff(self.doc_ptr.astype(np.int64)))
        order = np.argsort(self.doc_term, kind="stable")   # (the entries come ascending by row: a stable sort by term keeps that)
        term_ptr = np.zeros(self.vocab + 1, u64)
        np.cumsum(np.bincount(self.doc_term, minlength=self.vocab), out=term_ptr[1:])
        return term_ptr, row[order].astype(u32), self.doc_tf[order]


class Queries:
    """nq queries in CSR of (term id, count), slot order"""

    def __init__(self, lists):
        self.lists = [(np.asarray(t, u32), np.asarray(c, u32)) for t, c in lists]
        self.ptr = np.zeros(len(lists) + 1, u64)
        self.ptr[1:] = np.cumsum([t.size for t, _ in self.lists])
        self.terms = np.concatenate([t for t, _ in self.lists]) if lists else np.zeros(0, u32)
        self.counts = np.concatenate([c for _, c in self.lists]) if lists else np.zeros(0, u32)

    def __len__(self):
        return len(self.lists)

    def arrays(self):
        return self.ptr, self.terms, self.counts


class Ref:
    def __init__(self, lib):
        self.lib = lib

    def weights(self, docs, total, df, count, k):
        df, count = np.ascontiguousarray(df, u64), np.ascontiguousarray(count, u32)
        avg = C.c_float(0)
        w, cand = np.zeros(max(df.size, 1), f32), np.zeros(max(df.size, 1), u32)
        self.lib.tr_weights(int(docs), int(total), _p(df), _p(count), df.size, int(k), C.byref(avg), _p(w), _p(cand))
        return f32(avg.value), w[:df.size], cand[:df.size]

    def search(self, c: Corpus, terms, counts, k, live=None, reversed_=False):
        """one query -> dict(score f32[n], result bool[n], matched u8[n], docs, total, df, w, cand, passed)"""
        terms, counts = np.ascontiguousarray(terms, u32), np.ascontiguousarray(counts, u32)
        T = terms.size
        score, result, matched = np.zeros(c.n, f32), np.zeros(max(c.n, 1), u8), np.zeros(max(c.n, 1), u8)
        stats, w, cand = np.zeros(2 + T, u64), np.zeros(max(T, 1), f32), np.zeros(max(T, 1), u32)
        lv = None if live is None else np.ascontiguousarray(live, u8)
        passed = self.lib.tr_search(_p(c.doc_len), _p(c.doc_ptr), _p(c.doc_term), _p(c.doc_tf), c.n, None if lv is None else _p(lv),
                                    _p(terms), _p(counts), T, int(k), int(reversed_), _p(score), _p(result), _p(matched), _p(stats), _p(w), _p(cand))
        return dict(score=score, result=result[:c.n].astype(bool), matched=matched[:c.n], docs=int(stats[0]), total=int(stats[1]),
                    df=stats[2:].copy(), w=w[:T], cand=cand[:T], passed=int(passed))

    def batch(self, c: Corpus, q: Queries, k, live=None, reversed_=False):
        out = [None] * len(q)

        def one(i):
            out[i] = self.search(c, q.lists[i][0], q.lists[i][1], k, live, reversed_)

        oracle_for_every_query(one, len(q))
        return out


def build_ref(tmp_dir) -> Ref:
    cc = next((c for c in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang") if shutil.which(c)), None)
    assert cc, "no C compiler for tests/text_ref/text_ref.c"
    so = Path(tmp_dir) / "libtext_ref.so"
    subprocess.run([cc, "-O2", "-shared", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-o", str(so),
                    str(HERE / "text_ref" / "text_ref.c"), "-lm"], check=True)
    lib = C.CDLL(str(so))
    lib.tr_weights.restype = None
    lib.tr_weights.argtypes = [C.c_uint64, C.c_uint64, _vp, _vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_float), _vp, _vp]
    lib.tr_search.restype = C.c_uint64
    lib.tr_search.argtypes = [_vp, _vp, _vp, _vp, C.c_uint64, _vp, _vp, _vp, C.c_uint32, C.c_uint32, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp]
    return Ref(lib)


def popularity(vocab):
    """1 / rank"""
    p = 1.0 / np.arange(1, vocab + 1)
    return p / p.sum()


def gen_corpus(rng, n, vocab, mu=3.5, sigma=0.6, lo=1, hi=300) -> Corpus:
    """lengths log-normal(mu, sigma) clipped to [lo, hi]; every token drawn from the 1 / rank popularity"""
    lens = np.clip(np.rint(rng.lognormal(mu, sigma, n)), lo, hi).astype(np.int64)
    doc = np.repeat(np.arange(n, dtype=np.int64), lens)
    tok = rng.choice(vocab, size=int(lens.sum()), p=popularity(vocab)).astype(np.int64)
    key, tf = np.unique(doc * vocab + tok, return_counts=True)   # ascending by (document, term)
    ptr = np.zeros(n + 1, u64)
    np.cumsum(np.bincount(key // vocab, minlength=n), out=ptr[1:])
    return Corpus(ptr, key % vocab, tf, vocab)


def gen_queries(rng, nq, vocab, lo=3, hi=12) -> Queries:
    """lo..hi distinct terms from the 1 / rank popularity in drawing order (= slot order), a quarter of the counts 2 or 3"""
    p = popularity(vocab)
    out = []
    for _ in range(nq):
        t = rng.choice(vocab, size=int(rng.integers(lo, hi + 1)), replace=False, p=p)
        c = np.where(rng.random(t.size) < 0.25, rng.integers(2, 4, t.size), 1)
        out.append((t, c))
    return Queries(out)


def order_of(ref_one):
    """the rows of one query's results in result order: (score descending, row ascending)"""
    rows = np.nonzero(ref_one["result"])[0]
    return rows[np.lexsort((rows, -ref_one["score"][rows].astype(np.float64)))]


def check_batch(got, refs, k, what=None):
    """rows, counts, passer counts and score bits of every query of the batch against the restatement"""
    rows, scores, counts, passed = got
    assert rows.shape == (len(refs), k) and scores.shape == (len(refs), k)
    for qi, r in enumerate(refs):
        order = order_of(r)
        e_r, e_s = order[:k].astype(u64), r["score"][order[:k]]
        c = int(counts[qi])
        assert int(passed[qi]) == order.size == r["passed"], (what, qi, int(passed[qi]), order.size)
        assert c == e_r.size, (what, qi, c, e_r.size)
        assert np.array_equal(rows[qi, :c], e_r), (what, qi, rows[qi, :c][:12], e_r[:12])
        assert np.array_equal(scores[qi, :c].view(u32), e_s.view(u32)), (what, qi, scores[qi, :c][:12], e_s[:12])
        assert np.all(rows[qi, c:] == NO_ROW) and np.all(np.isneginf(scores[qi, c:])), (what, qi)
