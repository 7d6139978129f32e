"""Shared by tests/test_selection_planted_design.py (CPU) and tests/test_gpu_selection_planted.py: a numpy restatement of the selection
key (f32_to_ord, make_key, score_ord: csrc/common.h, csrc/pq.h), a model of the selection loop of ScoreCut::cut (csrc/rerank_host.inc,
k_pq_hist / k_pq_find) that counts the passes a query needs, the planted one-column datasets and the expected result of a range search
over a column of reference distances.  At dim = 1 the single-row kernels return the stored value (IP with the query [1.0]: 0 + 1 * v,
L1 with the query [0.0]: 0 + |0 - v|), so a column of f32 bit patterns IS the column of score images.  The model describes the inputs; the
expectation of a GPU test always comes from the oracle or the additive restatement.  TEST INFRASTRUCTURE."""
import numpy as np

f32, u32, u64 = np.float32, np.uint32, np.uint64

PQ_DIGIT = 11                      # csrc/pq.h
RANGE_FAIL = 0xFFFFFFFF            # csrc/range.h
HIST_BLOCK, HIST_TRIP, EMIT_TILE, RANGE_TILE = 8192, 2048, 2048, 128   # the row tilings a cluster should straddle
NO_ROW = u64(0xFFFFFFFFFFFFFFFF)
# digit -> the key bits it covers (image << 32 | row), high bit first: six passes of 11, 11, 11, 11, 11 and 9 bits
DIGITS = {1: (63, 53), 2: (52, 42), 3: (41, 31), 4: (30, 20), 5: (19, 9), 6: (8, 0)}


def bits_f32(bits):
    return np.asarray(bits, u32).view(f32)


# ---------------------------------------------------------------------------------------- the key ----
def f32_to_ord(x):
    b = np.ascontiguousarray(x, f32).view(u32)
    return np.where(b & u32(0x80000000), ~b, b | u32(0x80000000)).astype(u32)


def score_ord(s, asc):
    """the 32-bit image of a score: ascending = best first for the metric, NaN last, -0 == +0"""
    s = np.array(s, f32, copy=True, ndmin=1)
    s[np.isnan(s)] = np.inf if asc else -np.inf
    s = s + f32(0.0)
    o = f32_to_ord(s)
    return o if asc else ~o


def make_keys(images):
    """image << 32 | row for a column of images"""
    images = np.asarray(images, u32)
    return (images.astype(u64) << u64(32)) | np.arange(images.size, dtype=u64)


def range_images(scores, thr, asc):
    """the S row of k_range_scan for one query: the image of a passer, RANGE_FAIL for every other row"""
    with np.errstate(invalid="ignore"):
        ok = (scores <= f32(thr)) if asc else (scores >= f32(thr))
    return np.where(ok, score_ord(scores, asc), u32(RANGE_FAIL)).astype(u32)


# ------------------------------------------------------------------------------- the selection loop ----
def selection_passes(keys, need):
    """The passes of ScoreCut::cut for one query that starts {prefix 0, hi 64, need}: each takes the bucket of the next digit that holds
    rank `need`; done when that bucket holds exactly `need` keys or the last bit is fixed.  -> one dict per pass: the bucket taken, the
    keys in it, the rank still to find, and how many buckets of that digit the keys that still matched occupied."""
    keys = np.asarray(keys, u64)
    assert 1 <= need <= keys.size
    hi, out = 64, []
    while True:
        lo = max(hi - PQ_DIGIT, 0)
        w = hi - lo
        digit = ((keys >> u64(lo)) & u64((1 << w) - 1)).astype(np.int64)
        counts = np.bincount(digit, minlength=1 << w)
        cum = np.cumsum(counts)
        b = int(np.searchsorted(cum, need, "left"))      # the first bucket whose running count reaches `need`
        need -= int(cum[b] - counts[b])
        out.append({"bucket": b, "in_bucket": int(counts[b]), "need": need, "occupied": int((counts > 0).sum())})
        keys = keys[digit == b]
        hi = lo
        if counts[b] == need or lo == 0:
            return out


# ------------------------------------------------------------------------------------ the datasets ----
class Cut:
    """One named (threshold, cap) of a dataset.  `digit`: the digit the case is about — the selection cannot finish before it, and the
    keys that still match when it is histogrammed lie in more than one of its buckets."""

    def __init__(self, name, thr, cap, digit):
        self.name, self.thr, self.cap, self.digit = name, f32(thr), int(cap), int(digit)

    def __repr__(self):
        return f"{self.name}(cap={self.cap}, digit={self.digit})"


class Planted:
    """values: the column (every value positive, so the IP score of the query [1] and the L1 distance of the query [0] are both the
    value); asc: the direction it was built for (L1 ascending, IP descending); groups: name -> rows of a cluster"""

    def __init__(self, name, asc, values, cuts, groups):
        self.name, self.asc, self.values, self.cuts, self.groups = name, asc, np.ascontiguousarray(values, f32), cuts, groups
        self.n = self.values.size
        assert not np.signbit(self.values).any() and not np.isnan(self.values).any()

    @property
    def all_thr(self):
        return f32(np.inf) if self.asc else f32(-np.inf)


def _sides(asc, rng, n_better, n_worse):
    """distinct better and distinct worse values on either side of [1, 2), shuffled: ascending the better are the smaller"""
    lo = np.linspace(0.26, 0.49, max(n_better if asc else n_worse, 1)).astype(f32)
    hi = np.linspace(2.1, 3.9, max(n_worse if asc else n_better, 1)).astype(f32)
    better, worse = (lo, hi) if asc else (hi, lo)
    better, worse = better[:n_better], worse[:n_worse]
    assert np.unique(better).size == n_better and np.unique(worse).size == n_worse
    return rng.permutation(better), rng.permutation(worse)


def _column(n, rng, better, worse, clusters):
    """clusters: [(first row, values)] on runs of rows; the better values on random rows outside them, the worse ones on the rest"""
    v = np.zeros(n, f32)
    free = np.ones(n, bool)
    for r0, vals in clusters:
        assert free[r0:r0 + vals.size].all() and r0 + vals.size <= n
        v[r0:r0 + vals.size] = vals
        free[r0:r0 + vals.size] = False
    rest = rng.permutation(np.nonzero(free)[0])
    assert rest.size == better.size + worse.size
    v[rest[:better.size]] = better
    v[rest[better.size:]] = worse
    return v


def _straddles(r0, r1):
    """the run of rows [r0, r1) crosses a boundary of every row tiling behind the selection"""
    return all((r0 // t) != ((r1 - 1) // t) for t in (HIST_BLOCK, HIST_TRIP, EMIT_TILE, RANGE_TILE))


def _check_n(n):
    assert n % RANGE_TILE and n % HIST_TRIP and n % HIST_BLOCK
    return n


def digit2(asc):
    """900 better rows with distinct scores, a cluster of 2,000 values that share float bits 31..21 and differ in bits 20..10 (steps of
    2^10 ulps from 1.0) on rows [7000, 9000) in a shuffled order, worse rows behind"""
    rng = np.random.default_rng(202)
    n, nb, r0, m = _check_n(11003), 900, 7000, 2000
    cluster = bits_f32(0x3F800000 + (np.arange(m, dtype=np.int64) << 10))
    assert _straddles(r0, r0 + m) and (cluster.view(u32) >> 21 == 0x3F800000 >> 21).all()
    better, worse = _sides(asc, rng, nb, n - nb - m)
    v = _column(n, rng, better, worse, [(r0, rng.permutation(cluster))])
    thr = cluster.max() if asc else cluster.min()
    cuts = [Cut("first", thr, nb + 1, 2), Cut("middle", thr, nb + 1037, 2), Cut("last_but_one", thr, nb + m - 1, 2),
            Cut("middle_of_all_rows", np.inf if asc else -np.inf, nb + 611, 2)]
    return Planted("digit2", asc, v, cuts, {"cluster": np.arange(r0, r0 + m)})


def digit3(asc):
    """the same with a ladder of 1,024 consecutive floats from 1.0 (they share bits 31..10) on rows [7700, 8724)"""
    rng = np.random.default_rng(203)
    n, nb, r0, m = _check_n(11003), 900, 7700, 1024
    cluster = bits_f32(0x3F800000 + np.arange(m, dtype=np.int64))
    assert _straddles(r0, r0 + m) and (cluster.view(u32) >> 10 == 0x3F800000 >> 10).all()
    better, worse = _sides(asc, rng, nb, n - nb - m)
    v = _column(n, rng, better, worse, [(r0, rng.permutation(cluster))])
    thr = cluster.max() if asc else cluster.min()
    cuts = [Cut("first", thr, nb + 1, 3), Cut("middle", thr, nb + 517, 3), Cut("last_but_one", thr, nb + m - 1, 3),
            Cut("middle_of_all_rows", np.inf if asc else -np.inf, nb + 300, 3)]
    return Planted("digit3", asc, v, cuts, {"cluster": np.arange(r0, r0 + m)})


def rows_2p20(asc):
    """n = 2^20 + 4099: one group of equal values (1.0) on rows [2^20 - 300, 2^20 + 300), every other row worse.  The caps put the cut one
    row before row 2^20, exactly at it and one row after it: digit 4 (row bits 30..20) holds buckets 0 and 1"""
    rng = np.random.default_rng(204)
    n, r0, m = _check_n((1 << 20) + 4099), (1 << 20) - 300, 600
    _, worse = _sides(asc, rng, 0, n - m)
    v = _column(n, rng, np.zeros(0, f32), worse, [(r0, np.full(m, 1.0, f32))])
    assert _straddles(r0, r0 + m)
    cuts = [Cut("one_before_2p20", 1.0, 299, 4), Cut("at_2p20", 1.0, 300, 4), Cut("one_after_2p20", 1.0, 301, 4)]
    return Planted("rows_2p20", asc, v, cuts, {"group": np.arange(r0, r0 + m)})


def rows_512(asc):
    """Two groups of equal values, everything else worse.  `inside` (the best, 1.0) lies wholly inside the 512-row block 10, on rows
    [5200, 5400): digit 5 sees one bucket and digit 6 finishes.  `run` (the second best, 1.5) covers rows [7000, 9500), the blocks 13 to
    18: digit 5 picks the block and digit 6 finishes in the middle of it"""
    rng = np.random.default_rng(205)
    n = _check_n(11003)
    a0, am, b0, bm = 5200, 200, 7000, 2500
    va, vb = (1.0, 1.5) if asc else (1.5, 1.0)
    _, worse = _sides(asc, rng, 0, n - am - bm)
    v = _column(n, rng, np.zeros(0, f32), worse, [(a0, np.full(am, va, f32)), (b0, np.full(bm, vb, f32))])
    assert a0 // 512 == (a0 + am - 1) // 512 and _straddles(b0, b0 + bm) and a0 // RANGE_TILE != (a0 + am - 1) // RANGE_TILE
    mid = 8 * 1024 + 256 - b0 + 1    # the row in the middle of block 16 is the last one kept
    cuts = [Cut("inside_one_block", va, 100, 6), Cut("inside_one_block_all_rows", np.inf if asc else -np.inf, 199, 6),
            Cut("middle_of_block_16", vb, am + mid, 5), Cut("first_row_of_block_14", vb, am + 7168 - b0 + 1, 5),
            Cut("last_row_of_block_13", vb, am + 7168 - b0, 5), Cut("second_row_of_the_run", np.inf if asc else -np.inf, am + 2, 5)]
    return Planted("rows_512", asc, v, cuts, {"inside": np.arange(a0, a0 + am), "run": np.arange(b0, b0 + bm)})


def all_equal(asc):
    """every row has the same score; cap 7: digits 1 to 4 see one bucket, digit 5 six of them, digit 6 finishes"""
    n = _check_n(3001)
    return Planted("all_equal", asc, np.full(n, 1.25, f32), [Cut("seven", 1.25, 7, 5), Cut("seven_of_all_rows", np.inf if asc else -np.inf, 7, 5)],
                   {"all": np.arange(n)})


SORT_COUNTS = (1, 2, 3, 1024, 1025, 2048, 2049, 16383, 16384)   # passer counts at the edges of k_pool_select<256|1024> and its LDS


def sort_sizes(asc):
    """n = 40,000 for the sort boundaries: levels of equal values, best first, whose running sizes hit every count of SORT_COUNTS; every
    other level is a tie group of 4 on shuffled rows, so a group of 4 ends at and another begins after each boundary, and the caps 16385
    and 20000 of the host sort fall inside / at the end of one.  -> (values, the running sizes)"""
    rng = np.random.default_rng(206)
    sizes = [1, 1, 1] + [4] * 255 + [1, 1] + [4] * 255 + [3, 1] + [4] * 3583 + [2, 1] + [4] * 5904
    cum = np.cumsum(sizes)
    assert cum[-1] == 40000 and set(SORT_COUNTS) <= set(cum.tolist())
    level = np.repeat(np.arange(len(sizes)), sizes)
    bits = 0x3F800000 + 64 * (level if asc else len(sizes) - 1 - level)       # distinct values in [1, 2), better levels first
    v = np.empty(40000, f32)
    v[rng.permutation(40000)] = bits_f32(bits)
    return v, cum


FLT_MAX, FLT_MIN = f32(3.4028235e38), f32(1.1754944e-38)


def non_finite():
    """n = 1,003: normal values of both signs with ±inf, the largest and the smallest normal values, denormals, +0 and three NaN rows
    planted among them (no -0: make_key folds it into +0)"""
    rng = np.random.default_rng(207)
    n = 1003
    v = (rng.standard_normal(n) * np.exp2(rng.integers(-20, 20, n))).astype(f32)
    v[v == 0] = 1
    special = {0: np.nan, 500: np.nan, n - 1: np.nan, 3: np.inf, 130: np.inf, 64: -np.inf, 900: -np.inf, 7: FLT_MAX, 127: -FLT_MAX,
               128: FLT_MIN, 129: -FLT_MIN, 255: 1e-45, 256: -1e-45, 257: 5e-39, 600: 0.0}
    for r, x in special.items():
        v[r] = x
    v[601] = bits_f32([0x007FFFFF])[0]      # the largest denormal
    v[602] = bits_f32([0x807FFFFF])[0]
    assert not (np.signbit(v) & (v == 0)).any() and np.isnan(v).sum() == 3
    return v


DATASETS = {"digit2": digit2, "digit3": digit3, "rows_2p20": rows_2p20, "rows_512": rows_512, "all_equal": all_equal}
IP_SCALES = (1.0, 2.0, 0.5)   # the queries [1], [2], [0.5] scale every score exactly and keep the order


# --------------------------------------------------------------------------------- the expectation ----
class Column:
    """The reference's distances of one query to every row: the canonical order lexsort((row, distance in metric order)) computed once,
    the passers of a threshold a prefix of it.  -0 == +0; a NaN sorts last and never passes."""

    def __init__(self, d, asc):
        self.d, self.asc = np.ascontiguousarray(d, f32), asc
        key = self.d + f32(0.0)
        key = key if asc else -key
        self.order = np.lexsort((np.arange(key.size), key))
        self.sorted = key[self.order]
        self.n_nan = int(np.isnan(self.d).sum())

    def passed(self, thr):
        if np.isnan(thr):
            return 0
        t = f32(thr) if self.asc else -f32(thr)
        return int(np.searchsorted(self.sorted[:self.sorted.size - self.n_nan], t, "right"))

    def threshold_for(self, count):
        """the threshold that the `count` best rows pass (and whatever ties with the last of them)"""
        assert 1 <= count <= self.d.size - self.n_nan
        return self.d[self.order[count - 1]]

    @property
    def fail_thr(self):
        return f32(-np.inf) if self.asc else f32(np.inf)


def check_range(got, cols, thr, cap, what=None):
    """rows, counts, `passed`, f32 distance bits and the padding of one call against one Column per query"""
    rows, dists, counts, passed = got
    nq = len(cols)
    assert rows.shape == (nq, cap) and dists.shape == (nq, cap) and counts.shape == (nq,) and passed.shape == (nq,)
    for q, col in enumerate(cols):
        p = col.passed(thr[q])
        c = min(p, cap)
        e_rows = col.order[:c]
        assert int(passed[q]) == p, (what, q, thr[q], int(passed[q]), p)
        assert int(counts[q]) == c, (what, q, thr[q], int(counts[q]), c)
        assert np.array_equal(rows[q, :c], e_rows.astype(u64)), (what, q, thr[q], rows[q, :c][:8], e_rows[:8])
        assert np.array_equal(dists[q, :c].view(u32), col.d[e_rows].view(u32)), (what, q, thr[q])
        worst = f32(np.inf) if col.asc else f32(-np.inf)
        assert (rows[q, c:] == NO_ROW).all() and (dists[q, c:] == worst).all(), (what, q, thr[q])


def check_topk(got, col, nq, k, live=None, what=None):
    """search_batch_arrays under an ascending metric for nq copies of one query: the best min(k, live rows) of the Column (whose NaN
    distances were already made +inf, as the search reports them)"""
    rows, dists, counts = got
    order = col.order if live is None else col.order[live[col.order]]
    e_rows = order[:k]
    for q in range(nq):
        c = int(counts[q])
        assert c == e_rows.size, (what, q, c, e_rows.size)
        assert np.array_equal(rows[q, :c], e_rows.astype(u64)), (what, q, rows[q, :c][:8], e_rows[:8])
        assert np.array_equal(dists[q, :c].view(u32), col.d[e_rows].view(u32)), (what, q)
