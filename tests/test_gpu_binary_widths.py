"""Packed-binary scans (Hamming / Jaccard / Tanimoto / Dice over u64 words) at every width class and stage edge.

Reference: the oracle's integer popcounts and one correctly rounded division per pair, in the canonical (distance, row)
order (canonical_topk_packed; canonical_topk_filtered for subsets).  Row ids, counts and the f32 distance BITS are compared
with array_equal — nothing here is measured, so there is no tolerance — and EVERY query of every batch is checked.  The
canonical order makes top-k a prefix of top-k' for k < k': the oracle runs once per query at the largest k and is sliced.

Which instantiation of k_scan_binary_rows<KIND, WCAP, ODD> a row of W words reaches (launch_scan_binary_rows_k dispatches
on W & 1, then on the first WCAP >= W; `fast` is the kernel's `!ODD && W == WCAP && WCAP >= 2`, every other width walks
its pieces through park(); odd widths move 8-byte pieces, even ones 16-byte pieces; WCAP 64 runs without the prefetch):

      W        WCAP  ODD    fast                 W        WCAP  ODD    fast
      1          1   true   no                   2          2   false  yes
      3          4   true   no                   4          4   false  yes
      5, 7       8   true   no                   6          8   false  no
      9 .. 15   16   true   no                   8          8   false  yes
      17 .. 31  32   true   no                   10 .. 14  16   false  no
      33 .. 63  64   true   no                   16        16   false  yes
                                                 18 .. 30  32   false  no
                                                 32        32   false  yes
                                                 34 .. 62  64   false  no
                                                 64        64   false  yes
      W >= 65: k_scan_binary_wide (eight lanes per row, any width)

A subset filter always takes the lane-per-row kernel (or the wide one) with its row mask.  Unfiltered Hamming batches of
>= 72 queries over >= 65,536 rows run on the FP4 matrix path instead (k_bits_to_fp4, then k_scan_qs for 2 / 4 / 8 slabs
of 256 bits and k_scan_h16 for every other slab count).  The 8-lanes-per-row predecessor k_scan_binary only runs when
LYNSE_HIP_BIN_ROWS_MINQ (read once per process) is above the batch size: this suite cannot reach it.
"""
import functools

import numpy as np
import pytest

import oracle as O
from conftest import oracle_for_every_query

pytestmark = pytest.mark.gpu

f32 = np.float32
METRICS = ["hamming", "jaccard", "tanimoto", "dice"]
METRIC_ID = {"hamming": O.HAMMING, "jaccard": O.JACCARD, "tanimoto": O.TANIMOTO, "dice": O.DICE}

WIDTHS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 15, 16, 17, 18, 31, 32, 33, 34, 62, 63, 64, 65]
FILTER_WIDTHS = [1, 3, 5, 6, 12, 33, 64, 65]

N_BIG = 4389            # 4096 + 256 + 37: an emit-all stage, then a threshold stage of one full 256-row block and a 37-row partial wave
STAGE_EDGE = 4096       # stage0_rows of the default plan
ZERO_ROWS = (0, 30, 4200)            # all-zero rows: 0/0 -> distance 0.0 for Jaccard / Dice, ties resolved by row
COPIES = np.arange(4090, 4101)       # copies of row 5: one tie class on both sides of the stage edge
COPIED = 5
NQ_MAX = 33             # one past SCAN_BQ_SMALL


def bits_of(W):
    """A partial last word (64 W - 3 bits) for half the widths, a full one for the others — odd and even widths in both halves."""
    return 64 * W - 3 if WIDTHS.index(W) % 4 in (0, 3) else 64 * W


@pytest.fixture(scope="module")
def L():
    import lynsedb_amd as L_

    assert L_._lib.device_count() >= 1, "no HIP device: GPU tests need the MI355X box"
    return L_


def clear_tail(words, bits):
    if bits % 64:
        words[:, -1] &= np.uint64((1 << (bits % 64)) - 1)
    return words


def flip_bits(words, bits, rng, count):
    """`count` distinct bits below `bits` flipped in one packed row."""
    out = words.copy()
    for b in rng.choice(bits, size=count, replace=False):
        out[int(b) // 64] ^= np.uint64(1) << np.uint64(int(b) % 64)
    return out


@functools.lru_cache(maxsize=2)
def width_rows(W, bits=None):
    """(bits, rows u64[N_BIG, W]): Bernoulli rows (p = 0.1 for W <= 2: few set bits, so equal Jaccard / Dice ratios from different
    (numerator, denominator) pairs are common), three all-zero rows, and the copies of row 5 across the stage edge."""
    from lynsedb_amd.datasets import packed_bernoulli

    bits = bits_of(W) if bits is None else bits
    rows = clear_tail(packed_bernoulli(N_BIG, bits, 0.1 if W <= 2 else 0.5, 7000 + W), bits)
    rows[list(ZERO_ROWS)] = 0
    rows[COPIES] = rows[COPIED]
    rows.setflags(write=False)
    return bits, rows


def width_queries(W, bits, rows, n):
    """33 queries over rows[:n] and the row each was made from (-1: the all-zero query): row 5 with two bits flipped, the all-zero
    query, row 5 itself, then rows of the shard with 1..3 bits flipped.  A batch of nq queries is the first nq of them."""
    rng = np.random.default_rng(100 * W + n)
    src = [COPIED, -1, COPIED] + [int(r) for r in rng.integers(0, n, NQ_MAX - 3)]
    q = np.zeros((NQ_MAX, W), np.uint64)
    q[0] = flip_bits(rows[COPIED], bits, rng, 2)
    q[2] = rows[COPIED]
    for i in range(3, NQ_MAX):
        q[i] = flip_bits(rows[src[i]], bits, rng, 1 + i % 3)
    return q, np.array(src)


def unpack_f32(words, bits):
    """Packed rows as f32 0/1 rows of `bits` columns."""
    b = np.unpackbits(np.ascontiguousarray(words).view(np.uint8), axis=1, bitorder="little")
    return np.ascontiguousarray(b[:, :bits].astype(f32))


def width_case(W, n):
    bits, rows = width_rows(W)
    queries, src = width_queries(W, bits, rows, n)
    return bits, rows[:n], queries, src


def ks_of(n):
    return (1, 10, 100) + ((n, n + 5) if n <= 65 else ())


def expected_packed(oracle, queries, rows, k, metric):
    return oracle_for_every_query(lambda qi: oracle.canonical_topk_packed(queries[qi], rows, k, METRIC_ID[metric]), queries.shape[0])


def has_tie_at_k(want, n):
    """Some query made from a random row (not the copied row, not the all-zero query) has its k-th and (k+1)-th canonical
    distances equal for one of the k in use — from the oracle's numbers alone."""
    for qi in range(3, len(want)):
        d = want[qi][1]
        for k in ks_of(n):
            if k < len(d) and d[k - 1] == d[k]:
                return True
    return False


def straddles_stage_edge(want):
    return any((ids[:100] < STAGE_EDGE).any() and (ids[:100] >= STAGE_EDGE).any() for ids, _ in want)


def assert_topk(got, want, k, tag):
    """Every query: count, ids and distance bits equal the first k entries of the oracle's list."""
    rows, dists, counts = got
    assert rows.shape[0] == len(want) == dists.shape[0] == counts.shape[0], tag
    for qi, (e_ids, e_d) in enumerate(want):
        e_ids, e_d = e_ids[:k], e_d[:k]
        c = int(counts[qi])
        assert c == len(e_ids), (tag, qi, c, len(e_ids))
        assert np.array_equal(np.asarray(dists[qi, :c]).view(np.uint32), e_d.view(np.uint32)), (tag, qi, dists[qi, :c][:8], e_d[:8], rows[qi, :c][:8], e_ids[:8])
        assert np.array_equal(np.asarray(rows[qi, :c]).astype(np.uint32), e_ids), (tag, qi, rows[qi, :c][:12], e_ids[:12], e_d[:12])


# ------------------------------------------------------------------ 1. width classes of the lane-per-row kernel, the 64 / 65 switch

@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("W", WIDTHS)
def test_every_width_class_and_stage_edge(L, oracle, W, metric):
    tie_seen = False
    for n in (37, 65, N_BIG):        # one partial wave; one full wave + one row; two stages with a partial last wave
        bits, rows, queries, _ = width_case(W, n)
        kmax = min(n, 101)            # one past the largest k below n: the (k+1)-th distance of the tie check
        want = expected_packed(oracle, queries, rows, kmax, metric)
        tie_seen = tie_seen or has_tie_at_k(want, n)
        if n == N_BIG:
            assert straddles_stage_edge(want), "no query's top-100 has rows on both sides of the stage edge"
            # the all-zero query: all-zero rows first (0/0 -> 0.0 for Jaccard / Dice), a tie resolved by row
            assert want[1][0][0] == 0 and want[1][1][0] == 0.0 and want[1][1][2] == 0.0
        idx = L.FlatIndex(None, bits)
        idx.write_packed(rows)
        for nq in (1, 5, NQ_MAX):
            for k in ks_of(n):
                got = idx.search_packed_arrays(queries[:nq], k, metric)
                assert_topk(got, want[:nq], k, (metric, W, bits, n, nq, k))
    if W <= 2:
        assert tie_seen, "no query with equal k-th and (k+1)-th distances: the tie handling would pass vacuously"


# ------------------------------------------------------------------ 2. subset filters (masked scan)

@functools.lru_cache(maxsize=2)
def filter_case(W):
    """f32 0/1 rows of the width-class data (the device packs them lazily: k_pack_bits, tail bits included) and 33 f32 queries."""
    bits = bits_of(W) if W in WIDTHS else 64 * W - 3
    _, rows = width_rows(W, bits)
    queries, _ = width_queries(W, bits, rows, N_BIG)
    return bits, unpack_f32(rows, bits), unpack_f32(queries, bits)


def filter_subsets(W):
    rng = np.random.default_rng(300 + W)
    n = N_BIG
    forty = np.sort(rng.choice(n, int(0.4 * n), replace=False)).astype(np.uint64)
    return {
        # sorted, about 40 % of the rows, a few duplicates and ids >= n (skipped / counted once)
        "forty_percent": np.sort(np.concatenate([forty, forty[[3, 3, 500, 1700]], np.array([n, n + 7, n + 100_000], np.uint64)])),
        "smaller_than_k": np.array([0, 5, 30, 4090, 4096, 4100, 4388], np.uint64),             # 7 rows < k = 10, both sides of the edge
        "beyond_stage_edge": np.arange(STAGE_EDGE, n, 2, dtype=np.uint64),                      # the emit-all stage emits sentinels only
        "empty": np.zeros(0, np.uint64),
    }


@pytest.mark.parametrize("metric", ["hamming", "jaccard", "dice"])
@pytest.mark.parametrize("W", FILTER_WIDTHS)
def test_subset_filters_at_every_width_class(L, oracle, W, metric):
    bits, data, queries = filter_case(W)
    n, kmax = N_BIG, 300
    words = oracle.pack_binary(data)
    qwords = oracle.pack_binary(queries)
    idx = L.FlatIndex(None, bits, 0)
    idx.write(data)
    first = True
    for name, subset in filter_subsets(W).items():
        want = oracle_for_every_query(lambda qi: oracle.canonical_topk_filtered(None, None, kmax, METRIC_ID[metric], subset, packed_query=qwords[qi],
                                                                                packed_rows=words), NQ_MAX) if subset.size else None
        bitset = L.BitSet.from_rows(subset, n)
        for nq in (3, NQ_MAX):
            for k in (10, kmax):
                by_ids = idx.search_filtered_batch_arrays(queries[:nq], k, metric, subset)
                by_bits = idx.search_filtered_bitset_batch_arrays(queries[:nq], k, metric, bitset.words)
                for entry, got in (("ids", by_ids), ("bitset", by_bits)):
                    if subset.size == 0:
                        assert not got[2].any(), (metric, W, name, entry, nq, k, got[2])
                    else:
                        assert_topk(got, want[:nq], k, (metric, W, bits, name, entry, nq, k))
        if first:   # the first binary search packed the f32 rows on the device
            assert np.array_equal(idx.read_packed(0, n), words), (W, bits)
            first = False


# ------------------------------------------------------------------ 3. batched Hamming on the matrix path

N_MFMA = 65_536          # the matrix path's row floor (bin_mfma_eligible)
NQ_MFMA = 72             # and its batch floor


@functools.lru_cache(maxsize=1)
def mfma_case(bits, n_extra=300):
    """(words u64[65,536 + 300, W], 72 queries): rows with a few bits flipped; the first four queries are copies of rows among the last
    300 (distance 0 there: after an append the NEW rows must win)."""
    from lynsedb_amd.datasets import packed_bernoulli

    n = N_MFMA + n_extra
    words = clear_tail(packed_bernoulli(n, bits, 0.5, 500 + bits), bits)
    rng = np.random.default_rng(bits)
    qw = words[rng.integers(0, N_MFMA, NQ_MFMA)].copy()
    qw[:, 0] ^= np.uint64(0x5A5A)
    qw[:4] = words[[N_MFMA, N_MFMA + 150, N_MFMA + 298, N_MFMA + 299]]
    words.setflags(write=False)
    return words, qw


def in_pieces_of_32(idx, qw, k):
    """The same batch sent 32 queries at a time: the popcount kernels answer those."""
    parts = [idx.search_packed_arrays(qw[i:i + 32], k, "hamming") for i in range(0, qw.shape[0], 32)]
    return tuple(np.concatenate([p[j] for p in parts]) for j in range(3))


def assert_same(a, b, tag):
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), tag


@pytest.mark.parametrize("bits", [1600, 4160, 700])      # 7, 17 and 3 slabs of 256 bits; the last: rows wider than 4096 bits
def test_matrix_path_slab_counts(L, oracle, bits):
    words, qw = mfma_case(bits)
    n = words.shape[0]
    idx = L.FlatIndex(None, bits)
    idx.write_packed(words)
    idx.finalize()
    want = expected_packed(oracle, qw, words, 50, "hamming")
    for k in (5, 50):
        got = idx.search_packed_arrays(qw, k, "hamming")
        assert idx.coarse_state()["bpm_rows"] == n       # the +-1 copy was built: the matrix path ran
        assert_topk(got, want, k, (bits, k))
        assert_same(got, in_pieces_of_32(idx, qw, k), (bits, k))


@pytest.mark.parametrize("n,nq,on_matrix_path", [(N_MFMA - 1, NQ_MFMA, False), (N_MFMA, NQ_MFMA - 1, False), (N_MFMA, NQ_MFMA, True)])
def test_matrix_path_eligibility_edges(L, oracle, n, nq, on_matrix_path):
    words, qw = mfma_case(700)
    words, qw = words[:n], qw[:nq]
    idx = L.FlatIndex(None, 700)
    idx.write_packed(words)
    want = expected_packed(oracle, qw, words, 50, "hamming")
    for k in (5, 50):
        assert_topk(idx.search_packed_arrays(qw, k, "hamming"), want, k, (n, nq, k))
    assert idx.coarse_state()["bpm_rows"] == (n if on_matrix_path else 0)


@pytest.mark.parametrize("reserved", [False, True])
def test_matrix_path_copy_grows_with_the_shard(L, oracle, reserved):
    """Rows appended after the +-1 copy was built: ensure_bpm_locked converts rows [n_bpm, n) only — into a new allocation, or in place
    when the capacity was reserved up front."""
    words, qw = mfma_case(700)
    n = words.shape[0]
    idx = L.FlatIndex(None, 700)
    if reserved:
        idx.reserve(n)
    idx.write_packed(words[:N_MFMA])
    want = expected_packed(oracle, qw, words[:N_MFMA], 50, "hamming")
    assert_topk(idx.search_packed_arrays(qw, 50, "hamming"), want, 50, ("before", reserved))
    assert idx.coarse_state()["bpm_rows"] == N_MFMA
    idx.write_packed(words[N_MFMA:])
    want = expected_packed(oracle, qw, words, 50, "hamming")
    for qi in range(4):   # the appended copies of the queries win
        assert want[qi][0][0] >= N_MFMA and want[qi][1][0] == 0.0
    for k in (5, 50):
        got = idx.search_packed_arrays(qw, k, "hamming")
        assert_topk(got, want, k, ("after", reserved, k))
    assert idx.coarse_state()["bpm_rows"] == n == len(idx)


# ------------------------------------------------------------------ 4. device-resident entry points, appends, large k

@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("W", [3, 6, 65])
def test_device_entry_points_equal_the_host_entries(L, oracle, W, metric):
    import torch

    dev = torch.device("cuda", 0)
    bits, rows, queries, _ = width_case(W, N_BIG)
    host = L.FlatIndex(None, bits)
    host.write_packed(rows)
    twin = L.FlatIndex(None, bits)
    d_rows = torch.as_tensor(rows.copy().view(np.int64), device=dev)
    twin.write_packed_device(d_rows[:1500].contiguous())           # two appends of unequal size
    twin.write_packed_device(d_rows[1500:].contiguous())
    assert len(twin) == N_BIG
    assert np.array_equal(twin.read_packed(0, N_BIG), rows)
    d_q = torch.as_tensor(queries.view(np.int64), device=dev)
    want = expected_packed(oracle, queries, rows, 100, metric)
    for k in (10, 100):
        o_r = torch.zeros((NQ_MAX, k), dtype=torch.int64, device=dev)
        o_d = torch.zeros((NQ_MAX, k), dtype=torch.float32, device=dev)
        o_c = torch.zeros(NQ_MAX, dtype=torch.int32, device=dev)
        twin.search_packed_device(d_q, k, metric, o_r, o_d, o_c)
        torch.cuda.synchronize()
        got = (o_r.cpu().numpy().view(np.uint64), o_d.cpu().numpy(), o_c.cpu().numpy().view(np.uint32))
        assert_topk(got, want, k, (metric, W, k, "device"))
        assert_same(got, host.search_packed_arrays(queries, k, metric), (metric, W, k))


def test_packed_rows_appended_after_a_search(L, oracle):
    W, metric, k = 5, "jaccard", 10
    bits, rows, queries, _ = width_case(W, N_BIG)
    rng = np.random.default_rng(41)
    more = clear_tail(rng.integers(0, np.iinfo(np.uint64).max, size=(200, W), dtype=np.uint64, endpoint=True), bits)
    more[10:10 + NQ_MAX] = queries                                 # copies of the queries: the new rows must win
    idx = L.FlatIndex(None, bits)
    idx.write_packed(rows)
    assert_topk(idx.search_packed_arrays(queries, k, metric), expected_packed(oracle, queries, rows, k, metric), k, "before")
    idx.write_packed(more)
    both = np.concatenate([rows, more])
    want = expected_packed(oracle, queries, both, k, metric)
    assert all(w[0][0] >= N_BIG or qi in (1, 2) for qi, w in enumerate(want))   # (the all-zero query and row 5 itself tie with earlier rows)
    assert_topk(idx.search_packed_arrays(queries, k, metric), want, k, "after")
    assert np.array_equal(idx.read_packed(0, both.shape[0]), both)


def test_f32_rows_appended_after_the_lazy_pack(L, oracle):
    """dim 300: five words with a 44-bit tail.  The second search packs rows [n_packed, n) only: k_pack_bits on offset pointers."""
    dim, k = 300, 10
    _, rows = width_rows(5, dim)
    data = unpack_f32(rows, dim)
    qwords, _ = width_queries(5, dim, rows, N_BIG)
    queries = unpack_f32(qwords, dim)
    rng = np.random.default_rng(43)
    more = (rng.random((200, dim)) < 0.5).astype(f32)
    more[10:10 + NQ_MAX] = queries
    idx = L.FlatIndex(None, dim, 0)
    idx.write(data)
    words = oracle.pack_binary(data)
    assert np.array_equal(words, rows)
    assert_topk(idx.search_batch_arrays(queries, k, "hamming"), expected_packed(oracle, qwords, words, k, "hamming"), k, "before")
    idx.write(more)
    both = np.concatenate([words, oracle.pack_binary(more)])
    assert_topk(idx.search_batch_arrays(queries, k, "hamming"), expected_packed(oracle, qwords, both, k, "hamming"), k, "after")
    assert np.array_equal(idx.read_packed(0, both.shape[0]), both)


def test_large_k_over_a_width_that_is_no_power_of_two(L, oracle):
    """k above cap / 4 over more than cap rows: search_large_k's row-range views over the packed rows (W = 5: padded query words, odd
    pieces, ranges that start at any row)."""
    from lynsedb_amd.datasets import packed_bernoulli

    n, W, metric = 20_000, 5, "jaccard"
    bits = 64 * W - 3
    rows = clear_tail(packed_bernoulli(n, bits, 0.5, 77), bits)
    rows[[0, 17_000]] = 0
    rng = np.random.default_rng(78)
    queries = np.stack([flip_bits(rows[r], bits, rng, 2) for r in (5, 9_999, 19_999)] + [np.zeros(W, np.uint64)])
    idx = L.FlatIndex(None, bits)
    idx.write_packed(rows)
    want = expected_packed(oracle, queries, rows, n, metric)
    for k in (5000, n + 5):           # the second is clamped to n
        assert_topk(idx.search_packed_arrays(queries, k, metric), want, k, k)
