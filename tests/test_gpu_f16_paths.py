"""GPU: VectorDtype::F16 shards (lynse_hip_flat_set_dtype) on every path and width an F16 shard reaches.

The reference is the CPU restatement: oracle.canonical_topk_f16 over oracle.round_f16(rows) (sequential f32 sums of simd.rs:805-846,
canonical (distance, row) order), asked for EVERY query of every batch; row ids, counts and the 32 bits of every distance must be
equal.  Non-finite rows / queries follow the pinned order of include/lynse_hip.h applied to oracle.all_distances_f16."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
from conftest import oracle_for_every_query

pytestmark = pytest.mark.gpu
f32 = np.float32
u32 = np.uint32
METRICS = [(O.IP, "ip"), (O.L2, "l2"), (O.COS, "cosine")]
UNSUPPORTED = 9   # LYNSE_ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def L():
    import lynsedb_amd as L_

    assert L_._lib.device_count() >= 1, "no HIP device: GPU tests need the MI355X box"
    return L_


def f16_bits(a):
    """IEEE binary16 words of f32 values (numpy's cast is RNE; oracle.round_f16 agrees with it on every rounding boundary)."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.ascontiguousarray(np.asarray(a, f32).astype(np.float16)).view(np.uint16)


def same_f32(a, b):
    """Bit equality of two f32 arrays, NaN compared as NaN (payloads are not part of the contract)."""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(u32)[~na], b.view(u32)[~nb])


def make_f16(L, oracle, data, reserve=None):
    """An F16 shard of `data`: the first half enters as f32 (rounded on the device, k_f32_to_f16_rows), the second half as the u16
    words of an F16 segment file.  What the shard reads back must be the restatement's rounding, bit for bit."""
    n, dim = data.shape
    idx = L.FlatIndex(None, dim, dtype="f16")
    if reserve:
        idx.reserve(reserve)
    h = n // 2
    if h:
        idx.write(data[:h])
    idx.write_f16_bits(f16_bits(data[h:]))
    decoded = oracle.round_f16(data)
    assert same_f32(idx.read_rows(0, n), decoded)
    return idx, decoded


def expect_all(oracle, decoded, queries, k, metric):
    return oracle_for_every_query(lambda qi: oracle.canonical_topk_f16(queries[qi], decoded, k, metric), queries.shape[0])


def assert_results(got, want, tag, to_rows=None, first=0):
    """Every query, every returned slot: count, row ids, distance bits."""
    rows, dists, counts = got
    for qi in range(rows.shape[0]):
        e_ids, e_d = want[first + qi]
        c = int(counts[qi])
        assert c == len(e_ids), (tag, qi, c, len(e_ids))
        e_rows = e_ids.astype(np.uint64) if to_rows is None else to_rows(e_ids)
        g_d = np.ascontiguousarray(dists[qi, :c], f32)
        assert np.array_equal(g_d.view(u32), e_d.view(u32)), (tag, qi, g_d[:6], e_d[:6], rows[qi, :6], e_rows[:6])
        assert np.array_equal(np.asarray(rows[qi, :c]).astype(np.uint64), e_rows), (tag, qi, rows[qi, :8], e_rows[:8])


def nan_rule_model(oracle, q, decoded, k, metric):
    """include/lynse_hip.h, NON-FINITE VALUES, over the f16 kernels' own arithmetic: NaN = the worst value of the metric, then the
    canonical (score best-first, row ascending) order."""
    d = np.asarray(oracle.all_distances_f16(q, decoded, metric), f32)
    asc = metric != O.IP
    d = np.where(np.isnan(d), f32(np.inf if asc else -np.inf), d).astype(f32)
    order = np.lexsort((np.arange(len(d)), d if asc else -d))
    return order[:k].astype(u32), d[order[:k]]


def gaussian_shard(rng, n, dim, nq, scale=2.0):
    data = (rng.standard_normal((n, dim)) * scale).astype(f32)
    queries = (data[rng.integers(0, n, nq)] + 0.1 * scale * rng.standard_normal((nq, dim))).astype(f32)
    return data, queries


def device_tensors(torch, nq, k):
    dev = torch.device("cuda", 0)
    return (torch.zeros((nq, k), dtype=torch.int64, device=dev), torch.zeros((nq, k), dtype=torch.float32, device=dev),
            torch.zeros(nq, dtype=torch.int32, device=dev))


def to_host(t):
    r, d, c = t
    return r.cpu().numpy().view(np.uint64), d.cpu().numpy(), c.cpu().numpy().view(u32)


# ------------------------------------------------------------------ 1. widths
# exact_score_f16seq: the fast path takes D % 8 == 0 (64-element steps, a tail of (D % 64) / 8 groups), every other width the one-lane
# loop.  rescore_keys stages an f16 row through LDS while it has at most MAXV * SEL_NT / 8 = 8 * 512 / 8 = 512 16-byte pieces
# (4,096 halves) — the scratch behind the keys, sel_lds_bytes = min(cap * 8 + 48 KB, 150 KB), holds the query and 8 such rows up to
# ~7,400 halves, so the piece count is the limit that binds: 3072 is INSIDE the LDS route, 5120 BEYOND it (direct loads).
FAST_FULL = [384, 768, 1024, 1536, 3072]      # D % 64 == 0: 6, 12, 16, 24 and 48 full steps
FAST_TAIL = [200, 776, 1000]                  # D % 64 = 8, 8, 40: a tail of 1, 1 and 5 groups behind 3, 12 and 15 full steps
PADDED = [56, 120]                            # f16 pitch padded to 64 / 128 halves (lynse_hip_flat_create): the tail runs 7 groups over a padded row
ONE_LANE = [770, 1023, 1]                     # D % 8 != 0
BEYOND_LDS = [5120]                           # 640 pieces > 512


@pytest.mark.parametrize("dim", FAST_FULL + FAST_TAIL + PADDED + ONE_LANE + BEYOND_LDS)
def test_f16_widths_every_batch_size(L, oracle, dim):
    n = max(3000, min(40_000, 6_000_000 // dim))
    rng = np.random.default_rng(1000 + dim)
    data, queries = gaussian_shard(rng, n, dim, 300)
    data[5] = 0          # a zero row: cosine distance 1.0 by the `== 0` rule
    queries[7] = 0       # a zero query: cosine 1.0 against every row, ties by row
    idx, decoded = make_f16(L, oracle, data)
    idx.profile_enable(True)
    k = 10
    for metric, name in METRICS:
        want = expect_all(oracle, decoded, queries, k, metric)
        for nq in (1, 8, 40, 256, 300):           # 300: two chunks, the second of 44
            idx.profile_get(reset=True)
            got = idx.search_batch_arrays(queries[:nq], k, name)
            plan = int(idx.profile_get(reset=True)["last_plan"])
            last_chunk = nq if nq <= 256 else nq - 256
            assert not plan & 32, (name, nq, hex(plan))                       # never the fused few-query kernel (it reads f32 rows)
            assert bool(plan & 16) == (last_chunk <= 32), (name, nq, hex(plan))  # the <= 32-query kernel exactly for those batches
            assert_results(got, want, (dim, name, nq))


@pytest.mark.parametrize("dim", [96, 100, 768, 1023])
def test_f16_zero_rows_and_zero_query_come_back_at_cosine_one(L, oracle, dim):
    """k = n: every row is returned, so the zero rows (cosine distance exactly 1.0 by the `== 0` rule, on the fast path and in the
    one-lane loop) are part of the compared answer, and so is a zero query (1.0 against every row, rows in order)."""
    rng = np.random.default_rng(2000 + dim)
    n = 200
    data, queries = gaussian_shard(rng, n, dim, 9)
    data[[3, 77, 150]] = 0
    data[150, dim // 2] = 1e-9        # rounds to zero in f16: a zero row only after the append
    queries[8] = 0
    idx, decoded = make_f16(L, oracle, data)
    assert not decoded[150].any()
    for metric, name in METRICS:
        for nq in (1, 9):
            got = idx.search_batch_arrays(queries[9 - nq:], n, name)
            want = expect_all(oracle, decoded, queries[9 - nq:], n, metric)
            if metric == O.COS:
                assert np.all(want[-1][1] == 1.0) and np.array_equal(want[-1][0], np.arange(n))
                assert all(np.all(w[1][np.isin(w[0], [3, 77, 150])] == 1.0) and np.isin(w[0], [3, 77, 150]).sum() == 3 for w in want)
            assert_results(got, want, (dim, name, nq))


# ------------------------------------------------------------------ 2. rounding at append
def _boundary_values():
    """For every finite f16 value h >= 0 and its successor (the one after 65,504 being 65,536 = what rounds to inf): the f32 midpoint
    and its two f32 neighbours, both signs: 31,744 * 3 * 2 = 190,464 values."""
    h = np.arange(0x7C00, dtype=np.uint16)
    lo = h.view(np.float16).astype(np.float64)
    hi = np.append(lo[1:], 65536.0)
    mid = ((lo + hi) / 2).astype(f32)                       # exact: 12 significant bits at most
    assert np.array_equal(mid.astype(np.float64), (lo + hi) / 2)
    tri = np.stack([np.nextafter(mid, f32(-np.inf)), mid, np.nextafter(mid, f32(np.inf))], axis=1).reshape(-1)
    out = np.concatenate([tri, -tri]).astype(f32)
    assert out.size == 190_464
    return out


def test_f32_rows_round_to_nearest_even_at_every_f16_boundary(L, oracle):
    extra = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1.1754942e-38, 2.9802322e-08, 2.98023224e-08 * 0.999, 5.9604645e-08,
                      65504.0, 65505.0, 65512.0, 65519.0, 65519.996, -65519.996, 65520.0, -65520.0, 65521.0, 65536.0, 70000.0, -70000.0,
                      1e10, -1e10, 3.4028235e38, -3.4028235e38, np.inf, -np.inf, np.nan, -np.nan, 0.5, 0.5001, 0.5003, 1.0], f32)
    nan_payload = np.array([0x7FC00001, 0x7F800001, 0xFFC12345, 0x7FFFFFFF], u32).view(f32)
    vals = np.concatenate([_boundary_values(), extra, nan_payload])
    dim = 64
    vals = np.concatenate([vals, np.zeros(-vals.size % dim, f32)]).reshape(-1, dim)
    assert same_f32(oracle.round_f16(vals), f16_bits(vals).view(np.float16).astype(f32))     # the reference is sound
    idx = L.FlatIndex(None, dim, dtype="f16")
    idx.write(vals[:1000])
    idx.write(vals[1000:])
    got = idx.read_rows(0, vals.shape[0])
    want = oracle.round_f16(vals)
    bad = np.nonzero(~((got.view(u32) == want.view(u32)) | (np.isnan(got) & np.isnan(want))))
    assert bad[0].size == 0, (bad[0].size, vals[bad][:8], got[bad][:8], want[bad][:8])
    # one-column and odd-width shards take the same conversion kernel at another pitch
    flat = vals.reshape(-1)
    for d in (1, 33):
        v = np.ascontiguousarray(flat[::37].reshape(-1, 1) if d == 1 else flat[: (flat.size // d) * d].reshape(-1, d))
        i2 = L.FlatIndex(None, d, dtype="f16")
        i2.write(v)
        assert same_f32(i2.read_rows(0, v.shape[0]), oracle.round_f16(v)), d


def test_f16_bits_round_trip_of_every_bit_pattern(L, oracle):
    bits = np.arange(65536, dtype=np.uint16).reshape(1024, 64)
    idx = L.FlatIndex(None, 64, dtype="f16")
    idx.write_f16_bits(bits)
    got = idx.read_rows(0, 1024)
    want = bits.view(np.float16).astype(f32)
    assert same_f32(got, want)
    assert np.array_equal(np.signbit(got[~np.isnan(got)]), np.signbit(want[~np.isnan(want)]))
    assert same_f32(oracle.round_f16(want), want)     # every f16 value is a fixed point of the rounding


# ------------------------------------------------------------------ 3. scale transitions of the shadow
def _search_all_metrics(oracle, idx, decoded, queries, tag, k=10):
    for metric, name in METRICS:
        for nq in (40, 256):
            want = expect_all(oracle, decoded, queries[:nq], k, metric)
            assert_results(idx.search_batch_arrays(queries[:nq], k, name), want, (tag, name, nq))


def _copies(idx, cap, ld16):
    """1 or 2: f16 row copies the shard holds (hbm_bytes: rows + own shadow + norms + int8 codes of at most half a copy)."""
    base = cap * ld16 * 2
    b = idx.hbm_bytes()
    assert b >= base, (b, base)
    return 1 if b < 2 * base else 2


def test_f16_shadow_alias_to_own_buffer_and_back(L, oracle):
    """ensure_shadow_locked: max |v| in [2^-6, 2^15) -> the f16 bits ARE the shadow (one copy); outside -> a scaled copy of its own."""
    rng = np.random.default_rng(31)
    dim, n0, n1 = 64, 30_000, 10_000
    # (a) alias -> own: rows ~ 1, then rows with max |v| >= 2^15
    a0 = rng.standard_normal((n0, dim)).astype(f32)
    a1 = (rng.standard_normal((n1, dim)) * 6000.0).astype(f32)
    a1[3, 5] = 40000.0
    idx, dec0 = make_f16(L, oracle, a0, reserve=n0 + n1)
    q0 = (a0[rng.integers(0, n0, 256)] + 0.1 * rng.standard_normal((256, dim))).astype(f32)
    _search_all_metrics(oracle, idx, dec0, q0, "a0")
    assert _copies(idx, n0 + n1, dim) == 1
    idx.write(a1)
    both = np.concatenate([a0, a1])
    dec = oracle.round_f16(both)
    assert same_f32(idx.read_rows(0, n0 + n1), dec)
    q1 = np.concatenate([q0[:128], (a1[rng.integers(0, n1, 128)] + 50.0 * rng.standard_normal((128, dim))).astype(f32)])
    _search_all_metrics(oracle, idx, dec, q1, "a1")
    assert _copies(idx, n0 + n1, dim) == 2
    # (b) own -> alias: max |v| < 2^-6 (a scaled-up shadow of its own), then rows near 1: the owned buffer is freed
    s = f32(2.0 ** -10)
    b0 = (rng.standard_normal((n0, dim)) * s).astype(f32)
    assert np.abs(b0).max() < 2.0 ** -6
    b1 = rng.standard_normal((n1, dim)).astype(f32)
    idx, dec0 = make_f16(L, oracle, b0, reserve=n0 + n1)
    q0 = (b0[rng.integers(0, n0, 256)] + 0.1 * s * rng.standard_normal((256, dim))).astype(f32)
    _search_all_metrics(oracle, idx, dec0, q0, "b0")
    assert _copies(idx, n0 + n1, dim) == 2
    idx.write(b1)
    both = np.concatenate([b0, b1])
    dec = oracle.round_f16(both)
    q1 = np.concatenate([q0[:128], (b1[rng.integers(0, n1, 128)] + 0.1 * rng.standard_normal((128, dim))).astype(f32)])
    _search_all_metrics(oracle, idx, dec, q1, "b1")
    assert _copies(idx, n0 + n1, dim) == 1


def test_f16_shard_of_subnormal_rows(L, oracle):
    """(c) every element an f16 subnormal (|v| < 2^-14, integer multiples of 2^-24): exact in f16, a scaled shadow of its own."""
    rng = np.random.default_rng(32)
    n, dim = 30_000, 64
    m = rng.integers(-1023, 1024, (n, dim))
    data = (m * 2.0 ** -24).astype(f32)
    idx, decoded = make_f16(L, oracle, data, reserve=n)
    assert np.array_equal(decoded.view(u32), data.view(u32))
    queries = (data[rng.integers(0, n, 256)] + rng.integers(-60, 61, (256, dim)) * 2.0 ** -24).astype(f32)
    _search_all_metrics(oracle, idx, decoded, queries, "subnormal")
    assert _copies(idx, n, dim) == 2


# ------------------------------------------------------------------ 4. non-finite rows and queries
@pytest.mark.parametrize("n,dim,nq,k", [(64, 96, 1, 64), (64, 96, 8, 64), (64, 96, 40, 64), (5000, 96, 3, 20), (5000, 96, 40, 20),
                                         (100_000, 128, 2, 10), (300_000, 128, 64, 10), (300_000, 256, 64, 10), (20_000, 768, 40, 10)])
def test_f16_nan_and_infinite_rows_and_queries(L, oracle, n, dim, nq, k):
    """The f16 twin of test_gpu_flat_parity.py::test_nan_and_infinite_rows_and_queries.  NaN / +-inf rows enter as bits (second half);
    rows of the first half turn infinite only through the f32 -> f16 overflow at append (|v| >= 65,520)."""
    rng = np.random.default_rng(3 + n + nq)
    data = rng.standard_normal((n, dim)).astype(f32)
    h = n // 2
    sp = h + rng.choice(n - h, 12, replace=False)
    data[sp[0:4], 3] = np.nan
    data[sp[4:6], 5] = np.inf
    data[sp[6:8], 5] = -np.inf
    data[sp[8], 1] = np.inf
    data[sp[8], 2] = -np.inf                                # (IP / L2 of this row: inf - inf)
    ov = rng.choice(h, 5, replace=False)
    data[ov[0:2], 4] = 65520.0                              # the smallest f32 that becomes +inf
    data[ov[2], 4] = -70000.0
    data[ov[3], 6] = 65519.996                              # stays 65,504
    data[ov[4], 1] = 1e10
    data[ov[4], 2] = -1e10
    queries = rng.standard_normal((nq, dim)).astype(f32)
    queries[:, 1] = np.abs(queries[:, 1])
    queries[:, 2] = np.abs(queries[:, 2])
    if nq > 1:
        queries[-1, 7] = np.nan                             # every score NaN
    if nq > 2:
        queries[-2, 9] = np.inf
    idx, decoded = make_f16(L, oracle, data)
    assert np.isposinf(decoded[ov[0], 4]) and np.isneginf(decoded[ov[2], 4]) and decoded[ov[3], 6] == 65504.0
    idx.finalize()
    for metric, name in METRICS:
        got = idx.search_batch_arrays(queries, k, name)
        want = oracle_for_every_query(lambda qi: nan_rule_model(oracle, queries[qi], decoded, k, metric), nq)
        assert_results(got, want, (name, n, dim, nq))
    if nq > 1:      # the all-NaN query of the pinned rule, spelled out
        rows, dists, counts = idx.search_batch_arrays(queries, k, "cosine")
        kk = min(k, n)
        assert int(counts[-1]) == kk and np.array_equal(rows[-1, :kk], np.arange(kk, dtype=rows.dtype)) and np.all(np.isposinf(dists[-1, :kk]))
    if n >= 300_000 and dim >= 256 and nq >= 33:            # (IP batches over 128 columns stay on the f16 shadow: k_scan_qh)
        assert idx.coarse_state()["i8c_strikes"] == -1      # the certified int8 pass switched itself off for this shard


# ------------------------------------------------------------------ 5. every entry point an F16 shard accepts
@pytest.mark.parametrize("strategy", ["direct", "mask", "bitset"])
@pytest.mark.parametrize("dim", [96, 768])
def test_f16_filtered_search(L, oracle, dim, strategy, monkeypatch):
    """Subset filters on an F16 shard: the gathered-rows strategy (1), the row bitmask (2), and the BitSet-words entry point."""
    if strategy != "bitset":
        monkeypatch.setenv("LYNSE_HIP_FILTER_STRATEGY", "1" if strategy == "direct" else "2")
    n = 20_000 if dim == 96 else 8000
    rng = np.random.default_rng(50 + dim)
    data, queries = gaussian_shard(rng, n, dim, 256)
    idx, decoded = make_f16(L, oracle, data)
    k = 10
    for m in (200, n // 3, (9 * n) // 10):
        subset = np.sort(rng.choice(n, m, replace=False)).astype(np.uint64)
        sub_rows = np.ascontiguousarray(decoded[subset.astype(np.int64)])
        words = np.zeros((n + 63) // 64 + 1, np.uint64)
        np.bitwise_or.at(words, (subset // 64).astype(np.int64), np.uint64(1) << (subset % np.uint64(64)))
        words[-1] = np.uint64(0xFF)                       # bits beyond len: ignored
        for metric, name in METRICS:
            want = expect_all(oracle, sub_rows, queries, k, metric)
            for nq in (2, 40, 256):
                if strategy == "bitset":
                    got = idx.search_filtered_bitset_batch_arrays(queries[:nq], k, name, words)
                else:
                    got = idx.search_filtered_batch_arrays(queries[:nq], k, name, subset)
                assert_results(got, want, (dim, strategy, m, name, nq), to_rows=lambda e: subset[e.astype(np.int64)])


@pytest.mark.parametrize("nq", [3, 40, 300])
def test_f16_top1(L, oracle, nq):
    rng = np.random.default_rng(60 + nq)
    data, queries = gaussian_shard(rng, 30_000, 128, nq)
    idx, decoded = make_f16(L, oracle, data)
    for metric, name in METRICS:
        assert_results(idx.search_batch_arrays(queries, 1, name), expect_all(oracle, decoded, queries, 1, metric), (name, nq))


@pytest.mark.parametrize("metric,name", [(O.IP, "ip"), (O.L2, "l2")])
def test_f16_large_k_up_to_the_server_cap(L, oracle, metric, name):
    """search_large_k over the rows_h view: k > cap / 4 over more than cap rows (shapes of test_large_k_up_to_the_server_cap)."""
    import torch

    rng = np.random.default_rng(21 + metric)
    n, dim = 50_000, 24
    data = rng.standard_normal((n, dim)).astype(f32)
    queries = np.ascontiguousarray(data[rng.integers(0, n, 3)] + 0.05, f32)
    idx, decoded = make_f16(L, oracle, data)
    for k in (10_000, 5000):
        assert_results(idx.search_batch_arrays(queries, k, name), expect_all(oracle, decoded, queries, k, metric), (name, k))
    k = 60_000      # device API + k > n
    t = device_tensors(torch, 1, k)
    idx.search_device(torch.as_tensor(queries[:1], device=t[0].device), k, name, *t)
    torch.cuda.synchronize()
    r, d, c = to_host(t)
    assert int(c[0]) == n
    assert_results((r, d, c), expect_all(oracle, decoded, queries[:1], n, metric), (name, k))


@pytest.mark.parametrize("metric,name", [(O.IP, "ip"), (O.L2, "l2")])
def test_f16_large_k_with_a_subset_filter(L, oracle, metric, name):
    rng = np.random.default_rng(33 + metric)
    n, dim = 45_000, 16
    data = rng.standard_normal((n, dim)).astype(f32)
    queries = np.ascontiguousarray(data[rng.integers(0, n, 2)] + 0.05, f32)
    idx, decoded = make_f16(L, oracle, data)
    subset = np.sort(rng.choice(n, 30_000, replace=False)).astype(np.uint64)
    sub_rows = np.ascontiguousarray(decoded[subset.astype(np.int64)])
    for k in (6000, 40_000):          # > cap / 4 = 4096; the second is clamped to the subset length
        want = expect_all(oracle, sub_rows, queries, k, metric)
        assert len(want[0][0]) == min(k, subset.size)
        assert_results(idx.search_filtered_batch_arrays(queries, k, name, subset), want, (name, k), to_rows=lambda e: subset[e.astype(np.int64)])
    some = np.concatenate([np.arange(100, 9000), np.arange(20_000, 26_000)]).astype(np.uint64)
    words = np.zeros((n + 63) // 64, np.uint64)
    np.bitwise_or.at(words, (some // 64).astype(np.int64), np.uint64(1) << (some % np.uint64(64)))
    want = expect_all(oracle, np.ascontiguousarray(decoded[some.astype(np.int64)]), queries, 5000, metric)
    assert_results(idx.search_filtered_bitset_batch_arrays(queries, 5000, name, words), want, (name, "bitset"), to_rows=lambda e: some[e.astype(np.int64)])
    dup = np.concatenate([some, some[:50], [n + 5]]).astype(np.uint64)
    assert_results(idx.search_filtered_batch_arrays(queries, 5000, name, dup), want, (name, "list"), to_rows=lambda e: some[e.astype(np.int64)])


def test_f16_device_resident_search_and_tickets(L, oracle):
    """search_device, and search_submit / wait with several tickets outstanding: batches of 8 (the f16 shadow) and of 200 (the
    certified int8 pass on a shard of this size) interleaved."""
    import torch

    rng = np.random.default_rng(71)
    n, dim, k = 70_000, 256, 10                     # >= 65,536 rows of 256 columns: 33..256-query batches take the int8 pass
    data = rng.random((n, dim), dtype=f32)
    idx, decoded = make_f16(L, oracle, data)
    idx.finalize()
    idx.profile_enable(True)
    dev = torch.device("cuda", 0)
    big = (data[rng.integers(0, n, 200)] + 0.02 * rng.standard_normal((200, dim))).astype(f32)
    small = (data[rng.integers(0, n, 8)] + 0.02 * rng.standard_normal((8, dim))).astype(f32)
    l2q = (data[rng.integers(0, n, 40)] + 0.02 * rng.standard_normal((40, dim))).astype(f32)
    dbig, dsmall, dl2 = (torch.as_tensor(x, device=dev) for x in (big, small, l2q))
    for q, dq, metric, name in ((big, dbig, O.IP, "ip"), (small, dsmall, O.COS, "cosine"), (l2q, dl2, O.L2, "l2")):
        t = device_tensors(torch, q.shape[0], k)
        idx.profile_get(reset=True)
        idx.search_device(dq, k, name, *t)
        torch.cuda.synchronize()
        plan = int(idx.profile_get(reset=True)["last_plan"])
        if q.shape[0] != 40:    # the 200-query batch ran the certified int8 pass, the 8-query batch the f16 shadow
            assert bool(plan & 4) == (q.shape[0] == 200), (name, hex(plan))
        assert_results(to_host(t), expect_all(oracle, decoded, q, k, metric), ("device", name))
    o1, o2, o3, o4 = device_tensors(torch, 200, k), device_tensors(torch, 8, k), device_tensors(torch, 40, k), device_tensors(torch, 200, k)
    idx.prepare("cosine", 200)      # derived copies are built under the exclusive lock: not while tickets are outstanding (submit says so)
    t1 = idx.search_submit(dbig, k, "ip", *o1)
    t2 = idx.search_submit(dsmall, k, "ip", *o2)
    t3 = idx.search_submit(dl2, k, "l2", *o3)
    t4 = idx.search_submit(dbig, k, "cosine", *o4)
    for t in (t4, t2, t1, t3):
        t.wait()
    torch.cuda.synchronize()
    assert_results(to_host(o1), expect_all(oracle, decoded, big, k, O.IP), "t1")
    assert_results(to_host(o2), expect_all(oracle, decoded, small, k, O.IP), "t2")
    assert_results(to_host(o3), expect_all(oracle, decoded, l2q, k, O.L2), "t3")
    assert_results(to_host(o4), expect_all(oracle, decoded, big, k, O.COS), "t4")


def test_f16_row_map_and_one_rank_sharded_entry(L, oracle):
    import torch

    from lynsedb_amd.sharded import NativeComm

    rng = np.random.default_rng(72)
    n, dim, nq, k = 30_000, 64, 40, 10
    data, queries = gaussian_shard(rng, n, dim, nq)
    part = L.FlatIndex(None, dim, dtype="f16")
    part.set_row_map(3, 1)                                  # rank 1 of 3: returned ids are global
    part.write(data[: n // 2])
    part.write_f16_bits(f16_bits(data[n // 2:]))
    decoded = oracle.round_f16(data)
    for metric, name in METRICS:
        assert_results(part.search_batch_arrays(queries, k, name), expect_all(oracle, decoded, queries, k, metric), ("row map", name),
                       to_rows=lambda e: e.astype(np.uint64) * 3 + 1)
    idx, decoded = make_f16(L, oracle, data)
    idx.finalize()
    comm = NativeComm(None, 0, 1, 0)
    assert comm.ranks_seen() == 1
    dq = torch.as_tensor(queries, device=torch.device("cuda", 0))
    for metric, name in METRICS:
        t = device_tensors(torch, nq, k)
        L._lib.check(L._lib.lib.lynse_hip_flat_search_sharded_f32_device(
            idx.handle, comm.handle, C.c_void_p(dq.data_ptr()), nq, k, L.metric_from_str(name), C.c_void_p(t[0].data_ptr()),
            C.c_void_p(t[1].data_ptr()), C.c_void_p(t[2].data_ptr())))
        torch.cuda.synchronize()
        assert_results(to_host(t), expect_all(oracle, decoded, queries, k, metric), ("sharded", name))


def test_f16_massive_ties_and_append_after_search(L, oracle):
    """Rows drawn from 16 distinct vectors: thousands of exactly equal distances, resolved by row.  Then an append after the search."""
    rng = np.random.default_rng(73)
    n, dim, k = 40_000, 96, 25
    protos = rng.standard_normal((16, dim)).astype(f32)
    data = np.ascontiguousarray(protos[rng.integers(0, 16, n)])
    queries = (protos[rng.integers(0, 16, 40)] + 0.1 * rng.standard_normal((40, dim))).astype(f32)
    idx, decoded = make_f16(L, oracle, data)
    for metric, name in METRICS:
        for nq in (3, 40):
            assert_results(idx.search_batch_arrays(queries[:nq], k, name), expect_all(oracle, decoded, queries[:nq], k, metric), ("ties", name, nq))
    extra = (queries[:20] + 0.01 * rng.standard_normal((20, dim))).astype(f32)     # the new best rows of half the queries
    idx.write(extra)
    decoded = np.concatenate([decoded, oracle.round_f16(extra)])
    assert len(idx) == n + 20
    for metric, name in METRICS:
        assert_results(idx.search_batch_arrays(queries, k, name), expect_all(oracle, decoded, queries, k, metric), ("append", name))


# ------------------------------------------------------------------ 6. binary metrics on an F16 shard
@pytest.mark.parametrize("dim", [64, 130, 1024])
def test_f16_binary_metrics(L, oracle, dim):
    """k_pack_bits<_Float16>: bit = (stored f16 value > 0.5).  f32 0.5001 is stored as 0.5 (bit 0 here, 1 on an f32 shard), 0.5003 as
    0.50049 (bit 1)."""
    rng = np.random.default_rng(80 + dim)
    n, nq, k = 20_000, 200, 10
    pool = np.array([0.0, 1.0, 0.5, 0.5001, 0.5003, 0.4999, 0.75, 0.25, np.nan, 3e-6, -3e-6, 6e-8, -1.0, 0.50024, 0.50025], f32)
    data = pool[rng.integers(0, pool.size, (n, dim))]
    queries = data[rng.integers(0, n, nq)].copy()
    flip = rng.random(queries.shape) < 0.1
    queries = np.where(flip, (queries <= 0.5).astype(f32), queries).astype(f32)
    idx, decoded = make_f16(L, oracle, data)
    words = oracle.pack_binary(decoded)
    f32_words = oracle.pack_binary(data)
    assert not np.array_equal(words, f32_words)          # the rounding does move bits across 0.5
    assert np.array_equal(idx.read_packed(0, n), words)
    qw = oracle.pack_binary(queries)                     # queries are f32: thresholded as they are (pack_binary_query)
    for metric, name in ((O.HAMMING, "hamming"), (O.JACCARD, "jaccard"), (O.DICE, "dice")):
        want = oracle_for_every_query(lambda qi: oracle.canonical_topk_packed(qw[qi], words, k, metric), nq)
        for b in (5, 40, nq):                            # 200 queries: the batched Hamming route is asked for
            assert_results(idx.search_batch_arrays(queries[:b], k, name), want, (dim, name, b))


# ------------------------------------------------------------------ 7. refusals stay refusals
def test_f16_refusals_and_no_fused_search(L, oracle):
    rng = np.random.default_rng(90)
    n, dim = 4000, 64
    data, queries = gaussian_shard(rng, n, dim, 4)
    idx, decoded = make_f16(L, oracle, data)
    rows, dists, counts = np.zeros((4, 5), np.uint64), np.zeros((4, 5), f32), np.zeros(4, u32)
    lib = L._lib.lib
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    assert lib.lynse_hip_flat_search_sq8_f32(idx.handle, p(queries), 4, 5, 0, p(rows), p(dists), p(counts)) == UNSUPPORTED
    assert lib.lynse_hip_flat_build_pq(idx.handle, 8, 16) == UNSUPPORTED
    idx.profile_enable(True)
    for nq in (1, 2, 3, 4):
        for metric, name in METRICS:
            idx.profile_get(reset=True)
            got = idx.search_batch_arrays(queries[:nq], 5, name)
            assert not int(idx.profile_get(reset=True)["last_plan"]) & 32, (nq, name)
            assert_results(got, expect_all(oracle, decoded, queries[:nq], 5, metric), (nq, name))
