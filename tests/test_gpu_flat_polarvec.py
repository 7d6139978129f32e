"""GPU parity tests for FLAT-{IP,L2,COS}-POLARVEC<b> (PolarVecIndex, src/storage/polarvec_mmap.rs; Collection, src/engine.rs:4593-4602,
:5514-5515, :5921-5934) through the C ABI and the Collection, against the restatement of tests/polarvec_common.py and
tests/polarvec_ref/polarvec_ref.c: every exact distance from the oracle's exported single-pair kernel, both canonical (score, row) cuts
in numpy.  Codes, sign words, dim_mins / dim_scales / residual_sq / inv_v_hat_norms bits (a NaN as a NaN), result ids and f32 distance
bits are compared; there are no tolerances."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import polarvec_common as PC
from conftest import oracle_for_every_query
from polarvec_common import COS, IP, L2, NAME, OVERSAMPLE, check_index, check_search, pow2

pytestmark = pytest.mark.gpu
assert (IP, L2, COS) == (O.IP, O.L2, O.COS)
f32 = np.float32


@pytest.fixture(scope="module")
def L():
    import lynsedb_amd as L_

    assert L_._lib.device_count() >= 1
    return L_


@pytest.fixture(scope="module")
def ref(tmp_path_factory, oracle):
    return PC.compile_ref(tmp_path_factory.mktemp("polarvec_ref")), C.cast(oracle.lib.lo_compute_distance, C.c_void_p)


def ref_search_ks(ref, data, enc, queries, ks, metric, pools=None):
    return PC.ref_search_ks(ref[0], ref[1], oracle_for_every_query, data, enc, queries, ks, metric, OVERSAMPLE, pools)


def ref_search(ref, data, enc, queries, k, metric):
    return ref_search_ks(ref, data, enc, queries, [k], metric)[k]


def make_index(L, data):
    idx = L.FlatIndex(None, data.shape[1], device=0)
    idx.write(data)
    return idx


def built(L, ref, data, bits, metric, idx=None):
    """index + the restatement's encoding, checked equal to the device's"""
    idx = make_index(L, data) if idx is None else idx
    idx.build_polarvec(bits, NAME[metric])
    enc = PC.ref_encode(ref[0], data, bits, metric)
    check_index(idx.polarvec_params(), enc, data.shape[1])
    return idx, enc


def dataset(rng, n, dim):
    data = rng.standard_normal((n, dim)).astype(f32)
    data[5] = 0.0                         # an all-zero row
    data[6] = -0.0
    data[7, : max(1, dim // 2)] = 1e-40   # denormals
    return data


def sign_of_dim0():
    return -1.0 if int(PC.sign_words(1)[0]) & 1 else 1.0


# ----------------------------------------------------------------------------- fit and encode parity ----
@pytest.mark.parametrize("dim", [1, 3, 5, 20, 64, 100, 300, 768])
def test_fit_and_encode_bit_equal(L, ref, dim):
    """n = 1003: the last block and the last 64-row tile are partial.  bits 1, 2, 3, 5 cross bytes (3 and 5 inside a code), 4 and 8 do
    not; each of the three built-for metrics keeps another correction array."""
    data = dataset(np.random.default_rng(dim), 1003, dim)
    idx = make_index(L, data)
    for bits in (1, 2, 3, 4, 5, 8):
        for metric in (IP, L2, COS):
            built(L, ref, data, bits, metric, idx)


def test_fit_and_encode_at_dim_1536(L, ref):
    data = dataset(np.random.default_rng(1536), 1003, 1536)
    for metric in (IP, L2, COS):
        built(L, ref, data, 4, metric)


# ------------------------------------------------------------------------------------- planted cases ----
def test_rounding_tie_is_half_away_from_zero(L, ref):
    """Dim 1, bits 1, ROTATED values {0, 1, 0.5}: dim_min = -0.05f, dim_scale = 1.1f and the raw code of 0.5 is exactly 0.5
    ((0.5 - (-0.05f)) / 1.1f == 0x3F000000), which rounds half away from zero to 1 and half to even to 0.  Sign bit 0 of the seed-42 sign
    words is SET, so dimension 0 is negated by the rotation: the rows are planted with that sign so that the rotated values are the
    ones above.  The literal rows {0, 1, 0.5} (rotated {-0, -1, -0.5}: no tie) are checked for parity as well."""
    s = sign_of_dim0()
    data = np.array([[0.0], [1.0], [0.5]], f32) * f32(s)
    idx, enc = built(L, ref, data, 1, IP)
    assert enc.mins.view(np.uint32)[0] == f32(-0.05).view(np.uint32) and enc.scales.view(np.uint32)[0] == 0x3F8CCCCD
    raw = f32(ref[0].plr_raw_code(0.5, float(enc.mins[0]), float(enc.scales[0])))
    assert raw.view(np.uint32) == 0x3F000000
    assert enc.codes[:, 0].tolist() == [0, 1, 1]
    assert idx.polarvec_params()["codes"][2, 0] == 1
    built(L, ref, np.array([[0.0], [1.0], [0.5]], f32), 1, IP)


@pytest.mark.parametrize("n", [40, 2100])
@pytest.mark.parametrize("first", [0.0, -0.0])
def test_sign_of_a_zero_minimum_follows_the_first_row(L, ref, n, first):
    """Dim 1, rows {+0, -0, +0, ...} and the same with the first two swapped: range 0, so dim_min is the raw minimum, and of the equal
    values +0 and -0 the earliest row's (after the rotation's sign) stays.  2,100 rows: the tie crosses blocks of the fit."""
    data = np.zeros((n, 1), f32)
    data[1::2] = -0.0
    if np.signbit(f32(first)):
        data[0], data[1] = -0.0, 0.0
    for bits in (1, 4):
        idx, enc = built(L, ref, data, bits, L2)
        want = f32(sign_of_dim0()) * data[0, 0]
        got = idx.polarvec_params()["dim_mins"]
        assert got.view(np.uint32)[0] == want.view(np.uint32) and enc.scales[0] == 1.0


def test_non_finite_rows_and_queries(L, ref):
    """An all-NaN column keeps (+inf, -inf): dim_min +inf, scale 1.  Columns with +inf, with +inf and -inf, a row of 3e38 (the rotation
    overflows).  The rotation mixes the columns, so the planted column is one of a dim-1 index; the dim-20 index takes whole rows."""
    for col in ([np.nan] * 70, [1.0, np.inf, 2.0] + [0.5] * 67, [1.0, np.inf, -np.inf] + [0.5] * 67, [np.nan, 1.0, -2.0] + [0.25] * 67):
        data = np.array(col, f32).reshape(-1, 1)
        for bits in (2, 4):
            for metric in (IP, L2, COS):
                idx, enc = built(L, ref, data, bits, metric)
        if np.isnan(data).all():
            assert np.isposinf(abs(enc.mins[0])) and enc.scales[0] == 1.0 and not enc.codes.any()
    rng = np.random.default_rng(77)
    dim = 20
    data = rng.standard_normal((2500, dim)).astype(f32)
    data[3] = np.nan
    data[50, 7] = np.nan
    data[90, 0] = np.inf
    data[91, 19] = -np.inf
    data[92, 3], data[92, 4] = np.inf, -np.inf
    data[94] = 3e38
    queries = rng.standard_normal((6, dim)).astype(f32)
    queries[1] = np.nan
    queries[2, 5] = np.nan
    queries[3, 0] = np.inf
    queries[4] = -np.inf
    queries[5] = 3e38
    for bits in (3, 4):
        for metric in (IP, L2, COS):
            idx, enc = built(L, ref, data, bits, metric)
            exp = ref_search_ks(ref, data, enc, queries, (1, 10), metric)
            for k in (1, 10):
                check_search(idx.search_polarvec_batch_arrays(queries, k, NAME[metric]), exp[k])
    # finite rows, non-finite queries: the tables are NaN / inf, the grid is not
    data = rng.standard_normal((2500, dim)).astype(f32)
    idx, enc = built(L, ref, data, 4, L2)
    for metric in (IP, L2, COS):
        check_search(idx.search_polarvec_batch_arrays(queries, 10, NAME[metric]), ref_search(ref, data, enc, queries, 10, metric))


@pytest.mark.parametrize("n", [50_001, 100_003])
def test_fit_samples_at_most_50000_rows(L, ref, n):
    """n = 50,001: stride 1 over the first 50,000 rows, row 50,000 is unsampled.  n = 100,003: stride 2, the odd rows are unsampled.
    Extreme values planted only in unsampled rows do not move the grid and clip to code 0 / levels - 1."""
    rng = np.random.default_rng(n)
    dim, bits = 8, 4
    data = rng.standard_normal((n, dim)).astype(f32)
    stride = 1 if n <= 50_000 else n // 50_000
    sampled = np.zeros(n, bool)
    sampled[np.arange(50_000) * stride] = True
    out = np.nonzero(~sampled)[0]
    assert out.size and (n != 50_001 or out.tolist() == [50_000]) and (n != 100_003 or (stride == 2 and 1 in out))
    idx, enc = built(L, ref, data, bits, L2)
    planted = data.copy()
    hi, lo = out[-1], out[0]                         # (the same row at n = 50,001)
    planted[hi] = planted[lo] = 0.0
    planted[hi, 0], planted[lo, 0] = 1e6, -1e6       # one coordinate: every rotated value of the row is +-1e6
    idx2, enc2 = built(L, ref, planted, bits, L2)
    p = idx2.polarvec_params()
    assert np.array_equal(p["dim_mins"].view(np.uint32), enc.mins.view(np.uint32))
    assert np.array_equal(p["dim_scales"].view(np.uint32), enc.scales.view(np.uint32))
    assert set(np.unique(p["codes"][[hi, lo]]).tolist()) <= {0x00, 0x0F, 0xF0, 0xFF}


# ------------------------------------------------------------------------------------- search parity ----
@pytest.mark.parametrize("metric", [IP, L2, COS])
@pytest.mark.parametrize("bits", [2, 3, 4, 8])
@pytest.mark.parametrize("dim", [1, 3, 5, 100, 300, 768])
def test_search_parity(L, ref, metric, bits, dim):
    """Every query of every batch.  Dim 3 at bits 3 (padded 4 < 8) is the all-zero table sum.  k = 1, 10 cut the pool by the radix
    selection (N = 20, 200), k = 100 by N = 2,000 of 3,000.  nq = 1, 3: single-query blocks; 7 and 256: groups of four, 7 ending in a
    partial one.  Padded 512 and 1,024 take several LDS chunks at bits 8 (and at bits 4 with four queries)."""
    rng = np.random.default_rng(dim * 100 + bits * 10 + metric)
    data = dataset(rng, 3000, dim)
    idx, enc = built(L, ref, data, bits, metric)
    for nq in (1, 3, 7, 256):
        queries = rng.standard_normal((nq, dim)).astype(f32)
        queries[0] = data[11]
        exp = ref_search_ks(ref, data, enc, queries, (1, 10, 100), metric)
        for k in (1, 10, 100):
            check_search(idx.search_polarvec_batch_arrays(queries, k, NAME[metric]), exp[k])


@pytest.mark.parametrize("bits", [1, 5, 6, 7])
def test_search_parity_of_the_other_generic_widths(L, ref, bits):
    """bits 1, 5, 6, 7 take the one-chain order with 2, 32, 64 and 128 table entries per dimension (6 and 7: single-query blocks)."""
    rng = np.random.default_rng(bits)
    data = dataset(rng, 1500, 100)
    idx, enc = built(L, ref, data, bits, L2)
    queries = rng.standard_normal((7, 100)).astype(f32)
    for metric in (L2, IP):
        check_search(idx.search_polarvec_batch_arrays(queries, 10, NAME[metric]), ref_search(ref, data, enc, queries, 10, metric))


def test_pool_of_every_row_at_1500_rows(L, ref):
    rng = np.random.default_rng(15)
    data = dataset(rng, 1500, 100)
    queries = rng.standard_normal((5, 100)).astype(f32)
    for bits in (3, 4):
        idx, enc = built(L, ref, data, bits, L2)
        assert min(100 * OVERSAMPLE, 1500) == 1500
        check_search(idx.search_polarvec_batch_arrays(queries, 100, "l2"), ref_search(ref, data, enc, queries, 100, L2))


@pytest.mark.parametrize("bits", [3, 4, 8])
def test_search_with_another_metric_than_the_build(L, ref, bits):
    """Built for IP: neither array, so L2 adds nothing and cosine multiplies by nothing.  Built for L2: cosine finds no multiplier."""
    rng = np.random.default_rng(40 + bits)
    data = dataset(rng, 3000, 100)
    queries = rng.standard_normal((7, 100)).astype(f32)
    for built_for, searched in ((IP, (L2, COS)), (L2, (COS, IP))):
        idx, enc = built(L, ref, data, bits, built_for)
        for metric in searched:
            check_search(idx.search_polarvec_batch_arrays(queries, 10, NAME[metric]), ref_search(ref, data, enc, queries, 10, metric))


@pytest.mark.parametrize("dim", [5, 100])
def test_duplicates_and_all_zero_query_tie_by_row(L, ref, dim):
    rng = np.random.default_rng(50 + dim)
    base = rng.standard_normal((50, dim)).astype(f32)
    data = np.concatenate([np.repeat(base, 40, axis=0), np.full((300, dim), 0.25, f32), np.zeros((200, dim), f32)])   # 2,500 rows
    queries = np.stack([np.zeros(dim, f32), base[3], rng.standard_normal(dim).astype(f32), np.full(dim, -0.0, f32)])
    for bits in (3, 4):
        idx, enc = built(L, ref, data, bits, IP)
        for k in (1, 10, 100):
            pools = {}
            exp = ref_search_ks(ref, data, enc, queries, [k], IP, pools)
            got = idx.search_polarvec_batch_arrays(queries, k, "ip")
            check_search(got, exp[k])
            # the all-zero query: every IP table entry is +-0, every row scores the same -> the pool is rows 0 .. N-1
            N = min(k * OVERSAMPLE, data.shape[0])
            assert np.array_equal(np.sort(pools[k][0]), np.arange(N))
            assert int(got[0][0].max()) < N


def test_pool_beyond_the_device_selection_and_pool_of_all_rows(L, ref):
    """n = 21,000.  k = 900: N = 18,000 > 16,384 keys, cut by the radix selection, scored on the device and selected on the host.
    k = 1,050: k * 20 = n, the pool is every row.  k = 30,000 > n: k' = n."""
    rng = np.random.default_rng(21)
    n, dim = 21_000, 100
    data = rng.standard_normal((n, dim)).astype(f32)
    idx, enc = built(L, ref, data, 4, L2)
    queries = rng.standard_normal((3, dim)).astype(f32)
    assert min(900 * OVERSAMPLE, n) == 18_000 and 1050 * OVERSAMPLE == n
    for metric in (IP, L2):
        exp = ref_search_ks(ref, data, enc, queries, (900, 1050), metric)
        for k in (900, 1050):
            check_search(idx.search_polarvec_batch_arrays(queries, k, NAME[metric]), exp[k])
    got = idx.search_polarvec_batch_arrays(queries[:1], 30_000, "l2")
    assert int(got[2][0]) == n
    check_search(got, ref_search(ref, data, enc, queries[:1], 30_000, L2))


def test_query_chunks_of_256(L, ref):
    """The search driver (coded_search, csrc/coded_host.inc) takes at most QCHUNK = 256 queries at a time: 257 run as 256 + 1, the last
    chunk a single-query block.  k = 1, 10: N = 20, 200 < 300 rows, so both chunks go through the radix selection."""
    rng = np.random.default_rng(257)
    data = dataset(rng, 300, 20)
    idx, enc = built(L, ref, data, 4, L2)
    queries = rng.standard_normal((257, 20)).astype(f32)
    queries[256] = data[11]
    for metric in (L2, IP):
        exp = ref_search_ks(ref, data, enc, queries, (1, 10), metric)
        for k in (1, 10):
            check_search(idx.search_polarvec_batch_arrays(queries, k, NAME[metric]), exp[k])


def test_query_chunks_at_the_table_cap(L, ref):
    """dim 1,100 -> padded 2,048 at bits 8: one query's table is 2,048 << 8 floats = 2 MiB, and a chunk's tables stay at or under
    256 MiB, so a chunk is 128 queries, fewer than QCHUNK; 130 run as 128 + 2.  The smallest padded width at which the cap binds."""
    rng = np.random.default_rng(1100)
    dim, bits = 1100, 8
    table_bytes = (pow2(dim) << bits) * 4
    assert pow2(dim) == 2048 and (256 << 20) // table_bytes == 128 < 256
    data = dataset(rng, 300, dim)
    idx, enc = built(L, ref, data, bits, L2)
    queries = rng.standard_normal((130, dim)).astype(f32)
    queries[129] = data[11]
    for metric in (L2, IP):
        exp = ref_search_ks(ref, data, enc, queries, (1, 10), metric)
        for k in (1, 10):
            check_search(idx.search_polarvec_batch_arrays(queries, k, NAME[metric]), exp[k])


def test_widest_padded_dim_and_the_lds_refusal(L, ref):
    """dim 20,000 -> padded 32,768: 128 KiB of LDS in the rotation kernels (the raised limit), 16,384 code bytes at bits 4.  dim 33,000
    -> padded 65,536 floats do not fit the 160 KiB: refused."""
    from lynsedb_amd._lib import LynseUnsupportedError

    rng = np.random.default_rng(20)
    data = rng.standard_normal((70, 20_000)).astype(f32)
    idx, enc = built(L, ref, data, 4, L2)
    queries = rng.standard_normal((5, 20_000)).astype(f32)
    for metric in (IP, L2):
        exp = ref_search(ref, data, enc, queries, 3, metric)
        check_search(idx.search_polarvec_batch_arrays(queries, 3, NAME[metric]), exp)
        check_search(idx.search_polarvec_batch_arrays(queries[:1], 3, NAME[metric]), exp[:1])
    wide = make_index(L, rng.standard_normal((3, 33_000)).astype(f32))
    with pytest.raises(LynseUnsupportedError):
        wide.build_polarvec(4, "l2")


# ------------------------------------------------------------------------ files, handles, refusals ----
def test_file_round_trip_and_appends(L, ref, tmp_path):
    from lynsedb_amd.storage import PolarvecIndexFile, load_polarvec_index, save_polarvec_index

    rng = np.random.default_rng(9)
    dim = 100
    data = rng.standard_normal((3000, dim)).astype(f32)
    queries = rng.standard_normal((9, dim)).astype(f32)
    for bits, metric in ((4, L2), (3, COS), (8, IP)):
        a, enc = built(L, ref, data, bits, metric)
        p = a.polarvec_params()
        save_polarvec_index(tmp_path / "polarvec_index.bin",
                            PolarvecIndexFile(dim, p["padded_dim"], p["bits"], p["sign_words"], p["dim_mins"], p["dim_scales"], p["codes"],
                                              p["residual_sq"], p["inv_v_hat_norms"]))
        f = load_polarvec_index(tmp_path / "polarvec_index.bin")
        assert f.flags == {IP: 0, L2: 1, COS: 2}[metric]
        b = make_index(L, data)
        b.load_polarvec(f.bits, f.sign_words, f.dim_mins, f.dim_scales, f.codes, f.residual_sq, f.inv_v_hat_norms)
        check_index(b.polarvec_params(), enc, dim)
        exp = ref_search(ref, data, enc, queries, 10, metric)
        check_search(a.search_polarvec_batch_arrays(queries, 10, NAME[metric]), exp)
        check_search(b.search_polarvec_batch_arrays(queries, 10, NAME[metric]), exp)
    # an index over fewer rows than the handle holds, with sign words of its own (one word where two are needed: the second
    # negates nothing)
    own = np.array([0xDEADBEEF12345678], np.uint64)
    enc2 = PC.ref_encode(ref[0], data[:1000], 4, L2, signs=own)
    b.load_polarvec(4, own, enc2.mins, enc2.scales, enc2.codes, enc2.residual, None)
    p2 = b.polarvec_params()
    assert p2["n"] == 1000 and p2["sign_words"].tolist() == [0xDEADBEEF12345678, 0] and p2["flags"] == 1
    assert np.array_equal(p2["codes"], enc2.codes)
    check_search(b.search_polarvec_batch_arrays(queries, 10, "l2"), ref_search(ref, data, enc2, queries, 10, L2))
    # rows appended after the build stay outside the index
    a.write(rng.standard_normal((500, dim)).astype(f32))
    assert a.polarvec_params(arrays=False)["n"] == 3000
    rows, _, counts = a.search_polarvec_batch_arrays(queries, 3000, "ip")
    assert int(counts.min()) == 3000 and int(rows[:, :3000].max()) < 3000
    check_search(a.search_polarvec_batch_arrays(queries, 10, "ip"), ref_search(ref, data, enc, queries, 10, IP))
    a.drop_polarvec()
    assert a.polarvec_params()["padded_dim"] == 0
    with pytest.raises(ValueError, match="no PolarVec index"):
        a.search_polarvec_batch_arrays(queries, 10, "l2")


def test_refusals(L):
    from lynsedb_amd._lib import LynseUnsupportedError

    rng = np.random.default_rng(1)
    data = rng.random((100, 64)).astype(f32)
    idx = make_index(L, data)
    for bits in (0, 9):
        with pytest.raises(ValueError, match=r"bits must be in \[1, 8\]"):
            idx.build_polarvec(bits, "l2")
    with pytest.raises(LynseUnsupportedError):
        idx.build_polarvec(4, "hamming")
    idx.build_polarvec(4, "l2")
    with pytest.raises(LynseUnsupportedError):
        idx.search_polarvec_batch_arrays(data[:2], 5, "hamming")
    rows, dists, counts = idx.search_polarvec_batch_arrays(data[:2], 0, "ip")
    assert rows.shape == (2, 0) and counts.tolist() == [0, 0]
    h16 = L.FlatIndex(None, 64, device=0, dtype="f16")
    h16.write(data)
    with pytest.raises(LynseUnsupportedError):
        h16.build_polarvec(4, "l2")
    packed = L.FlatIndex(None, 64, device=0)
    packed.write_packed(rng.integers(0, 1 << 63, (100, 1), dtype=np.uint64))
    with pytest.raises(LynseUnsupportedError):
        packed.build_polarvec(4, "l2")
    empty = L.FlatIndex(None, 64, device=0)
    with pytest.raises(ValueError, match="at least one vector"):
        empty.build_polarvec(4, "l2")
    p = idx.polarvec_params()
    with pytest.raises(ValueError):
        idx.load_polarvec(4, p["sign_words"], p["dim_mins"], p["dim_scales"], p["codes"][:, :4])          # bytes_per_vec of another dim
    big = np.zeros((101, 32), np.uint8)
    with pytest.raises(ValueError, match="more rows than the handle holds"):
        idx.load_polarvec(4, p["sign_words"], p["dim_mins"], p["dim_scales"], big)
    for mode in ("FLAT-HAMMING-POLARVEC4", "FLAT-L2-POLARVEC"):
        c = L.Collection("c", 64, device=0)
        c.add_items(data, list(range(100)))
        c.commit()
        with pytest.raises(NotImplementedError):
            c.build_index(mode)


def test_row_mutation_drops_the_index(L):
    """update_rows and compact release every auxiliary index of the handle, PolarVec among them."""
    rng = np.random.default_rng(8)
    data = rng.standard_normal((300, 16)).astype(f32)
    idx = make_index(L, data)
    for mutate in (lambda: idx.update_rows([3], data[:1]), lambda: idx.compact(np.arange(len(idx)) != 5)):
        idx.build_polarvec(4, "l2")
        assert idx.polarvec_params(arrays=False)["n"] == len(idx)
        mutate()
        assert idx.polarvec_params(arrays=False)["padded_dim"] == 0
        with pytest.raises(ValueError, match="no PolarVec index"):
            idx.search_polarvec_batch_arrays(data[:1], 3, "l2")


def test_stage_times(L):
    rng = np.random.default_rng(2)
    data = rng.standard_normal((5000, 32)).astype(f32)
    idx = make_index(L, data)
    idx.build_polarvec(4, "ip")
    idx.profile_enable(True)
    idx.polarvec_stage_times(reset=True)
    idx.search_polarvec_batch_arrays(data[:4], 10, "ip")
    assert idx.polarvec_stage_times()["searches"] == 1     # reading does not clear by default
    t = idx.polarvec_stage_times(reset=True)
    idx.profile_enable(False)
    assert t["searches"] == 1 and t["scan_us"] > 0 and t["rescore_us"] > 0
    assert idx.polarvec_stage_times()["searches"] == 0


# ---------------------------------------------------------------------------------------- Collection ----
def _collection(L, data, path=None, ids=None):
    c = L.Collection("plv", data.shape[1], device=0, path=path)
    c.add_items(data, list(range(data.shape[0])) if ids is None else list(ids))
    c.commit()
    return c


def _check_collection(c, ref, data, enc, q, k, metric, ids=None):
    exp = ref_search(ref, data, enc, q, k, metric)
    res = c.batch_search(q, k)
    for r, (e_r, e_d) in zip(res, exp):
        want = e_r if ids is None else np.asarray(ids, np.uint64)[e_r.astype(np.int64)]
        assert np.array_equal(np.asarray(r.ids(), np.uint64), want)
        assert np.array_equal(np.asarray(r.distances(), f32).view(np.uint32), e_d.view(np.uint32))


@pytest.mark.parametrize("bits", [3, 4, 8])
@pytest.mark.parametrize("name,metric", [("IP", IP), ("L2", L2), ("COS", COS), ("COSINE", COS)])
def test_collection_modes(L, ref, name, metric, bits):
    """Fails on a build without the feature: FLAT-*-POLARVEC<b> built nothing there and index_path was flat_mmap."""
    mode = f"FLAT-{name}-POLARVEC{bits}"
    rng = np.random.default_rng(len(mode) + bits)
    data = rng.standard_normal((4000, 64)).astype(f32)
    c = _collection(L, data)
    c.build_index(mode)
    enc = PC.ref_encode(ref[0], data, bits, metric)
    check_index(c._flat.polarvec_params(), enc, 64)
    q = rng.standard_normal((3, 64)).astype(f32)
    _check_collection(c, ref, data, enc, q, 10, metric)
    prof = c.search_profile(q[0], 10)["profile"]
    assert prof["index_path"] == "polarvec_two_pass"
    assert prof["rerank_us"] >= 0
    assert prof["device"]["polarvec_stages"]["scan_us"] > 0 and prof["device"]["polarvec_stages"]["rescore_us"] > 0


def test_collection_subset_pending_tombstones_and_rebuild(L, ref, oracle):
    rng = np.random.default_rng(3)
    data = rng.standard_normal((3000, 32)).astype(f32)
    c = _collection(L, data)
    c.build_index("FLAT-L2-POLARVEC4")
    enc = PC.ref_encode(ref[0], data, 4, L2)
    q = data[:2] + f32(0.01)
    # subset=: the exact filtered scan, never PolarVec candidates
    res = c.batch_search(q, 10, subset=np.arange(0, 3000, 2, dtype=np.uint64))
    for qi, r in enumerate(res):
        ids = np.asarray(r.ids())
        assert ids.size == 10 and np.all(ids % 2 == 0)
        e_ids, _ = oracle.canonical_topk(q[qi], data[::2], 10, L2)
        assert np.array_equal(ids, 2 * e_ids.astype(np.int64))
    assert c.search_profile(q[0], 10, subset=np.arange(10, dtype=np.uint64))["profile"]["index_path"] == "flat_mmap_filtered"
    # tombstones: search_k = k + |tombstones| goes into the PolarVec search, the deleted ids are filtered afterwards
    exp = ref_search(ref, data, enc, q, 13, L2)
    gone = [int(exp[0][0][0]), int(exp[0][0][4]), 999999]
    c.delete_items(gone)
    res = c.batch_search(q, 10)
    assert [int(x) for x in res[0].ids()] == [x for x in exp[0][0].tolist() if x not in gone][:10]
    c.restore_items(gone)
    # pending rows are merged; rows committed after the build stay outside the index
    c.add_items(np.repeat(q[:1], 3, axis=0), [5000, 5001, 5002])
    assert {5000, 5001, 5002} <= set(int(x) for x in c.batch_search(q[:1], 5)[0].ids())
    c.commit()
    assert not ({5000, 5001, 5002} & set(int(x) for x in c.batch_search(q[:1], 5)[0].ids()))
    assert c._flat.polarvec_params(arrays=False)["n"] == 3000
    # at most one auxiliary index: PolarVec -> PQ -> PolarVec -> exact
    c.build_index("FLAT-L2-PQ8")
    assert c._flat.polarvec_params(arrays=False)["padded_dim"] == 0 and c._flat.pq_params(arrays=False)["M"] == 8
    assert c.search_profile(q[0], 10)["profile"]["index_path"] == "pq_two_pass"
    c.build_index("FLAT-IP-POLARVEC3")
    p = c._flat.polarvec_params(arrays=False)
    assert c._flat.pq_params(arrays=False)["M"] == 0 and (p["n"], p["bits"], p["flags"]) == (3003, 3, 0)
    assert c.search_profile(q[0], 10)["profile"]["index_path"] == "polarvec_two_pass"
    c.build_index("FLAT-IP")
    assert c._flat.polarvec_params(arrays=False)["padded_dim"] == 0
    assert c.search_profile(q[0], 10)["profile"]["index_path"] == "flat_mmap"
    # PQ and RaBitQ come before PolarVec in a name that carries two tokens (engine.rs:4559-4600)
    c.build_index("FLAT-IP-RABITQ-POLARVEC4")
    assert c._flat.polarvec_params(arrays=False)["padded_dim"] == 0 and c._flat.rabitq_params(arrays=False)["n"] == 3003
    # nothing is built over 0 rows
    e = L.Collection("empty", 32, device=0)
    e.build_index("FLAT-L2-POLARVEC4")
    assert e._flat.polarvec_params(arrays=False)["padded_dim"] == 0 and len(e.batch_search(q, 5)[0].ids()) == 0


def test_collection_reopens_from_disk(L, ref, tmp_path):
    rng = np.random.default_rng(4)
    data = rng.standard_normal((2500, 48)).astype(f32)
    c = _collection(L, data, path=tmp_path)
    c.build_index("FLAT-COS-POLARVEC4")
    assert (tmp_path / "polarvec_index.bin").exists()
    enc = PC.ref_encode(ref[0], data, 4, COS)
    q = rng.standard_normal((4, 48)).astype(f32)
    again = _collection(L, data, path=tmp_path)             # the rows come back first, then the auxiliary index
    assert not again.try_load_polarvec("FLAT-COS")          # the stored mode does not name PolarVec
    assert not again.try_load_polarvec("FLAT-COS-POLARVEC3")   # ... or names another width than the file's
    assert again.try_load_polarvec("FLAT-COS-POLARVEC4")
    check_index(again._flat.polarvec_params(), enc, 48)
    _check_collection(again, ref, data, enc, q, 10, COS)
    assert again.search_profile(q[0], 10)["profile"]["index_path"] == "polarvec_two_pass"
    fewer = _collection(L, data[:100], path=tmp_path)       # a file that covers more rows than are there is not installed
    assert not fewer.try_load_polarvec("FLAT-COS-POLARVEC4")
    c.build_index("FLAT-COS-RABITQ")                        # building another mode removes the file
    assert not (tmp_path / "polarvec_index.bin").exists() and (tmp_path / "rabitq_index.bin").exists()
    assert not _collection(L, data, path=tmp_path).try_load_polarvec("FLAT-COS-POLARVEC4")


def test_collection_mutations_equal_a_fresh_collection(L, ref, tmp_path):
    """After update_items, upsert_items and compact the index is rebuilt (and saved again): every search equals the search of a fresh
    collection that was given the final rows, which in turn equals the restatement over those rows."""
    rng = np.random.default_rng(6)
    dim = 32
    data = rng.standard_normal((3000, dim)).astype(f32)
    q = rng.standard_normal((5, dim)).astype(f32)
    c = _collection(L, data, path=tmp_path)
    c.build_index("FLAT-L2-POLARVEC4")
    ids = list(range(3000))

    def check():
        fresh = _collection(L, data, ids=ids)
        fresh.build_index("FLAT-L2-POLARVEC4")
        enc = PC.ref_encode(ref[0], data, 4, L2)
        check_index(c._flat.polarvec_params(), enc, dim)
        _check_collection(c, ref, data, enc, q, 10, L2, ids)
        for a, b in zip(c.batch_search(q, 10), fresh.batch_search(q, 10)):
            assert list(a.ids()) == list(b.ids()) and np.array_equal(np.asarray(a.distances(), f32), np.asarray(b.distances(), f32))
        from lynsedb_amd.storage import load_polarvec_index

        assert np.array_equal(load_polarvec_index(tmp_path / "polarvec_index.bin").codes, enc.codes)

    data[[7, 1500]] = q[:2] * f32(3.0)     # values beyond the old grid: the fit moves
    c.update_items(data[[7, 1500]], [7, 1500])
    check()
    new = rng.standard_normal((2, dim)).astype(f32)
    data[40] = new[0]
    data = np.concatenate([data, new[1:]])
    ids.append(9000)
    c.upsert_items(new, [40, 9000])
    check()
    c.delete_items([0, 40, 2999])
    assert c.compact() == 3
    keep = np.ones(len(ids), bool)
    keep[[0, 40, 2999]] = False
    data, ids = np.ascontiguousarray(data[keep]), [i for i, k_ in zip(ids, keep) if k_]
    check()
