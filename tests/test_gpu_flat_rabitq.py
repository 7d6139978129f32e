"""GPU parity tests for FLAT-{IP,L2,COS}-RABITQ (RaBitQIndex, src/storage/rabitq_mmap.rs; Collection, src/engine.rs:4476, :4552,
:5504-5526) through the C ABI and the Collection, against a restatement: the SmallRng sign words in Python, encode / query transform /
binary score in tests/rabitq_ref/rabitq_ref.c, every exact distance from the oracle's exported single-pair kernel, both canonical
(score, row) cuts in numpy.  Codes, sign words, norm bits, result ids and f32 distance bits are compared; there are no tolerances.
(A NaN norm is compared as NaN: neither IEEE 754 nor Rust pins a NaN's sign and payload.)"""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import oracle as O
from conftest import oracle_for_every_query

pytestmark = pytest.mark.gpu
IP, L2, COS = O.IP, O.L2, O.COS
NAME = {IP: "ip", L2: "l2", COS: "cosine"}
f32 = np.float32
HERE = Path(__file__).resolve().parent
_vp = C.c_void_p
M64 = (1 << 64) - 1
OVERSAMPLE = 200


@pytest.fixture(scope="module")
def L():
    import lynsedb_amd as L_

    assert L_._lib.device_count() >= 1
    return L_


@pytest.fixture(scope="module")
def ref(tmp_path_factory, oracle):
    cc = next((c for c in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang") if shutil.which(c)), None)
    assert cc, "no C compiler for tests/rabitq_ref/rabitq_ref.c"
    so = tmp_path_factory.mktemp("rabitq_ref") / "librabitq_ref.so"
    subprocess.run([cc, "-O2", "-shared", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-o", str(so),
                    str(HERE / "rabitq_ref" / "rabitq_ref.c"), "-lm"], check=True)
    lib = C.CDLL(str(so))
    lib.rbr_encode.argtypes = [_vp, C.c_size_t, C.c_size_t, _vp, C.c_size_t, _vp, _vp]
    lib.rbr_query.argtypes = [_vp, C.c_size_t, _vp, C.c_size_t, _vp, _vp]
    lib.rbr_scores.argtypes = [_vp, _vp, C.c_size_t, C.c_size_t, _vp, C.c_float, C.c_int, _vp]
    lib.rbr_dists.argtypes = [_vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_int, _vp, _vp]
    for fn in (lib.rbr_encode, lib.rbr_query, lib.rbr_scores, lib.rbr_dists):
        fn.restype = None
    return lib, C.cast(oracle.lib.lo_compute_distance, _vp)


def _p(a):
    return a.ctypes.data_as(_vp)


# ------------------------------------------------------------------------------------- restatement ----
def sign_words(count, seed=42):
    """the first `count` next_u64() of SmallRng::seed_from_u64(seed): xoshiro256++ whose state is four SplitMix64 outputs"""
    s, st = [], seed
    for _ in range(4):
        st = (st + 0x9E3779B97F4A7C15) & M64
        z = st
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        s.append(z ^ (z >> 31))
    rotl = lambda x, k: ((x << k) | (x >> (64 - k))) & M64
    out = []
    for _ in range(count):
        out.append((rotl((s[0] + s[3]) & M64, 23) + s[0]) & M64)
        t = (s[1] << 17) & M64
        s[2] ^= s[0]; s[3] ^= s[1]; s[1] ^= s[2]; s[0] ^= s[3]; s[2] ^= t
        s[3] = rotl(s[3], 45)
    return np.array(out, np.uint64)


def pow2(dim):
    return 1 << max(dim - 1, 0).bit_length()


def ref_encode(ref, data, signs=None):
    lib, _ = ref
    n, dim = data.shape
    P = pow2(dim)
    signs = sign_words((P + 63) // 64) if signs is None else signs
    codes = np.zeros((n, (P + 7) // 8), np.uint8)
    norms = np.zeros(n, f32)
    lib.rbr_encode(_p(np.ascontiguousarray(data)), n, dim, _p(signs), signs.size, _p(codes), _p(norms))
    return signs, codes, norms


def _cut(scores, asc, N, rows):
    """positions of the N best by the canonical (score, row) key: NaN ranks last (as +-inf), -0 == +0.  A partition first keeps
    every key up to the N-th smallest (ties at the cut included), so the lexsort that decides them sees all of them."""
    s = np.where(np.isnan(scores), np.inf if asc else -np.inf, scores).astype(f32) + f32(0.0)
    key = s if asc else -s
    cand = np.arange(key.size)
    if 0 < N < key.size:
        cand = np.nonzero(key <= np.partition(key, N - 1)[N - 1])[0]
    order = cand[np.lexsort((rows[cand], key[cand]))]
    return order[:N], s


def ref_search(ref, data, signs, codes, norms, queries, k, metric, oversample=OVERSAMPLE, pools=None):
    """per query (rows, exact distances); `pools`, a list, receives each query's pool"""
    lib, dist = ref
    n_rbq, dim = codes.shape[0], data.shape[1]
    cb = codes.shape[1]
    asc = metric != IP
    kk = min(k, n_rbq)
    N = min(kk * oversample, n_rbq)
    data = np.ascontiguousarray(data)

    def one(qi):
        q = np.ascontiguousarray(queries[qi])
        lut, total = np.zeros((cb, 256), f32), np.zeros(1, f32)
        lib.rbr_query(_p(q), dim, _p(signs), signs.size, _p(lut), _p(total))
        sc = np.zeros(n_rbq, f32)
        lib.rbr_scores(_p(codes), _p(norms), n_rbq, dim, _p(lut), C.c_float(float(total[0])), 1 if asc else 0, _p(sc))
        pool, _ = _cut(sc, asc, N, np.arange(n_rbq))
        pool = np.ascontiguousarray(pool, np.uint64)
        d = np.zeros(pool.size, f32)
        lib.rbr_dists(_p(q), _p(data), dim, _p(pool), pool.size, metric, dist, _p(d))
        sel, s = _cut(d, asc, kk, pool)
        return pool[sel].astype(np.uint64), s[sel], pool

    res = oracle_for_every_query(one, queries.shape[0])
    if pools is not None:
        pools.extend(r[2] for r in res)
    return [(r[0], r[1]) for r in res]


def check_search(got, exp):
    rows, dists, counts = got
    assert counts.shape[0] == len(exp)
    for qi, (e_r, e_d) in enumerate(exp):
        c = int(counts[qi])
        assert c == e_r.size, (qi, c, e_r.size)
        assert np.array_equal(rows[qi, :c], e_r), (qi, rows[qi, :c][:10], e_r[:10])
        assert np.array_equal(dists[qi, :c].view(np.uint32), e_d.view(np.uint32)), (qi, dists[qi, :c][:10], e_d[:10])


def norm_bits(a):
    """f32 bits with every NaN mapped to one pattern"""
    return np.where(np.isnan(a), f32(np.nan), a).astype(f32).view(np.uint32)


def check_index(p, signs, codes, norms):
    assert np.array_equal(p["sign_words"], signs)
    assert np.array_equal(p["codes"], codes)
    assert np.array_equal(np.isnan(p["norms"]), np.isnan(norms))
    assert np.array_equal(norm_bits(p["norms"]), norm_bits(norms))


def make_index(L, data):
    idx = L.FlatIndex(None, data.shape[1], device=0)
    idx.write(data)
    return idx


def built(L, ref, data):
    """index + the restatement's (signs, codes, norms), checked equal to the device's"""
    idx = make_index(L, data)
    idx.build_rabitq()
    p = idx.rabitq_params()
    dim = data.shape[1]
    assert (p["dim"], p["padded_dim"], p["code_bytes"], p["n"]) == (dim, pow2(dim), (pow2(dim) + 7) // 8, data.shape[0])
    enc = ref_encode(ref, data)
    check_index(p, *enc)
    return idx, enc


# ------------------------------------------------------------------------------------------- tests ----
@pytest.mark.parametrize("dim", [1, 2, 3, 5, 8, 16, 20, 33, 64, 100, 128, 300, 768, 1536, 5000])
def test_codes_norms_and_sign_words_bit_equal(L, ref, dim):
    """padded_dim 1, 2, 4, 8, 16, 32 (a wave's ballot holds 64 ... 2 whole codes; code_bytes = 1 with unused high bits up to 4),
    64 and 128 (one and two ballots per row), 512, 1024, 2048 (8, 4, 2 rows per block) and 8192 (one row per block).  1003 rows: the
    last block and the last 64-row tile are partial."""
    rng = np.random.default_rng(dim)
    n = 1003 if dim <= 1536 else 67
    data = rng.standard_normal((n, dim)).astype(f32)
    data[5] = 0.0                      # an all-zero row: every rotated value +0.0, every bit set, norm 0
    data[6] = -0.0
    data[7, : max(1, dim // 2)] = 1e-20   # squares in the denormal range
    built(L, ref, data)


@pytest.mark.parametrize("metric", [IP, L2, COS])
@pytest.mark.parametrize("dim", [1, 3, 5, 100, 128, 300, 768, 1536])
def test_search_parity(L, ref, metric, dim):
    """Every query of every batch.  code_bytes 1 (padded 1, 4, 8), 16 (one 16-byte column group, one LDS chunk), 64 (four groups:
    one chunk of 64 bytes at nq < 4, four of 16 from four queries on), 128 and 256 (two and four chunks, 8 and 16).  k = 1, 10 cut
    the pool by the radix selection (N = 200, 2000), k = 100 pools every row.  nq = 3: single-query blocks; 7 and 256: groups of
    four, 7 ending in a partial one."""
    rng = np.random.default_rng(dim * 10 + metric)
    n = 3000 if dim <= 128 else 2100
    data = rng.standard_normal((n, dim)).astype(f32)
    idx, enc = built(L, ref, data)
    for nq in (1, 3, 7, 256):
        queries = rng.standard_normal((nq, dim)).astype(f32)
        queries[0] = data[11]
        for k in (1, 10, 100):
            exp = ref_search(ref, data, *enc, queries, k, metric)
            check_search(idx.search_rabitq_batch_arrays(queries, k, NAME[metric]), exp)


def test_pool_beyond_the_device_selection_and_pool_of_all_rows(L, ref):
    """n = 21,000.  k = 100: N = 20,000 > 16,384 keys, cut by the radix selection, scored on the device and selected on the host.
    k = 105: k * 200 = n, the pool is every row.  k = 30,000 > n: k' = n."""
    rng = np.random.default_rng(21)
    n, dim = 21_000, 100
    data = rng.standard_normal((n, dim)).astype(f32)
    idx, enc = built(L, ref, data)
    queries = rng.standard_normal((3, dim)).astype(f32)
    for metric in (IP, L2, COS):
        for k in (100, 105):
            assert min(k * OVERSAMPLE, n) == (20_000 if k == 100 else n)
            exp = ref_search(ref, data, *enc, queries, k, metric)
            check_search(idx.search_rabitq_batch_arrays(queries, k, NAME[metric]), exp)
    exp = ref_search(ref, data, *enc, queries[:1], 30_000, L2)
    got = idx.search_rabitq_batch_arrays(queries[:1], 30_000, "l2")
    assert int(got[2][0]) == n
    check_search(got, exp)


def test_query_chunks_of_223_at_600k_rows(L, ref):
    """n_rbq = 600,000: the [chunk][n_rbq] score matrix caps a query chunk at floor(512 MiB / 4 n_rbq) = 223 queries, which is no
    multiple of the scan's groups of four; 230 queries run as 223 + 7.  One metric (IP: the descending key)."""
    rng = np.random.default_rng(600)
    n, dim = 600_000, 16
    assert (512 << 20) // (4 * n) == 223
    data = rng.standard_normal((n, dim)).astype(f32)
    idx, enc = built(L, ref, data)
    queries = rng.standard_normal((230, dim)).astype(f32)
    queries[0] = data[599_999]
    exp = ref_search(ref, data, *enc, queries, 10, IP)
    check_search(idx.search_rabitq_batch_arrays(queries, 10, "ip"), exp)


def test_query_chunks_of_256(L, ref):
    """The search driver (coded_search, csrc/coded_host.inc) takes at most QCHUNK = 256 queries at a time: 257 run as 256 + 1, the last
    chunk a single-query block.  k = 1: N = 200 < 300 rows, so both chunks go through the radix selection."""
    rng = np.random.default_rng(257)
    data = rng.standard_normal((300, 20)).astype(f32)
    idx, enc = built(L, ref, data)
    queries = rng.standard_normal((257, 20)).astype(f32)
    queries[256] = data[11]
    assert min(1 * OVERSAMPLE, 300) == 200
    for metric in (IP, L2, COS):
        exp = ref_search(ref, data, *enc, queries, 1, metric)
        check_search(idx.search_rabitq_batch_arrays(queries, 1, NAME[metric]), exp)


def test_query_chunks_at_the_table_cap(L, ref):
    """dim 9,000 -> padded 16,384, 2,048 code bytes: one query's byte tables are 2,048 * 256 floats = 2 MiB, and a chunk's tables stay
    at or under 256 MiB, so a chunk is 128 queries, fewer than QCHUNK; 130 run as 128 + 2.  The smallest padded width at which the cap
    binds."""
    rng = np.random.default_rng(9000)
    dim = 9000
    table_bytes = (pow2(dim) + 7) // 8 * 256 * 4
    assert pow2(dim) == 16_384 and (256 << 20) // table_bytes == 128 < 256
    data = rng.standard_normal((300, dim)).astype(f32)
    idx, enc = built(L, ref, data)
    queries = rng.standard_normal((130, dim)).astype(f32)
    queries[129] = data[11]
    for metric in (IP, L2):
        exp = ref_search(ref, data, *enc, queries, 1, metric)
        check_search(idx.search_rabitq_batch_arrays(queries, 1, NAME[metric]), exp)


def test_widest_padded_dim_and_the_lds_refusal(L, ref):
    """dim 20,000 -> padded 32,768: 128 KiB of LDS in the rotation kernels (the raised limit), 4,096 code bytes in 256 chunks of 16
    (five queries: a group of four and a partial one) and in 64 chunks of 64 (one query).  dim 33,000 -> padded 65,536 floats do
    not fit the 160 KiB: refused."""
    from lynsedb_amd._lib import LynseUnsupportedError

    rng = np.random.default_rng(20)
    data = rng.standard_normal((70, 20_000)).astype(f32)
    idx, enc = built(L, ref, data)
    queries = rng.standard_normal((5, 20_000)).astype(f32)
    for metric in (IP, L2):
        exp = ref_search(ref, data, *enc, queries, 3, metric)
        check_search(idx.search_rabitq_batch_arrays(queries, 3, NAME[metric]), exp)
        check_search(idx.search_rabitq_batch_arrays(queries[:1], 3, NAME[metric]), exp[:1])
    wide = make_index(L, rng.standard_normal((3, 33_000)).astype(f32))
    with pytest.raises(LynseUnsupportedError):
        wide.build_rabitq()


@pytest.mark.parametrize("dim", [5, 100])
def test_all_zero_query_duplicates_and_constant_rows(L, ref, dim):
    rng = np.random.default_rng(50 + dim)
    base = rng.standard_normal((50, dim)).astype(f32)
    data = np.concatenate([np.repeat(base, 40, axis=0), np.full((300, dim), 0.25, f32), np.zeros((200, dim), f32)])   # 2,500 rows
    idx, enc = built(L, ref, data)
    queries = np.stack([np.zeros(dim, f32), base[3], rng.standard_normal(dim).astype(f32), np.full(dim, -0.0, f32)])
    for metric in (IP, L2, COS):
        for k in (1, 10, 100):
            pools = []
            exp = ref_search(ref, data, *enc, queries, k, metric, pools=pools)
            got = idx.search_rabitq_batch_arrays(queries, k, NAME[metric])
            check_search(got, exp)
            # the all-zero query: total_q and every table entry are 0, every row scores the same (IP: +-0; L2: norm^2 differs,
            # so only IP ties everywhere) -> the IP pool is rows 0 .. N-1
            if metric == IP:
                N = min(k * OVERSAMPLE, data.shape[0])
                assert np.array_equal(np.sort(pools[0]), np.arange(N))
                assert int(got[0][0].max()) < N


def test_non_finite_rows_and_queries(L, ref):
    rng = np.random.default_rng(77)
    dim = 20
    data = rng.standard_normal((2500, dim)).astype(f32)
    data[3] = np.nan
    data[50, 7] = np.nan
    data[90, 0] = np.inf
    data[91, 19] = -np.inf
    data[92, 3], data[92, 4] = np.inf, -np.inf
    data[93] = np.inf
    data[94] = 3e38                                   # the norm's sum overflows to +inf
    idx, enc = built(L, ref, data)
    queries = rng.standard_normal((6, dim)).astype(f32)
    queries[1] = np.nan
    queries[2, 5] = np.nan
    queries[3, 0] = np.inf
    queries[4] = -np.inf
    queries[5] = 3e38
    for metric in (IP, L2, COS):
        for k in (1, 10, 100):
            exp = ref_search(ref, data, *enc, queries, k, metric)
            check_search(idx.search_rabitq_batch_arrays(queries, k, NAME[metric]), exp)


def test_file_round_trip_and_appends(L, ref, tmp_path):
    from lynsedb_amd.storage import RabitqIndexFile, load_rabitq_index, save_rabitq_index

    rng = np.random.default_rng(9)
    dim = 100
    data = rng.standard_normal((3000, dim)).astype(f32)
    a, enc = built(L, ref, data)
    p = a.rabitq_params()
    save_rabitq_index(tmp_path / "rabitq_index.bin", RabitqIndexFile(dim, p["padded_dim"], p["sign_words"], p["codes"], p["norms"]))
    f = load_rabitq_index(tmp_path / "rabitq_index.bin")
    b = make_index(L, data)
    b.load_rabitq(f.sign_words, f.codes, f.norms)
    check_index(b.rabitq_params(), *enc)
    queries = rng.standard_normal((9, dim)).astype(f32)
    for metric in (IP, L2, COS):
        exp = ref_search(ref, data, *enc, queries, 10, metric)
        check_search(a.search_rabitq_batch_arrays(queries, 10, NAME[metric]), exp)
        check_search(b.search_rabitq_batch_arrays(queries, 10, NAME[metric]), exp)
    # an index over fewer rows than the handle holds, with sign words of its own (one word where two are needed: the second
    # negates nothing)
    own = np.array([0xDEADBEEF12345678], np.uint64)
    enc2 = ref_encode(ref, data[:1000], own)
    b.load_rabitq(*enc2)
    p2 = b.rabitq_params()
    assert p2["n"] == 1000 and p2["sign_words"].tolist() == [0xDEADBEEF12345678, 0]
    assert np.array_equal(p2["codes"], enc2[1])
    exp = ref_search(ref, data, *enc2, queries, 10, IP)
    check_search(b.search_rabitq_batch_arrays(queries, 10, "ip"), exp)
    # rows appended after the build stay outside the index
    a.write(rng.standard_normal((500, dim)).astype(f32))
    assert a.rabitq_params(arrays=False)["n"] == 3000
    rows, _, counts = a.search_rabitq_batch_arrays(queries, 3000, "l2")
    assert int(counts.min()) == 3000 and int(rows[:, :3000].max()) < 3000
    exp = ref_search(ref, data, *enc, queries, 10, L2)
    check_search(a.search_rabitq_batch_arrays(queries, 10, "l2"), exp)
    a.drop_rabitq()
    assert a.rabitq_params()["padded_dim"] == 0
    with pytest.raises(ValueError, match="no RaBitQ index"):
        a.search_rabitq_batch_arrays(queries, 10, "l2")


def test_refusals(L):
    from lynsedb_amd._lib import LynseUnsupportedError

    rng = np.random.default_rng(1)
    data = rng.random((100, 64)).astype(f32)
    idx = make_index(L, data)
    idx.build_rabitq()
    with pytest.raises(LynseUnsupportedError):
        idx.search_rabitq_batch_arrays(data[:2], 5, "hamming")
    rows, dists, counts = idx.search_rabitq_batch_arrays(data[:2], 0, "ip")
    assert rows.shape == (2, 0) and counts.tolist() == [0, 0]
    h16 = L.FlatIndex(None, 64, device=0, dtype="f16")
    h16.write(data)
    with pytest.raises(LynseUnsupportedError):
        h16.build_rabitq()
    empty = L.FlatIndex(None, 64, device=0)
    with pytest.raises(ValueError, match="at least one vector"):
        empty.build_rabitq()
    p = idx.rabitq_params()
    with pytest.raises(ValueError):
        idx.load_rabitq(p["sign_words"], p["codes"][:, :4], p["norms"])          # code_bytes of another dim
    big = np.zeros((101, 8), np.uint8)
    with pytest.raises(ValueError, match="more rows than the handle holds"):
        idx.load_rabitq(p["sign_words"], big, np.zeros(101, f32))
    for mode in ("FLAT-HAMMING-RABITQ", "FLAT-IP-POLARVEC"):
        c = L.Collection("c", 64, device=0)
        c.add_items(data, list(range(100)))
        c.commit()
        with pytest.raises(NotImplementedError):
            c.build_index(mode)


def _collection(L, data, path=None):
    c = L.Collection("rbq", data.shape[1], device=0, path=path)
    c.add_items(data, list(range(data.shape[0])))
    c.commit()
    return c


def _check_collection(c, ref, data, enc, q, k, metric):
    exp = ref_search(ref, data, *enc, q, k, metric)
    res = c.batch_search(q, k)
    for r, (e_r, e_d) in zip(res, exp):
        assert np.array_equal(np.asarray(r.ids(), np.uint64), e_r)
        assert np.array_equal(np.asarray(r.distances(), f32).view(np.uint32), e_d.view(np.uint32))


@pytest.mark.parametrize("mode,metric", [("FLAT-IP-RABITQ", IP), ("FLAT-L2-RABITQ", L2), ("FLAT-COS-RABITQ", COS),
                                         ("FLAT-COSINE-RABITQ", COS)])
def test_collection_modes(L, ref, mode, metric):
    rng = np.random.default_rng(len(mode))
    data = rng.standard_normal((4000, 64)).astype(f32)
    c = _collection(L, data)
    c.build_index(mode)
    enc = ref_encode(ref, data)
    check_index(c._flat.rabitq_params(), *enc)
    q = rng.standard_normal((3, 64)).astype(f32)
    _check_collection(c, ref, data, enc, q, 10, metric)
    prof = c.search_profile(q[0], 10)["profile"]
    assert prof["index_path"] == "rabitq_two_pass"
    assert prof["rerank_us"] >= 0
    assert prof["device"]["rabitq_stages"]["scan_us"] > 0 and prof["device"]["rabitq_stages"]["rescore_us"] > 0


def test_collection_subset_pending_tombstones_and_rebuild(L, ref, oracle):
    rng = np.random.default_rng(3)
    data = rng.standard_normal((3000, 32)).astype(f32)
    c = _collection(L, data)
    c.build_index("FLAT-L2-RABITQ")
    enc = ref_encode(ref, data)
    q = data[:2] + f32(0.01)
    # subset=: the exact filtered scan, never RaBitQ candidates (engine.rs:4784-4791)
    res = c.batch_search(q, 10, subset=np.arange(0, 3000, 2, dtype=np.uint64))
    for qi, r in enumerate(res):
        ids = np.asarray(r.ids())
        assert ids.size == 10 and np.all(ids % 2 == 0)
        e_ids, _ = oracle.canonical_topk(q[qi], data[::2], 10, L2)
        assert np.array_equal(ids, 2 * e_ids.astype(np.int64))
    assert c.search_profile(q[0], 10, subset=np.arange(10, dtype=np.uint64))["profile"]["index_path"] == "flat_mmap_filtered"
    # tombstones: search_k = k + |tombstones| goes into the RaBitQ search, the deleted ids are filtered afterwards
    exp = ref_search(ref, data, *enc, q, 13, L2)
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
    assert c._flat.rabitq_params(arrays=False)["n"] == 3000
    # at most one auxiliary index: RaBitQ -> PQ -> RaBitQ -> exact
    c.build_index("FLAT-L2-PQ8")
    assert c._flat.rabitq_params(arrays=False)["padded_dim"] == 0 and c._flat.pq_params(arrays=False)["M"] == 8
    assert c.search_profile(q[0], 10)["profile"]["index_path"] == "pq_two_pass"
    c.build_index("FLAT-IP-RABITQ")
    assert c._flat.pq_params(arrays=False)["M"] == 0 and c._flat.rabitq_params(arrays=False)["n"] == 3003
    assert c.search_profile(q[0], 10)["profile"]["index_path"] == "rabitq_two_pass"
    c.build_index("FLAT-IP")
    assert c._flat.rabitq_params(arrays=False)["padded_dim"] == 0
    assert c.search_profile(q[0], 10)["profile"]["index_path"] == "flat_mmap"
    # nothing is built over 0 rows
    e = L.Collection("empty", 32, device=0)
    e.build_index("FLAT-L2-RABITQ")
    assert e._flat.rabitq_params(arrays=False)["padded_dim"] == 0 and len(e.batch_search(q, 5)[0].ids()) == 0


def test_collection_reopens_from_disk(L, ref, tmp_path):
    rng = np.random.default_rng(4)
    data = rng.standard_normal((2500, 48)).astype(f32)
    c = _collection(L, data, path=tmp_path)
    c.build_index("FLAT-COS-RABITQ")
    assert (tmp_path / "rabitq_index.bin").exists()
    enc = ref_encode(ref, data)
    q = rng.standard_normal((4, 48)).astype(f32)
    again = _collection(L, data, path=tmp_path)          # the rows come back first, then the auxiliary index
    assert not again.try_load_rabitq("FLAT-COS")         # the stored mode does not name RaBitQ
    assert again.try_load_rabitq("FLAT-COS-RABITQ")
    check_index(again._flat.rabitq_params(), *enc)
    _check_collection(again, ref, data, enc, q, 10, COS)
    assert again.search_profile(q[0], 10)["profile"]["index_path"] == "rabitq_two_pass"
    fewer = _collection(L, data[:100], path=tmp_path)    # a file that covers more rows than are there is not installed
    assert not fewer.try_load_rabitq("FLAT-COS-RABITQ")
    c.build_index("FLAT-COS")                            # building another mode removes the file
    assert not (tmp_path / "rabitq_index.bin").exists()
    assert not _collection(L, data, path=tmp_path).try_load_rabitq("FLAT-COS-RABITQ")


def test_stage_times(L):
    rng = np.random.default_rng(2)
    data = rng.standard_normal((5000, 32)).astype(f32)
    idx = make_index(L, data)
    idx.build_rabitq()
    idx.profile_enable(True)
    idx.rabitq_stage_times(reset=True)
    idx.search_rabitq_batch_arrays(data[:4], 10, "ip")
    t = idx.rabitq_stage_times(reset=True)
    idx.profile_enable(False)
    assert t["searches"] == 1 and t["scan_us"] > 0 and t["rescore_us"] > 0
    assert idx.rabitq_stage_times()["searches"] == 0
