"""GPU parity tests for FLAT-{IP,L2,COS}-PQ (PQIndex, src/storage/pq_mmap.rs; Collection, src/engine.rs:4559-4600, :5504-5526)
through the C ABI and the Collection, against a restatement: the SmallRng draws in Python, kmeans_subspace / encode_vectors /
build_lut in tests/pq_ref/pq_ref.c (control flow only), every distance from the oracle's exported single-pair kernels, the ADC sums
and both canonical (score, row) cuts in numpy.  Ids and f32 distance bits are compared."""
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


@pytest.fixture(scope="module")
def L():
    import lynsedb_amd as L_

    assert L_._lib.device_count() >= 1
    return L_


@pytest.fixture(scope="module")
def ref(tmp_path_factory, oracle):
    cc = next((c for c in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang") if shutil.which(c)), None)
    assert cc, "no C compiler for tests/pq_ref/pq_ref.c"
    so = tmp_path_factory.mktemp("pq_ref") / "libpq_ref.so"
    subprocess.run([cc, "-O2", "-shared", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-o", str(so), str(HERE / "pq_ref" / "pq_ref.c")],
                   check=True)
    lib = C.CDLL(str(so))
    lib.pqr_train.argtypes = [_vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, _vp, _vp, _vp, _vp]
    lib.pqr_encode.argtypes = [_vp, C.c_size_t, _vp, C.c_size_t, C.c_size_t, C.c_size_t, _vp, _vp, _vp]
    lib.pqr_lut.argtypes = [_vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, _vp, _vp, _vp]
    lib.pqr_dists.argtypes = [_vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_int, _vp, _vp]
    olib = oracle.lib
    fp = {name: C.cast(getattr(olib, name), _vp) for name in ("lo_l2_single", "lo_ip_single", "lo_compute_distance")}
    return lib, fp


def _p(a):
    return a.ctypes.data_as(_vp)


# ------------------------------------------------------------------------------------- restatement ----
M64 = (1 << 64) - 1


def splitmix_stream(seed, count):
    out, st = [], seed
    for _ in range(count):
        st = (st + 0x9E3779B97F4A7C15) & M64
        z = st
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        out.append(z ^ (z >> 31))
    return out


class Xoshiro:
    def __init__(self, s):
        self.s = list(s)

    @staticmethod
    def seed_from_u64(seed):
        s = splitmix_stream(seed, 4)
        return Xoshiro(s) if any(s) else Xoshiro.seed_from_u64(0)

    def next(self):
        s = self.s
        rotl = lambda x, k: ((x << k) | (x >> (64 - k))) & M64
        res = (rotl((s[0] + s[3]) & M64, 23) + s[0]) & M64
        t = (s[1] << 17) & M64
        s[2] ^= s[0]; s[3] ^= s[1]; s[1] ^= s[2]; s[0] ^= s[3]; s[2] ^= t
        s[3] = rotl(s[3], 45)
        return res

    def below(self, n):
        zone = ((n << (64 - n.bit_length())) & M64) - 1
        while True:
            p = self.next() * n
            if (p & M64) <= zone:
                return p >> 64


def init_indices(seed, n, k):
    rng, chosen, out, attempts = Xoshiro.seed_from_u64(seed), set(), [], 0
    while len(out) < k and attempts < k * 10:
        i = rng.below(n)
        if i not in chosen:
            chosen.add(i)
            out.append(i)
        attempts += 1
    return out


def ref_build(ref, data, M, n_clusters=256, code_rows=None):
    lib, fp = ref
    n, dim = data.shape
    K = min(max(n_clusters, 1), 256, n)
    train_n = min(n, 50000)
    if train_n < n:
        s = max(n // train_n, 1)
        train = np.ascontiguousarray(data[::s][:train_n])
    else:
        train = data
    idx = np.zeros((M, K), np.uint32)
    chosen = np.zeros(M, np.uint32)
    for m in range(M):
        d = init_indices(m, train.shape[0], K)
        idx[m, :len(d)] = d
        chosen[m] = len(d)
    cb = np.zeros((M, K, dim // M), f32)
    lib.pqr_train(_p(train), train.shape[0], dim, M, K, 6 if K <= 64 else 15, _p(idx), _p(chosen), fp["lo_l2_single"], _p(cb))
    rows = np.arange(n, dtype=np.uint64) if code_rows is None else np.ascontiguousarray(code_rows, np.uint64)
    codes = np.zeros((rows.size, M), np.uint8)
    lib.pqr_encode(_p(data), dim, _p(rows), rows.size, M, K, _p(cb), fp["lo_l2_single"], _p(codes))
    return cb, codes


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


def ref_search(ref, data, cb, codes, queries, k, metric, oversample=32):
    lib, fp = ref
    M, K, ss = cb.shape
    n_pq, dim = codes.shape[0], data.shape[1]
    lut = np.zeros((queries.shape[0], M, K), f32)
    lib.pqr_lut(_p(queries), queries.shape[0], dim, M, K, _p(cb), fp["lo_ip_single" if metric == IP else "lo_l2_single"], _p(lut))
    asc = metric != IP
    kk = min(k, n_pq)
    N = min(kk * oversample, n_pq)
    by_m = np.ascontiguousarray(codes.T)

    def one(qi):
        acc = np.zeros(n_pq, f32)
        for m in range(M):
            acc = (acc + lut[qi, m, by_m[m]]).astype(f32)
        pool, _ = _cut(acc, asc, N, np.arange(n_pq))
        pool = np.ascontiguousarray(pool, np.uint64)
        d = np.zeros(pool.size, f32)
        lib.pqr_dists(_p(np.ascontiguousarray(queries[qi])), _p(data), dim, _p(pool), pool.size, metric, fp["lo_compute_distance"], _p(d))
        sel, s = _cut(d, asc, kk, pool)
        return pool[sel].astype(np.uint64), s[sel]

    return oracle_for_every_query(one, queries.shape[0])


def check_search(got, exp):
    rows, dists, counts = got
    assert counts.shape[0] == len(exp)
    for qi, (e_r, e_d) in enumerate(exp):
        c = int(counts[qi])
        assert c == e_r.size, (qi, c, e_r.size)
        assert np.array_equal(rows[qi, :c], e_r), (qi, rows[qi, :c][:10], e_r[:10])
        assert np.array_equal(dists[qi, :c].view(np.uint32), e_d.view(np.uint32)), (qi, dists[qi, :c][:10], e_d[:10])


def make_index(L, data):
    idx = L.FlatIndex(None, data.shape[1], device=0)
    idx.write(data)
    return idx


def loaded_pq(L, rng, n, dim, M, K):
    """n random rows with random codebooks [M][K][dim / M] and codes < K installed through load_pq: search cases without a
    training restatement"""
    data = rng.standard_normal((n, dim)).astype(f32)
    cb = rng.standard_normal((M, K, dim // M)).astype(f32)
    codes = rng.integers(0, K, (n, M), dtype=np.uint8)
    idx = make_index(L, data)
    idx.load_pq(cb, codes)
    return idx, data, cb, codes


# ------------------------------------------------------------------------------------------- tests ----
@pytest.mark.parametrize("n,dim,M,ncl", [(2000, 32, 8, 256), (50, 16, 4, 256), (300, 24, 6, 1), (1000, 36, 12, 64),
                                         (1000, 384, 16, 256), (1000, 768, 16, 256), (1000, 1536, 16, 256), (1000, 300, 4, 256),
                                         (1000, 768, 4, 256)])
def test_codebooks_and_codes_bit_equal(L, ref, n, dim, M, ncl):
    """The sub-vector width ss = dim / M picks k_pq_assign's instance and the codebook's home (LDS when K ss 4 <= 64 KiB):
    ss <= 16 below; 24 -> <32> (24 KiB in LDS), 48 -> <64> (48 KiB in LDS), 96 -> <128> (96 KiB: global memory), 75 -> <128>
    (75 KiB: global memory; nine 8-chunks, the odd one and a tail of 3), 192 -> <0> (sub-vector read from memory).  ss = 75, 96 and
    192 also take k_pq_update / k_pq_empty past one 64-column pass."""
    rng = np.random.default_rng(n + dim)
    data = rng.standard_normal((n, dim)).astype(f32)
    idx = make_index(L, data)
    idx.build_pq(M, ncl)
    p = idx.pq_params()
    cb, codes = ref_build(ref, data, M, ncl)
    assert (p["M"], p["K"], p["ss"], p["n"]) == (M, cb.shape[1], dim // M, n)
    assert np.array_equal(p["codebooks"].view(np.uint32), cb.view(np.uint32))
    assert np.array_equal(p["codes"], codes)


def test_training_edge_cases(L, ref):
    rng = np.random.default_rng(7)
    # stops at the first assignment: K = number of distinct points, every row on its own seed
    base = rng.standard_normal((4, 8)).astype(f32)
    cases = [np.repeat(base, 25, axis=0),                                     # duplicate-heavy: perturbation fill, empty clusters
             np.concatenate([np.zeros((60, 8), f32), rng.standard_normal((4, 8)).astype(f32) * 100]),   # big cluster + outliers
             np.tile(rng.standard_normal((1, 8)).astype(f32), (40, 1))]       # a single distinct row
    nan_rows = rng.standard_normal((200, 16)).astype(f32)
    nan_rows[[3, 50, 77]] = np.nan
    nan_rows[90, 5] = np.nan
    cases.append(nan_rows)
    for data in cases:
        for M, ncl in ((2, 256), (4, 16), (1, 3)):
            if data.shape[1] % M:
                continue
            idx = make_index(L, data)
            idx.build_pq(M, ncl)
            p = idx.pq_params()
            cb, codes = ref_build(ref, data, M, ncl)
            assert np.array_equal(p["codebooks"].view(np.uint32), cb.view(np.uint32)), (data.shape, M, ncl)
            assert np.array_equal(p["codes"], codes), (data.shape, M, ncl)


def test_stride_sample_120k(L, ref):
    rng = np.random.default_rng(120)
    data = rng.standard_normal((120000, 16)).astype(f32)
    idx = make_index(L, data)
    idx.build_pq(4, 256)
    p = idx.pq_params()
    sample = np.sort(rng.choice(120000, 3000, replace=False)).astype(np.uint64)
    cb, codes = ref_build(ref, data, 4, 256, code_rows=sample)
    assert np.array_equal(p["codebooks"].view(np.uint32), cb.view(np.uint32))
    assert np.array_equal(p["codes"][sample.astype(np.int64)], codes)


@pytest.mark.parametrize("metric", [IP, L2, COS])
@pytest.mark.parametrize("dim,M", [pytest.param(32, 8, id="8"), pytest.param(32, 16, id="16"), pytest.param(32, 32, id="32"),
                                   pytest.param(384, 16, id="384x16"), pytest.param(768, 16, id="768x16"),
                                   pytest.param(1536, 16, id="1536x16"), pytest.param(300, 4, id="300x4"),
                                   pytest.param(768, 4, id="768x4")])
def test_search_parity(L, ref, metric, dim, M):
    """Every query of every batch.  The tables' sub-vector width ss = dim / M picks the path through pq_pair in k_pq_lut: 4, 2, 1
    (one 8-chunk or the tail only), 24 (one 16-wide two-accumulator step and the odd 8-chunk), 48 (three steps), 96 (six),
    75 (four steps, the odd 8-chunk and a tail of 3) and 192 (twelve steps).  k = 1, 10 cut the pool by the radix selection,
    k = 100 pools every row."""
    rng = np.random.default_rng(M * 10 + metric + (0 if dim == 32 else dim))
    n = 3000 if dim == 32 else 1500
    data = rng.standard_normal((n, dim)).astype(f32)
    idx = make_index(L, data)
    idx.build_pq(M, 256)
    p = idx.pq_params()
    cb, codes = p["codebooks"], p["codes"]
    for nq in (1, 7, 256):
        queries = rng.standard_normal((nq, dim)).astype(f32)
        queries[0] = data[11]
        for k in (1, 10, 100):
            exp = ref_search(ref, data, cb, codes, queries, k, metric)
            check_search(idx.search_pq_batch_arrays(queries, k, NAME[metric]), exp)


def test_search_odd_dim_large_pool_and_k(L, ref):
    rng = np.random.default_rng(36)
    n, dim = 20000, 36
    data = rng.standard_normal((n, dim)).astype(f32)
    idx = make_index(L, data)
    idx.build_pq(12, 256)
    p = idx.pq_params()
    queries = rng.standard_normal((3, dim)).astype(f32)
    for metric in (IP, L2, COS):
        for k in (600, 10000):          # N = 19,200 (> 16,384: the host-selected pool) and N = n_pq
            exp = ref_search(ref, data, p["codebooks"], p["codes"], queries, k, metric)
            check_search(idx.search_pq_batch_arrays(queries, k, NAME[metric]), exp)
    # 300 queries at k = 600: two query chunks (256 + 44), the host selection's buffers reused by the second one
    many = rng.standard_normal((300, dim)).astype(f32)
    exp = ref_search(ref, data, p["codebooks"], p["codes"], many, 600, L2)
    check_search(idx.search_pq_batch_arrays(many, 600, "l2"), exp)


@pytest.mark.parametrize("dim,M,K,nqs", [pytest.param(768, 96, 256, (1, 3, 7), id="M96"),
                                         pytest.param(768, 768, 256, (1, 5), id="PQ768"),
                                         pytest.param(64, 32, 150, (1, 4, 9), id="K150")])
def test_adc_table_chunks(L, ref, dim, M, K, nqs):
    """k_pq_adc when the tables of a query group exceed 64 KiB: mc = min(M, 16384 / (qb K)) subspaces per LDS chunk, qb = 4 from
    four queries on, else 1.  M = 96: six chunks at qb = 4, two (64 + 32) at qb = 1.  PQ768 (ss = 1): 48 chunks at qb = 4, 12 at
    qb = 1.  K = 150, M = 32: mc = 27 at qb = 4, so the byte path (mc % 4 != 0) with a ragged last chunk of 5; one chunk of 32 on
    the word path at qb = 1.  nq = 7, 5, 9 end in a partial group of four."""
    rng = np.random.default_rng(M + K)
    idx, data, cb, codes = loaded_pq(L, rng, 4000, dim, M, K)
    for nq in nqs:
        queries = rng.standard_normal((nq, dim)).astype(f32)
        queries[0] = data[7]
        for metric in (IP, L2, COS):
            exp = ref_search(ref, data, cb, codes, queries, 10, metric)
            check_search(idx.search_pq_batch_arrays(queries, 10, NAME[metric]), exp)


def test_query_chunks_of_256(L, ref):
    """nq = 601: query chunks of 256 / 256 / 89 (QCHUNK), the last ending in a partial group of four; every query checked."""
    rng = np.random.default_rng(601)
    n, dim = 3000, 32
    data = rng.standard_normal((n, dim)).astype(f32)
    idx = make_index(L, data)
    idx.build_pq(8, 256)
    p = idx.pq_params()
    queries = rng.standard_normal((601, dim)).astype(f32)
    for metric in (IP, L2, COS):
        exp = ref_search(ref, data, p["codebooks"], p["codes"], queries, 10, metric)
        check_search(idx.search_pq_batch_arrays(queries, 10, NAME[metric]), exp)


def test_query_chunks_of_223_at_600k_rows(L, ref):
    """n_pq = 600,000: the [chunk][n_pq] score matrix caps a query chunk at floor(512 MiB / 4 n_pq) = 223 queries, which is no
    multiple of the ADC's groups of four; 230 queries run as 223 + 7.  One metric (IP: the descending key) keeps the restatement's
    600,000-row ADC sums to a few seconds."""
    rng = np.random.default_rng(600)
    n = 600_000
    assert (512 << 20) // (4 * n) == 223
    idx, data, cb, codes = loaded_pq(L, rng, n, 16, 4, 256)
    queries = rng.standard_normal((230, 16)).astype(f32)
    queries[0] = data[599_999]
    exp = ref_search(ref, data, cb, codes, queries, 10, IP)
    check_search(idx.search_pq_batch_arrays(queries, 10, "ip"), exp)


def test_rescore_at_768_on_both_sides_of_the_lds_limit(L, ref):
    """D = 768 (a 3 KiB query in LDS beside the keys).  k = 512: a pool of N = 16,384 keys, sorted in LDS (128 KiB + 3 KiB of
    160 KiB).  k = 513: N = 16,416 > 16,384, scored on the device and selected on the host.  n = 17,000 keeps N < n, so both pools
    come from the radix selection."""
    rng = np.random.default_rng(768)
    n = 17_000
    idx, data, cb, codes = loaded_pq(L, rng, n, 768, 16, 256)
    queries = rng.standard_normal((3, 768)).astype(f32)
    queries[0] = data[5]
    for k, N in ((512, 16_384), (513, 16_416)):
        assert min(k * 32, n) == N
        for metric in (IP, L2, COS):
            exp = ref_search(ref, data, cb, codes, queries, k, metric)
            got = idx.search_pq_batch_arrays(queries, k, NAME[metric])
            assert (got[2] == k).all()
            check_search(got, exp)


def test_ties_and_nan_query(L, ref):
    rng = np.random.default_rng(5)
    base = rng.standard_normal((50, 16)).astype(f32)
    data = np.repeat(base, 40, axis=0)           # 2,000 rows, 40 copies each: ADC and exact ties everywhere
    idx = make_index(L, data)
    idx.build_pq(4, 256)
    p = idx.pq_params()
    queries = np.stack([base[3], rng.standard_normal(16).astype(f32), np.full(16, np.nan, f32)])
    for metric in (IP, L2, COS):
        for k in (1, 10, 100):
            exp = ref_search(ref, data, p["codebooks"], p["codes"], queries, k, metric)
            check_search(idx.search_pq_batch_arrays(queries, k, NAME[metric]), exp)


def test_load_round_trip_and_appends(L, ref, tmp_path):
    from lynsedb_amd.storage import PqIndexFile, load_pq_index, save_pq_index

    rng = np.random.default_rng(9)
    data = rng.standard_normal((3000, 32)).astype(f32)
    a = make_index(L, data)
    a.build_pq(8, 256)
    p = a.pq_params()
    save_pq_index(tmp_path / "pq_index.bin", PqIndexFile(8, p["K"], 4, 32, p["codebooks"], p["codes"]))
    f = load_pq_index(tmp_path / "pq_index.bin")
    b = make_index(L, data)
    b.load_pq(f.codebooks, f.codes)
    queries = rng.standard_normal((9, 32)).astype(f32)
    for metric in ("ip", "l2", "cosine"):
        ra, rb = a.search_pq_batch_arrays(queries, 10, metric), b.search_pq_batch_arrays(queries, 10, metric)
        for x, y in zip(ra, rb):
            assert np.array_equal(x, y)
    # rows appended after the build stay outside the index
    b.write(rng.standard_normal((500, 32)).astype(f32))
    assert b.pq_params(arrays=False)["n"] == 3000
    rows, _, counts = b.search_pq_batch_arrays(queries, 3000, "l2")
    assert int(counts.min()) == 3000 and int(rows[:, :3000].max()) < 3000


def test_refusals(L):
    from lynsedb_amd._lib import LynseUnsupportedError

    rng = np.random.default_rng(1)
    data = rng.random((100, 64)).astype(f32)
    idx = make_index(L, data)
    idx.build_pq(8, 16)
    with pytest.raises(LynseUnsupportedError):
        idx.search_pq_batch_arrays(data[:2], 5, "hamming")
    h16 = L.FlatIndex(None, 64, device=0, dtype="f16")
    h16.write(data)
    with pytest.raises(LynseUnsupportedError):
        h16.build_pq(8, 16)
    with pytest.raises(ValueError):
        idx.build_pq(7, 16)
    bad = idx.pq_params()
    codes = bad["codes"].copy()
    codes[0, 0] = 200
    with pytest.raises(ValueError, match="out-of-range code"):
        idx.load_pq(bad["codebooks"], codes)
    for mode in ("FLAT-HAMMING-PQ", "IVF-IP-PQ", "IVF-L2-PQ8"):
        c = L.Collection("c", 64, device=0)
        c.add_items(data, list(range(100)))
        c.commit()
        with pytest.raises(NotImplementedError):
            c.build_index(mode)


def _collection(L, data, ids=None):
    c = L.Collection("pq", data.shape[1], device=0)
    c.add_items(data, list(range(data.shape[0])) if ids is None else ids)
    c.commit()
    return c


@pytest.mark.parametrize("mode,metric,M", [("FLAT-IP-PQ", IP, 16), ("FLAT-L2-PQ", L2, 16), ("FLAT-COS-PQ8", COS, 8),
                                           ("FLAT-COSINE-PQ", COS, 16)])
def test_collection_modes(L, ref, mode, metric, M):
    rng = np.random.default_rng(len(mode))
    data = rng.standard_normal((4000, 64)).astype(f32)
    c = _collection(L, data)
    c.build_index(mode)
    p = c._flat.pq_params()
    assert p["M"] == M
    q = rng.standard_normal((3, 64)).astype(f32)
    exp = ref_search(ref, data, p["codebooks"], p["codes"], q, 10, metric)
    res = c.batch_search(q, 10)
    for r, (e_r, e_d) in zip(res, exp):
        assert np.array_equal(np.asarray(r.ids(), np.uint64), e_r)
        assert np.array_equal(np.asarray(r.distances(), f32).view(np.uint32), e_d.view(np.uint32))
    prof = c.search_profile(q[0], 10)["profile"]
    assert prof["index_path"] == "pq_two_pass"
    assert prof["rerank_us"] >= 0


def test_collection_subset_pending_tombstones_and_rebuild(L, ref, oracle):
    rng = np.random.default_rng(3)
    data = rng.standard_normal((3000, 32)).astype(f32)
    c = _collection(L, data)
    c.build_index("FLAT-L2-PQ8")
    p = c._flat.pq_params()
    q = data[:2] + f32(0.01)
    # subset=: the exact filtered scan, never PQ candidates (engine.rs:9600-9633)
    even = np.arange(0, 3000, 2, dtype=np.uint64)
    res = c.batch_search(q, 10, subset=even)
    for qi, r in enumerate(res):
        ids = np.asarray(r.ids())
        assert ids.size == 10 and np.all(ids % 2 == 0)
        e_ids, e_d = oracle.canonical_topk(q[qi], data[::2], 10, L2)
        assert np.array_equal(ids, 2 * e_ids.astype(np.int64))
    # tombstones: search_k = k + |tombstones| goes into the PQ search, the deleted ids are filtered afterwards
    exp = ref_search(ref, data, p["codebooks"], p["codes"], q, 13, L2)
    c.delete_items([int(exp[0][0][0]), int(exp[0][0][4]), 999999])
    res = c.batch_search(q, 10)
    keep = [x for x in exp[0][0].tolist() if x not in (int(exp[0][0][0]), int(exp[0][0][4]))][:10]
    assert [int(x) for x in res[0].ids()] == keep
    c.restore_items([int(exp[0][0][0]), int(exp[0][0][4]), 999999])
    # pending rows are merged; rows committed after the build stay outside the index
    extra = np.repeat(q[:1], 3, axis=0)
    c.add_items(extra, [5000, 5001, 5002])
    r = c.batch_search(q[:1], 5)[0]
    assert {5000, 5001, 5002} <= set(int(x) for x in r.ids())
    c.commit()
    r = c.batch_search(q[:1], 5)[0]
    assert not ({5000, 5001, 5002} & set(int(x) for x in r.ids()))
    # rebuilding to FLAT-IP drops PQ: exact search again
    c.build_index("FLAT-IP")
    assert c._flat.pq_params(arrays=False)["M"] == 0
    assert c.search_profile(q[0], 10)["profile"]["index_path"] == "flat_mmap"


def test_stage_times(L):
    rng = np.random.default_rng(2)
    data = rng.standard_normal((5000, 32)).astype(f32)
    idx = make_index(L, data)
    idx.build_pq(8, 256)
    idx.profile_enable(True)
    idx.pq_stage_times(reset=True)
    idx.search_pq_batch_arrays(data[:4], 10, "ip")
    t = idx.pq_stage_times(reset=True)
    idx.profile_enable(False)
    assert t["searches"] == 1 and t["scan_us"] > 0 and t["rescore_us"] > 0
