"""Sparse vectors without a GPU: the restatement the GPU tests compare against (tests/sparse_ref/sparse_ref.c) checked on its own, the
host-only normaliser of the C ABI, the Python normaliser, the jsonl store file and the entry points' argument checks.  No GPU."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import sparse_common as sc
from sparse_common import Csr, f32, u32, u64

HERE = Path(__file__).resolve().parent
INVALID, DEVICE = 1, 6
_vp = C.c_void_p


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return sc.build_ref(tmp_path_factory.mktemp("sparse_ref"))


@pytest.fixture(scope="module")
def L():
    import lynsedb_amd as L_

    return L_


def lib_normalize(L, csr):
    from lynsedb_amd.core import sparse_normalize_arrays

    return Csr(*sparse_normalize_arrays(*csr.arrays()))


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def test_restatement_gives_the_reference_known_answer(ref):
    """engine.rs:9432-9458: three rows, query {2: 1} -> rows 1, 2 with 2.0, 0.5; query {5: 1} -> rows 1, 0 with 1.0, 0.5 (the reference
    asserts the second query under a filter only: the unfiltered order follows from the scoring rule)."""
    rows = Csr.of([{1: 1.0, 5: 0.5}, {2: 2.0, 5: 1.0}, {2: 0.5, 7: 1.0}])
    for q, e_rows, e_scores in [({2: 1.0}, [1, 2], [2.0, 0.5]), ({5: 1.0}, [1, 0], [1.0, 0.5])]:
        s = ref.scores(Csr.of([q]), rows)[0]
        order = sc.order_of(s)
        assert list(order) == e_rows and list(s[order]) == e_scores


def test_restatement_against_float64(ref):
    rng = np.random.default_rng(5)
    rows = sc.gen_vectors(rng, 400, 200, 1, 80)
    queries = sc.gen_vectors(rng, 6, 200, 30, 30)
    got = ref.scores(queries, rows)
    for qi in range(len(queries)):
        q = dict(zip(*[x.tolist() for x in queries.row(qi)]))
        for r in range(len(rows)):
            ri, rv = rows.row(r)
            terms = [np.float64(q[i]) * np.float64(v) for i, v in zip(ri.tolist(), rv.tolist()) if i in q]
            exact = float(np.sum(terms)) if terms else 0.0
            # n terms summed in f32: |error| <= (n + 1) * 2^-24 * sum |term| (one rounding per multiply and per add, first order)
            bound = (len(terms) + 1) * 2.0 ** -23 * float(np.sum(np.abs(terms))) if terms else 0.0
            assert abs(float(got[qi, r]) - exact) <= bound, (qi, r, got[qi, r], exact, bound)
            if not terms:
                assert got[qi, r] == 0 and not np.signbit(got[qi, r])


def test_restatement_reversed_order_differs(ref):
    """the order probe itself: on config A a fifth of the pairs, at the very least, change bits when summed the other way round"""
    rng = np.random.default_rng(1)
    rows = sc.gen_vectors(rng, 3000, 200, 1, 80)
    queries = sc.gen_vectors(rng, 4, 200, 30, 30)
    a, b = ref.scores(queries, rows), ref.scores(queries, rows, reversed_=True)
    assert np.mean(a.view(u32) != b.view(u32)) >= 0.2
    assert np.allclose(a, b, rtol=1e-3, atol=1e-3)


# ---- lynse_hip_sparse_normalize ------------------------------------------------------------------------------------------------------
NORMALIZE_CASES = [
    # duplicates whose sum depends on the order: (1e8 + 1) - 1e8 = 0 in f32, (1e8 - 1e8) + 1 = 1
    ([3, 3, 3], [1e8, 1.0, -1e8]),
    ([3, 3, 3], [1e8, -1e8, 1.0]),
    ([3, 9, 3, 9, 3], [0.1, 0.2, 0.3, 0.7, 0.6]),
    ([4, 4], [2.5, -2.5]),                       # cancels to zero: dropped
    ([4, 1, 4, 7], [2.5, 1.0, -2.5, 0.0]),
    ([5, 2, 9], [0.0, -0.0, 3.0]),               # zeros skipped
    ([9, 2, 5, 0], [1.0, 2.0, 3.0, 4.0]),        # unsorted
    ([], []),
    ([0, 0xFFFFFFFF, 0, 0xFFFFFFFF], [1.0, 2.0, 0.5, -0.25]),
    ([6], [1e-45]),                               # a subnormal is finite and non-zero
]


def test_lib_normalize_equals_the_restatement(L, ref):
    for idx, val in NORMALIZE_CASES:
        e_i, e_v = ref.normalize(idx, val)
        got = lib_normalize(L, Csr.of([(idx, val)]))
        assert np.array_equal(got.indices, e_i) and np.array_equal(got.values.view(u32), e_v.view(u32)), (idx, val, got.indices, got.values)
        assert np.all(np.diff(got.indices.astype(np.int64)) > 0) and np.all(got.values != 0)
    assert ref.normalize([3, 3, 3], [1e8, 1.0, -1e8])[1].size == 0 and list(ref.normalize([3, 3, 3], [1e8, -1e8, 1.0])[1]) == [1.0]
    # the whole list as one batch, and random vectors with many duplicates
    batch = lib_normalize(L, Csr.of(NORMALIZE_CASES))
    for r, (idx, val) in enumerate(NORMALIZE_CASES):
        e_i, e_v = ref.normalize(idx, val)
        g_i, g_v = batch.row(r)
        assert np.array_equal(g_i, e_i) and np.array_equal(g_v.view(u32), e_v.view(u32))
    rng = np.random.default_rng(2)
    vecs = [(rng.integers(0, 12, m).astype(u32), sc.gen_values(rng, m) * (rng.random(m) > 0.1)) for m in rng.integers(0, 60, 50)]
    batch = lib_normalize(L, Csr.of(vecs))
    for r, (idx, val) in enumerate(vecs):
        e_i, e_v = ref.normalize(idx, val)
        g_i, g_v = batch.row(r)
        assert np.array_equal(g_i, e_i) and np.array_equal(g_v.view(u32), e_v.view(u32))


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_lib_normalize_refuses_non_finite_values(L, ref, bad):
    assert ref.normalize([1, 2], [1.0, bad]) is None
    with pytest.raises(ValueError, match="sparse vector values must be finite"):
        lib_normalize(L, Csr.of([([1], [1.0]), ([1, 2], [1.0, bad])]))
    with pytest.raises(ValueError, match="sparse vector values must be finite"):
        lib_normalize(L, Csr.of([([2, 2], [bad, 0.0])]))


# ---- normalize_sparse_vector (python/lynse/_backend.py:31-43) ------------------------------------------------------------------------
def test_normalize_sparse_vector(L):
    assert L.normalize_sparse_vector({3: 1, 1: 0.5}) == [(3, 1.0), (1, 0.5)]
    assert L.normalize_sparse_vector([(7, 2), [0xFFFFFFFF, 0.1]]) == [(7, 2.0), (0xFFFFFFFF, float(f32(0.1)))]
    assert L.normalize_sparse_vector(np.array([[2, 1.5]])) == [(2, 1.5)]
    with pytest.raises(ValueError, match=re.escape("sparse vector entries must be (index, value) pairs")):
        L.normalize_sparse_vector([(1, 2.0, 3.0)])
    with pytest.raises(ValueError, match=re.escape("sparse vector entries must be (index, value) pairs")):
        L.normalize_sparse_vector([(1,)])
    with pytest.raises(ValueError, match="sparse vector indices must be non-negative"):
        L.normalize_sparse_vector({-1: 1.0})
    with pytest.raises(OverflowError):
        L.normalize_sparse_vector({1 << 32: 1.0})


# ---- sparse_vectors.jsonl ------------------------------------------------------------------------------------------------------------
def test_jsonl_round_trip(L, tmp_path):
    from lynsedb_amd.storage import load_sparse_vectors, save_sparse_vectors

    rng = np.random.default_rng(3)
    store = {42: (np.array([0, 5, 0xFFFFFFFF], u32), np.array([1e-45, 1e-30, 3e38], f32)),
             7: (np.array([1, 2, 3, 4], u32), np.array([-1e-40, -0.1, -3e38, 1.0], f32)),
             (1 << 63) + 5: (np.array([9], u32), np.array([16777216.0], f32))}
    for i in range(100, 130):
        idx = np.sort(rng.choice(1000, 20, replace=False)).astype(u32)
        store[i] = (idx, sc.gen_values(rng, 20))
    p = tmp_path / "sub" / "sparse_vectors.jsonl"
    save_sparse_vectors(p, store)
    lines = p.read_text().splitlines()
    assert len(lines) == len(store) and [int(re.match(r'\{"id":(\d+),', l).group(1)) for l in lines] == sorted(store)
    assert lines[0] == '{"id":7,"indices":[1,2,3,4],"values":[-1e-40,-0.1,-3e38,1.0]}'
    assert not list(p.parent.glob("*.tmp"))
    back = load_sparse_vectors(p)
    assert sorted(back) == sorted(store)
    for i, (idx, val) in store.items():
        assert np.array_equal(back[i][0], idx) and np.array_equal(back[i][1].view(u32), val.view(u32)), i
    save_sparse_vectors(p, {})   # rewritten whole
    assert p.read_text() == "" and load_sparse_vectors(p) == {}
    assert load_sparse_vectors(tmp_path / "missing.jsonl") == {}


def test_jsonl_fixture(L, golden_dir):
    from lynsedb_amd.storage import load_sparse_vectors

    got = load_sparse_vectors(golden_dir / "sparse_vectors_fixture.jsonl")
    want = {3: ([4], [3.5]),                                       # a duplicate index summed, an explicit zero skipped
            7: ([1, 6], [0.25, 4.0]),                              # the later line wins; its indices were out of order
            11: ([0, 100, 0xFFFFFFFF], [-3.25, 1e20, 1e-10]),      # exponent forms
            5: ([2], [150.0])}                                     # cancelled to empty (removed), then set again; 12 was removed last
    assert sorted(got) == sorted(want)
    for i, (idx, val) in want.items():
        assert np.array_equal(got[i][0], np.array(idx, u32)) and np.array_equal(got[i][1].view(u32), np.array(val, f32).view(u32)), i


def test_jsonl_length_mismatch_and_garbage(L, tmp_path):
    from lynsedb_amd.storage import StorageError, load_sparse_vectors

    p = tmp_path / "sparse_vectors.jsonl"
    p.write_text('{"id":1,"indices":[1],"values":[1.0]}\n{"id":9,"indices":[1,2,3],"values":[1.0,2.0]}\n')
    with pytest.raises(StorageError, match="sparse vector record for id 9 has 3 indices but 2 values"):
        load_sparse_vectors(p)
    p.write_text('{"id":1,"indices":[1],"values":[1.0]}\nnot json\n')
    with pytest.raises(StorageError, match="failed to parse sparse vector record at line 2"):
        load_sparse_vectors(p)
    for bad_id in ("1.5", '"7"', "true", "-3", "18446744073709551616"):   # serde's u64 refuses these
        p.write_text('{"id":%s,"indices":[1],"values":[1.0]}\n' % bad_id)
        with pytest.raises(StorageError, match="failed to parse sparse vector record at line 1"):
            load_sparse_vectors(p)
    p.write_text('{"id":1,"indices":[1],"values":[1e39]}\n')
    with pytest.raises(StorageError, match="sparse vector values must be finite"):
        load_sparse_vectors(p)


# ---- the C ABI's argument checks -----------------------------------------------------------------------------------------------------
def test_null_handle_is_an_invalid_argument(L):
    lib = L._lib.lib
    z = np.zeros(4, u64)
    p = L._lib.Profile()
    assert lib.lynse_hip_sparse_set_rows(None, sc._p(z), sc._p(z), sc._p(z), 0) == INVALID
    assert lib.lynse_hip_sparse_len(None, None, None) == INVALID
    assert lib.lynse_hip_sparse_search(None, sc._p(z), sc._p(z), sc._p(z), 1, 1, None, 0, sc._p(z), sc._p(z), sc._p(z), None) == INVALID
    assert lib.lynse_hip_sparse_profile_enable(None, 1) == INVALID
    assert lib.lynse_hip_sparse_profile_get(None, C.byref(p), 0) == INVALID
    assert lib.lynse_hip_sparse_create(0, None) == INVALID
    assert lib.lynse_hip_sparse_hbm_bytes(None) == 0
    assert lib.lynse_hip_sparse_destroy(None) == 0
    assert lib.lynse_hip_sparse_len(None, None, None) == INVALID and L._lib.last_error() == "handle is NULL"


def test_create_without_a_device_is_a_device_error(L):
    if L._lib.device_count() >= 1:
        pytest.skip("a HIP device is present")
    h = _vp()
    assert L._lib.lib.lynse_hip_sparse_create(0, C.byref(h)) == DEVICE and not h
    with pytest.raises(L._lib.LynseHipError):
        L.SparseIndex(device=0)


def test_sparse_scan_kernel_has_no_scratch():
    import lynsedb_amd

    rep = Path(lynsedb_amd.__file__).parent / "csrc" / "resource_usage.txt"
    assert rep.exists(), "the build writes csrc/resource_usage.txt"
    blocks = re.findall(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", rep.read_text(), flags=re.S)
    mine = [(n, int(s)) for n, s in blocks if "k_sparse_scan" in n]
    assert mine and all(s == 0 for _, s in mine), mine
