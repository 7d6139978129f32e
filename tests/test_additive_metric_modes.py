"""Host side of the additive metrics (ids 7-10: Manhattan, Chebyshev, Canberra, Bray-Curtis): names, index modes, flags, the host merges,
and the restatement the GPU tests compare against (tests/additive_ref/additive_ref.c) checked on its own.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import lynsedb_amd as L
from additive_common import build_ref
from lynsedb_amd import _lib
from lynsedb_amd.core import ADDITIVE_FLAT_MODES, additive_mode_of
from lynsedb_amd.shard_node import merge_row_results

f32 = np.float32
L1, CHEB, CANB, BRAY = 7, 8, 9, 10
ALIASES = {L1: ["l1", "manhattan", "cityblock", "L1", "Manhattan"],
           CHEB: ["chebyshev", "chebychev", "linf", "l_inf", "l-infinity", "LINF"],
           CANB: ["canberra", "CANBERRA"],
           BRAY: ["bray_curtis", "bray-curtis", "braycurtis", "Bray_Curtis"]}
FLAT_MODES = {"FLAT-L1": L1, "FLAT-MANHATTAN": L1, "FLAT-CITYBLOCK": L1, "FLAT-CHEBYSHEV": CHEB, "FLAT-CHEBYCHEV": CHEB, "FLAT-LINF": CHEB,
              "FLAT-CANBERRA": CANB, "FLAT-BRAY-CURTIS": BRAY, "FLAT-BRAYCURTIS": BRAY}
REFUSED_MODES = ["FLAT-L1-SQ8", "FLAT-L1-PQ8", "FLAT-CANBERRA-BINARY", "IVF-L1", "SPANN-CHEBYSHEV", "FLAT-BRAY-CURTIS-RABITQ", "IVF-LINF-SQ8"]


def test_ids_and_names():
    assert (_lib.METRIC_L1, _lib.METRIC_CHEBYSHEV, _lib.METRIC_CANBERRA, _lib.METRIC_BRAY_CURTIS) == (L1, CHEB, CANB, BRAY)
    assert _lib.lib.lynse_hip_abi_version() == 1
    for m, names in ALIASES.items():
        for name in names:
            assert L.metric_from_str(name) == m, name
    from lynsedb_amd.core import _METRIC_NAMES

    for m in (L1, CHEB, CANB, BRAY):
        assert L.metric_from_str(_METRIC_NAMES[m]) == m


def test_the_six_other_domain_metrics_stay_refused():
    for name in ["haversine", "haversine_m", "geo", "correlation", "pearson", "hellinger", "wasserstein", "wasserstein1d", "emd",
                 "jensen_shannon", "jensen-shannon", "js"]:
        with pytest.raises(NotImplementedError):
            L.metric_from_str(name)
    with pytest.raises(ValueError, match="Unknown metric: bogus"):
        L.metric_from_str("bogus")
    for mode in ["FLAT-JS", "FLAT-JENSEN-SHANNON", "FLAT-JENSENSHANNON", "FLAT-HAVERSINE", "HNSW-CORRELATION", "FLAT-HELLINGER", "FLAT-EMD"]:
        with pytest.raises(NotImplementedError):
            L.metric_from_index_mode(mode)


def test_index_modes_follow_the_chain_order():
    for mode, m in FLAT_MODES.items():
        assert L.metric_from_index_mode(mode) == m
        assert L.metric_from_index_mode(mode.lower()) == m
        assert additive_mode_of(mode) == m and additive_mode_of(mode.lower()) == m
    assert ADDITIVE_FLAT_MODES == FLAT_MODES
    # the chain: Jensen-Shannon first (still refused), then Chebyshev, Canberra, Bray-Curtis, the binary metrics, the refused rest, L1, l2 / cos / ip
    with pytest.raises(NotImplementedError):
        L.metric_from_index_mode("FLAT-JS-CHEBYSHEV")
    assert L.metric_from_index_mode("FLAT-CHEBYSHEV-CANBERRA") == CHEB
    assert L.metric_from_index_mode("FLAT-CANBERRA-BRAY-CURTIS") == CANB
    assert L.metric_from_index_mode("FLAT-BRAYCURTIS-HAMMING") == BRAY
    assert L.metric_from_index_mode("FLAT-HAMMING-L1") == _lib.METRIC_HAMMING
    with pytest.raises(NotImplementedError):
        L.metric_from_index_mode("FLAT-HAVERSINE-L1")
    assert L.metric_from_index_mode("FLAT-L1-L2") == L1
    with pytest.raises(ValueError):   # ("BRAY" alone names nothing)
        L.metric_from_index_mode("FLAT-BRAY")
    for mode in ("FLAT-IP", "FLAT-L2-SQ8", "IVF-COS", "SPANN-L2", "FLAT-HAMMING-BINARY", "FLAT-BOGUS"):
        assert additive_mode_of(mode) is None


@pytest.mark.parametrize("mode", REFUSED_MODES)
def test_other_modes_naming_an_additive_metric_are_unknown_index_types(mode):
    with pytest.raises(ValueError, match="Invalid argument: Unknown index type: "):
        additive_mode_of(mode)
    with pytest.raises(ValueError, match="Invalid argument: Unknown index type: "):
        additive_mode_of(mode.lower())


def test_flags():
    lib = _lib.lib
    for m in (L1, CHEB, CANB, BRAY):
        assert lib.lynse_hip_metric_is_ascending(m) == 1
        assert lib.lynse_hip_metric_is_binary(m) == 0
    assert lib.lynse_hip_metric_is_binary(6) == 1 and lib.lynse_hip_metric_is_binary(3) == 1 and lib.lynse_hip_metric_is_binary(2) == 0
    assert lib.lynse_hip_metric_is_binary(11) == 0


def test_host_merges_treat_them_as_ascending_and_id_11_is_unknown():
    rng = np.random.default_rng(5)
    ids = rng.permutation(400).astype(np.uint64).reshape(8, 50)
    ds = rng.integers(0, 6, size=(8, 50)).astype(f32)
    ds[2, 3] = np.inf
    cnt = rng.integers(0, 51, size=8).astype(np.uint32)
    e_i, e_d = L.merge_topk(ids, ds, cnt, 37, 1)
    li, ld = np.arange(0, 40, 2, dtype=np.uint64), np.sort(rng.integers(0, 9, 20)).astype(f32)
    ri, rd = np.arange(1, 31, 2, dtype=np.uint64), np.sort(rng.integers(0, 9, 15)).astype(f32)
    r_i, r_d = merge_row_results(li, ld, ri, rd, 12, 1)
    for m in (L1, CHEB, CANB, BRAY):
        g_i, g_d = L.merge_topk(ids, ds, cnt, 37, m)
        assert np.array_equal(g_i, e_i) and np.array_equal(g_d.view(np.uint32), e_d.view(np.uint32))
        g_i, g_d = merge_row_results(li, ld, ri, rd, 12, m)
        assert np.array_equal(g_i, r_i) and np.array_equal(g_d.view(np.uint32), r_d.view(np.uint32))
    for name, m in (("manhattan", L1), ("bray-curtis", BRAY)):
        g_i, g_d = L.merge_topk(ids, ds, cnt, 37, name)
        assert np.array_equal(g_i, e_i)
    for bad in (11, -1, 99):
        with pytest.raises(ValueError, match="Unknown metric id"):
            L.merge_topk(ids, ds, cnt, 37, bad)
        with pytest.raises(ValueError, match="Unknown metric id"):
            merge_row_results(li, ld, ri, rd, 12, bad)


def test_entries_without_an_additive_form_refuse_before_they_touch_a_device():
    """The C ABI answers ids 7-10 with LYNSE_ERR_UNSUPPORTED (9), never "Unknown metric id", where the argument check comes before any
    device work: IVF builds, the sharded search, the device merge."""
    lib = _lib.lib
    rows = np.zeros((8, 4), f32)
    out = C.c_void_p()
    p = rows.ctypes.data_as(C.c_void_p)
    for m in (L1, CHEB, CANB, BRAY):
        assert lib.lynse_hip_ivf_build(p, 8, 4, 2, 3, m, 0, 0, C.byref(out)) == 9
        assert "Unknown metric" not in _lib.last_error()
        assert lib.lynse_hip_ivf_build_sq8(p, 8, 4, 2, 3, m, 0, C.byref(out)) == 9
        assert lib.lynse_hip_flat_search_sharded_f32_device(None, None, None, 1, 1, m, None, None, None) == 9
        assert lib.lynse_hip_merge_topk_device(None, 0, 0, 0, 0, 1, 1, 1, m, None, None, None, None) == 9
    assert lib.lynse_hip_merge_topk_device(None, 0, 0, 0, 0, 1, 1, 1, 11, None, None, None, None) == 3   # LYNSE_ERR_UNKNOWN_METRIC


# ---- the restatement itself -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    r = build_ref(tmp_path_factory.mktemp("additive_ref"))
    return lambda m, a, b: float(r.dist(m, a, b))


def test_restatement_known_answers(ref):
    """the reference's own known answers, at 1e-5 absolute"""
    for m, a, b, exp in [(L1, [1, 2, 3], [3, 0, 4], 5.0), (L1, [1, 2], [4, 0], 5.0), (CHEB, [1, 2, 3], [4, 0, 3], 3.0),
                         (CANB, [1, 0, 3], [2, 0, 1], 5 / 6), (BRAY, [1, 2], [2, 4], 1 / 3)]:
        assert abs(ref(m, a, b) - exp) < 1e-5, (m, a, b)


def np64(m, a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    d = np.abs(a - b)
    if m == L1:
        return d.sum()
    if m == CHEB:
        return d.max()
    if m == CANB:
        den = np.abs(a) + np.abs(b)
        return (d[den != 0] / den[den != 0]).sum()
    den = np.abs(a + b).sum()
    return d.sum() / den


@pytest.mark.parametrize("D", [1, 3, 7, 8, 9, 15, 16, 17, 24, 100, 128, 771, 1536])
def test_restatement_against_float64(ref, D):
    """finite data, 1e-5 relative (the project's score contract; an emulation of the 8-lane order stayed within 3.9e-7)"""
    rng = np.random.default_rng(D)
    for kind in range(2):
        a = (rng.standard_normal(D) if kind == 0 else rng.random(D) + 0.01).astype(f32)
        b = (rng.standard_normal(D) if kind == 0 else rng.random(D) + 0.01).astype(f32)
        for m in (L1, CHEB, CANB, BRAY):
            if m == BRAY and kind == 0:
                continue   # (a Gaussian denominator sum cancels: no relative bound)
            e = np64(m, a, b)
            assert abs(ref(m, a, b) - e) <= 1e-5 * abs(e), (m, D, kind)


def test_restatement_special_values(ref):
    nan, inf = np.nan, np.inf
    z = np.zeros(16, f32)
    a = z.copy(); a[0] = nan; a[8] = 2          # a NaN step is erased by the lane's next step
    assert ref(CHEB, a, z) == 2.0
    a = z.copy(); a[1] = 3; a[8] = nan           # a NaN left by a lane's last step is dropped
    assert ref(CHEB, a, z) == 3.0
    assert ref(CHEB, np.array([nan, 1, nan], f32), np.zeros(3, f32)) == 1.0   # the tail: f32::max
    assert ref(CHEB, np.full(8, nan, f32), np.zeros(8, f32)) == 0.0
    assert np.isnan(ref(L1, a, z)) and ref(L1, np.array([inf, 1], f32), np.array([1, 1], f32)) == inf
    assert np.isnan(ref(L1, np.array([inf], f32), np.array([inf], f32)))    # inf - inf
    a = np.ones(8, f32); b = np.ones(8, f32); a[2] = nan
    assert ref(CANB, a, b) == 0.0                # a NaN denominator adds +0 in the body ...
    assert np.isnan(ref(CANB, a[:3], b[:3]))     # ... and NaN in the tail
    assert ref(CANB, np.zeros(11, f32), np.zeros(11, f32)) == 0.0   # 0 / 0 pairs add nothing
    assert ref(CANB, np.array([inf, 1], f32), np.array([1, 1], f32)) != ref(CANB, np.array([inf, 1], f32), np.array([1, 1], f32))   # inf / inf
    assert ref(BRAY, np.zeros(9, f32), np.zeros(9, f32)) == 0.0
    a = np.arange(1, 10, dtype=f32)
    assert ref(BRAY, a, -a) == inf               # a = -b: a zero denominator under a non-zero numerator
    assert ref(BRAY, a, a) == 0.0
