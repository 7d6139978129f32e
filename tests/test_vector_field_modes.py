"""Named vector fields without a device: the three resolvers against the reference's rules and messages
(engine.rs:2017-2091), the dtype aliases, and the remap model of tests/vector_fields_common.py against hand-written cases."""
import pytest

import vector_fields_common as V


@pytest.fixture(scope="module")
def VF():
    from lynsedb_amd import vector_fields

    return vector_fields


def invalid(msg):
    return "^" + __import__("re").escape("Invalid argument: " + msg) + "$"


def test_field_names(VF):
    assert VF.validate_vector_field_name(" img ") == "img"
    assert VF.validate_vector_field_name("Title_emb-2") == "Title_emb-2"
    assert VF.validate_vector_field_name("a" * 128) == "a" * 128
    for name, msg in (("", "vector field name cannot be empty"),
                      ("   ", "vector field name cannot be empty"),
                      ("default", "'default' is reserved for the primary collection vector"),
                      (" default ", "'default' is reserved for the primary collection vector"),
                      ("a" * 129, "vector field name cannot exceed 128 characters"),
                      ("a b", "vector field name may only contain ASCII letters, digits, '_' and '-'"),
                      ("é", "vector field name may only contain ASCII letters, digits, '_' and '-'"),
                      ("a.b", "vector field name may only contain ASCII letters, digits, '_' and '-'")):
        with pytest.raises(RuntimeError, match=invalid(msg)):
            VF.validate_vector_field_name(name)
    assert VF.validate_vector_field_name("Default") == "Default"   # the reserved name is case-sensitive


def test_metric_resolution(VF):
    from lynsedb_amd import _lib

    r = VF.resolve_named_vector_metric
    assert r(None, None) == _lib.METRIC_IP                              # neither: inner product
    assert r("l2", None) == _lib.METRIC_L2 and r("euclidean", None) == _lib.METRIC_L2
    assert r("cos", None) == _lib.METRIC_COSINE and r("HAMMING", None) == _lib.METRIC_HAMMING
    assert r("manhattan", None) == _lib.METRIC_L1
    assert r(None, "FLAT-L2") == _lib.METRIC_L2 and r(None, "hnsw-cos") == _lib.METRIC_COSINE
    assert r(None, "FLAT-HAMMING-BINARY") == _lib.METRIC_HAMMING and r(None, "FLAT-BRAY-CURTIS") == _lib.METRIC_BRAY_CURTIS
    assert r(None, "FLAT") == _lib.METRIC_IP                            # metric_from_mode_str: no metric token -> inner product
    assert r("l2", "FLAT-L2") == _lib.METRIC_L2 and r("cosine", "HNSW-COS") == _lib.METRIC_COSINE   # agreeing
    with pytest.raises(RuntimeError, match=invalid("vector field metric 'ip' does not match index mode 'FLAT-L2'")):
        r("ip", "FLAT-L2")
    with pytest.raises(RuntimeError, match=invalid("vector field metric 'l2' does not match index mode 'hnsw-cos'")):
        r("l2", "hnsw-cos")
    with pytest.raises(RuntimeError, match=invalid("unsupported vector field metric 'nope'")):
        r("nope", None)
    with pytest.raises(RuntimeError, match=invalid("unsupported vector field metric 'nope'")):
        r("nope", "FLAT-IP")


def test_index_mode_normalisation(VF):
    from lynsedb_amd import _lib

    n = VF.normalize_field_index_mode
    for metric, mode in ((_lib.METRIC_IP, "FLAT-IP"), (_lib.METRIC_L2, "FLAT-L2"), (_lib.METRIC_COSINE, "FLAT-COS"),
                         (_lib.METRIC_HAMMING, "FLAT-HAMMING-BINARY"), (_lib.METRIC_JACCARD, "FLAT-JACCARD-BINARY"),
                         (_lib.METRIC_DICE, "FLAT-DICE-BINARY"), (_lib.METRIC_TANIMOTO, "FLAT-TANIMOTO-BINARY"), (_lib.METRIC_L1, "FLAT-L1"),
                         (_lib.METRIC_CHEBYSHEV, "FLAT-CHEBYSHEV"), (_lib.METRIC_CANBERRA, "FLAT-CANBERRA"),
                         (_lib.METRIC_BRAY_CURTIS, "FLAT-BRAY-CURTIS")):
        assert n(None, metric) == mode and n("", metric) == mode and n("  ", metric) == mode   # the default: the metric's flat mode
    assert n("flat-l2", _lib.METRIC_L2) == "FLAT-L2" and n(" hnsw-cosine ", _lib.METRIC_COSINE) == "HNSW-COSINE"   # lower case, trimmed
    for known in ("FLAT-IP-SQ8", "HNSW-L2-SQ8", "DISKANN-IP", "DISKANN-L2-PQ16", "DISKANN-COS-PQ", "IVF-HAMMING", "IVF-JACCARD-BINARY",
                  "SPANN-COS-SQ8", "FLAT-SORENSEN-DICE-BINARY", "FLAT-MANHATTAN", "HNSW-L1", "HNSW-JS", "FLAT-HAVERSINE-M", "FLAT-LINF"):
        assert n(known, _lib.METRIC_IP) == known
    for unknown in ("FLAT", "NOPE-L2", "FLAT-IP-PQ", "FLAT-L2-RABITQ", "HNSW-HAMMING", "HNSW-CANBERRA", "HNSW-BRAY-CURTIS", "IVF-L1",
                    "DISKANN-COS-PQ8", "FLAT-L1-BINARY", "FLAT-IP-BINARY", "SPANN-HAMMING"):
        with pytest.raises(RuntimeError, match=invalid(f"unknown vector field index mode '{unknown}'")):
            n(unknown, _lib.METRIC_IP)
    with pytest.raises(RuntimeError, match=invalid("unknown vector field index mode 'BOGUS'")):
        n("bogus", _lib.METRIC_IP)                                      # the message carries the upper-cased mode


def test_dtype_aliases(VF):
    d = VF.vector_dtype_name
    assert d(None) == "float32" and d(None, "float16") == "float16"     # the default is the collection's
    for alias in ("float32", "f32", "float", " F32 "):
        assert d(alias) == "float32"
    for alias in ("float16", "f16", "half", "fp16", "HALF"):
        assert d(alias) == "float16"
    with pytest.raises(RuntimeError, match="unsupported vector dtype 'bf16'"):
        d("bf16")


def test_mode_kinds(VF):
    k = VF.field_mode_kind
    for mode in ("FLAT-IP", "FLAT-L2", "FLAT-COS", "FLAT-COSINE", "FLAT-HAMMING", "FLAT-JACCARD-BINARY", "FLAT-TANIMOTO", "FLAT-DICE-BINARY",
                 "FLAT-L1", "FLAT-CHEBYSHEV", "FLAT-CANBERRA", "FLAT-BRAY-CURTIS"):
        assert k(mode) == "flat"
    for mode in ("HNSW-IP", "HNSW-L2", "HNSW-COS", "HNSW-COSINE"):
        assert k(mode) == "hnsw"
    for mode in ("FLAT-IP-SQ8", "HNSW-L2-SQ8", "IVF-L2", "SPANN-IP", "DISKANN-L2", "HNSW-L1", "FLAT-HAVERSINE"):
        with pytest.raises(NotImplementedError):
            k(mode)


# ---- the remap model ------------------------------------------------------------------------------------------------------------
def test_remap_model_by_hand(VF):
    import numpy as np

    N = V.NONE
    assert N == VF.ROWMAP_NONE                                           # the model's sentinel is the library's
    # the library's own packing of rows into BitSet words (what a subset= becomes) is the model's layout: an identity remap of them
    rows = [0, 1, 3, 63, 64, 129]
    packed = VF.words_of_rows(np.array(rows, np.uint64), 130).tolist()
    assert packed == [0b1011 | (1 << 63), 1, 0b10]
    assert V.remap_model(list(range(130)), packed, 130) == (packed, len(rows))
    src = [0b1011]                                                       # rows 0, 1, 3 of 4
    assert V.remap_model([0, 1, 2, 3], src, 4) == ([0b1011], 3)          # identity
    assert V.remap_model([3, 2, 1, 0], src, 4) == ([0b1101], 3)          # reversed
    assert V.remap_model([3, 3, 3], src, 4) == ([0b111], 3)              # every field row on one source row
    assert V.remap_model([2, 2], src, 4) == ([0], 0)
    assert V.remap_model([N, 0, N, 1, N], src, 4) == ([0b01010], 2)      # the sentinel gives 0
    assert V.remap_model([], src, 4) == ([], 0)
    # the tail: collection rows 4 .. 6 are tail bits 0 .. 2
    tail = [0b101]
    assert V.remap_model([4, 5, 6, 0, 2], src, 4, tail, 3) == ([0b01101], 3)
    assert V.remap_model([2, N, 1], [], 0, [0b100], 3) == ([0b001], 1)   # no flushed rows at all: every row is a tail row
    # word edges: 130 field rows over 128 source rows, the bits of source rows 63, 64 and 127 set
    src = [1 << 63, 1 | (1 << 63)]
    row_of = [N] * 130
    row_of[0], row_of[63], row_of[64], row_of[129] = 63, 64, 127, 63
    row_of[1], row_of[65] = 62, 65
    words, count = V.remap_model(row_of, src, 128)
    assert words == [1 | (1 << 63), 1, 0b10] and count == 4
    with pytest.raises(AssertionError):
        V.remap_model([4], [0b1111], 4)                                  # out of range: the host refuses it, the model is not asked


def test_field_search_model_by_hand(VF):
    """the order of the model against the library's notion of it: which metrics rank the smaller distance first"""
    from lynsedb_amd import _lib

    def ascending(metric):
        m = VF.resolve_named_vector_metric(metric, None)
        assert VF.metric_name(m) == metric
        return bool(_lib.lib.lynse_hip_metric_is_ascending(m))

    ids = [10, 11, 12, 13, 14]
    d = [0.5, 0.25, 0.25, 1.0, 0.0]
    assert V.field_search_model(ids, d, None, set(), 3, ascending("l2")) == ([14, 11, 12], [4, 1, 2])        # ties by field row
    assert V.field_search_model(ids, d, None, set(), 3, ascending("ip")) == ([13, 10, 11], [3, 0, 1])        # inner product: larger first
    assert V.field_search_model(ids, d, {11, 13, 99}, {13}, 9, ascending("hamming")) == ([11], [1])          # filter, then tombstones
    assert V.field_search_model(ids, d, set(), set(), 3, ascending("l1")) == ([], [])
