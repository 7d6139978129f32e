"""Multi-vector search without a GPU: the argument checks, the refusals of rule 7 (include/lynse_hip.h, MULTI-VECTOR SEARCH), the
id-added-twice refusal and the mode string — everything that is decided before a device is touched."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

f32 = np.float32
INVALID, UNSUPPORTED = 1, 9


@pytest.fixture()
def coll():
    """a collection that never opened a device: ids 1 .. 5 are known, nothing else of it is touched before the device"""
    import lynsedb_amd as L

    c = L.Collection.__new__(L.Collection)
    c._id_arrays, c._pending_ids, c._tombstone = [np.arange(1, 6, dtype=np.int64)], [], set()
    c._mv_reset()
    return c


def test_mode_string_and_empty_results(coll):
    from lynsedb_amd.core import MULTIVEC_INDEX_MODE

    assert MULTIVEC_INDEX_MODE == "MULTIVEC-MAXSIM-IP"
    q = np.ones((3, 8), f32)
    res = coll.search_multi_vector(q, 5)   # nothing was added: empty, no device
    assert len(res) == 0 and res.index_mode() == "MULTIVEC-MAXSIM-IP" and res._k == 5
    assert coll.search_multi_vector(q)._k == 10   # k=None means 10
    coll.add_multi_vectors([1, 2], [np.ones((4, 8), f32), np.zeros((0, 8), f32)])
    assert coll.multi_vector_len() == 2 and coll._mv_dim == 8
    assert len(coll.search_multi_vector(q, 0)) == 0   # k = 0: no device
    assert [len(r) for r in coll.batch_search_multi_vector([q, q[:1]], 0)] == [0, 0]


def test_query_argument_checks_and_rule_7(coll):
    coll.add_multi_vectors([1], [np.ones((4, 8), f32)])
    with pytest.raises(ValueError, match="2-D"):
        coll.search_multi_vector(np.ones(8, f32), 3)
    with pytest.raises(ValueError, match="at least one token"):
        coll.search_multi_vector(np.ones((0, 8), f32), 3)
    with pytest.raises(RuntimeError, match="Dimension mismatch: expected 8, got 9"):
        coll.search_multi_vector(np.ones((2, 9), f32), 3)
    with pytest.raises(OverflowError):
        coll.search_multi_vector(np.ones((2, 8), f32), -1)
    with pytest.raises(ValueError, match="either as where= or as subset="):
        coll.search_multi_vector(np.ones((2, 8), f32), 0, where="a > 1", subset=[0])
    with pytest.raises(NotImplementedError, match="more than 256 tokens"):
        coll.search_multi_vector(np.ones((257, 8), f32), 3)
    with pytest.raises(NotImplementedError, match="more than 256 tokens"):
        coll.batch_search_multi_vector([np.ones((256, 8), f32), np.ones((300, 8), f32)], 3)


# (dim_mv, Tq) -> (query tiles, waves of a workgroup), or None where 160 KiB of LDS do not hold the tiles and one wave's two blocks:
# each line is one side of a boundary of rule 7
PLAN = [(128, 32, (1, 4)), (128, 33, (2, 2)), (128, 128, (4, 2)), (128, 129, None), (96, 256, (8, 2)), (97, 129, None),
        (192, 128, (4, 1)), (193, 65, None), (288, 64, (2, 1)), (289, 33, None), (416, 32, (1, 1)), (417, 1, None), (1024, 1, None)]


@pytest.mark.parametrize("dim,tq,want", PLAN)
def test_lds_plan_and_its_refusal(coll, dim, tq, want):
    import lynsedb_amd._lib as lb

    tiles, waves, lds = C.c_uint32(0), C.c_uint32(0), C.c_uint64(0)
    rc = lb.lib.lynse_hip_multivec_plan(dim, tq, C.byref(tiles), C.byref(waves), C.byref(lds))
    if want is None:
        assert rc == UNSUPPORTED and "do not fit in LDS" in lb.last_error()
        if dim <= 416:   # the store can exist: the query is what is refused, before a device is touched
            coll.add_multi_vectors([1], [np.ones((2, dim), f32)])
            with pytest.raises(NotImplementedError, match="do not fit in LDS"):
                coll.search_multi_vector(np.ones((tq, dim), f32), 3)
    else:
        assert rc == 0 and (tiles.value, waves.value) == want and lds.value <= 160 * 1024
        assert lb.lib.lynse_hip_multivec_plan(dim, tq, C.byref(tiles), C.byref(waves), None) == 0


def test_add_argument_checks_leave_the_store_unchanged(coll):
    with pytest.raises(NotImplementedError, match="dimension outside 1..1024"):
        coll.add_multi_vectors([1], [np.ones((2, 1025), f32)])
    with pytest.raises(NotImplementedError, match="1 query tile.s. and two token blocks of dimension 417 do not fit in LDS"):
        coll.add_multi_vectors([1], [np.ones((2, 417), f32)])
    with pytest.raises(ValueError, match="fixes dim_mv"):
        coll.add_multi_vectors([1], [[]])
    assert coll._mv_dim is None and coll.multi_vector_len() == 0
    coll.add_multi_vectors([1, 2], [np.ones((2, 416), f32), []])   # the widest dimension served; a record without tokens
    for ids, sets, exc, msg in [
        ([1], [np.ones((1, 416), f32)], RuntimeError, "multi-vector id 1 was already added"),
        ([3, 3], [np.ones((1, 416), f32)] * 2, RuntimeError, "multi-vector id 3 was already added"),
        ([3, 2], [np.ones((1, 416), f32)] * 2, RuntimeError, "multi-vector id 2 was already added"),   # (an empty record counts)
        ([99], [np.ones((1, 416), f32)], RuntimeError, "cannot add multi-vector for unknown id 99"),
        ([3, 4], [np.ones((1, 416), f32)], RuntimeError, r"ids length \(2\) must match token set count \(1\)"),
        ([3], [np.ones((1, 8), f32)], RuntimeError, "Dimension mismatch: expected 416, got 8"),
        ([3], [np.ones(416, f32)], ValueError, "2-D"),
    ]:
        with pytest.raises(exc, match=msg):
            coll.add_multi_vectors(ids, sets)
        assert coll.multi_vector_len() == 2 and len(coll._mv_pending) == 2 and coll._mv_seen == {1, 2}


def test_c_abi_refusals_without_a_handle():
    import lynsedb_amd._lib as lb

    z = np.zeros(4, np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    h, prof = C.c_void_p(), lb.Profile()
    assert lb.lib.lynse_hip_multivec_create(0, 0, C.byref(h)) == INVALID and not h
    assert lb.lib.lynse_hip_multivec_create(0, 1025, C.byref(h)) == UNSUPPORTED and "above 1024" in lb.last_error() and not h
    assert lb.lib.lynse_hip_multivec_create(0, 417, C.byref(h)) == UNSUPPORTED and "do not fit in LDS" in lb.last_error() and not h
    assert lb.lib.lynse_hip_multivec_create(0, 8, None) == INVALID
    assert lb.lib.lynse_hip_multivec_plan(8, 0, None, None, None) == INVALID and lb.lib.lynse_hip_multivec_plan(8, 257, None, None, None) == UNSUPPORTED
    assert lb.lib.lynse_hip_multivec_append(None, p(z), p(z), 1) == INVALID
    assert lb.lib.lynse_hip_multivec_counts(None, None, None, None) == INVALID and lb.last_error() == "handle is NULL"
    assert lb.lib.lynse_hip_multivec_search_f32(None, p(z), p(z), 1, 1, p(z), p(z), p(z)) == INVALID
    assert lb.lib.lynse_hip_multivec_search_bitset_f32(None, p(z), p(z), 1, 1, p(z), 1, p(z), p(z), p(z)) == INVALID
    assert lb.lib.lynse_hip_multivec_profile_enable(None, 1) == INVALID
    assert lb.lib.lynse_hip_multivec_profile_get(None, C.byref(prof), 0) == INVALID
    assert lb.lib.lynse_hip_multivec_destroy(None) == 0


def test_maxsim_kernels_have_no_scratch():
    import lynsedb_amd

    rep = Path(lynsedb_amd.__file__).parent / "csrc" / "resource_usage.txt"
    assert rep.exists(), "the build writes csrc/resource_usage.txt"
    blocks = re.findall(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", rep.read_text(), flags=re.S)
    mine = [(n, int(s)) for n, s in blocks if "k_maxsim_scan" in n]
    assert len(mine) == 4 and all(s == 0 for _, s in mine), mine
