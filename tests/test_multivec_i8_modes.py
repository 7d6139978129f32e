"""int8 token storage of multi-vector search without a GPU (include/lynse_hip.h, INT8 TOKEN STORAGE): the dtype argument, the plan of
rule 7" and its refusals, the C refusals that need no handle, and the new kernel's entries in the build's resource report."""
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


@pytest.mark.parametrize("spelling", ["i8", "int8", " INT8 ", "I8"])
def test_dtype_spellings_and_mode(coll, spelling):
    coll.add_multi_vectors([1], [np.ones((2, 8), np.float16)], dtype=spelling)
    assert coll.multi_vector_dtype() == "i8" and coll._mv_pending[0].dtype == f32   # halves are widened, the device quantises
    assert coll.search_multi_vector(np.ones((3, 8), f32), 0).index_mode() == "MULTIVEC-MAXSIM-IP-I8"   # k = 0: no device


@pytest.mark.parametrize("first,other", [("i8", "f32"), ("i8", "f16"), ("f32", "i8"), ("f16", "int8")])
def test_first_call_fixes_the_dtype(coll, first, other):
    coll.add_multi_vectors([1, 2], [np.ones((2, 8), f32), []], dtype=first)
    with pytest.raises(RuntimeError, match=f"holds {first} tokens"):
        coll.add_multi_vectors([3], [np.ones((1, 8), f32)], dtype=other)
    coll.add_multi_vectors([3], [np.ones((1, 8), f32)])   # None: whatever the store has
    assert coll.multi_vector_len() == 3 and coll._mv_seen == {1, 2, 3} and coll.multi_vector_dtype() == first


# (dim_mv, Tq) -> (query tiles, LDS bytes) or None: DESIGN.md §30's table, both sides of each boundary of rule 7"
PLAN = [(608, 256, (8, 161280)), (609, 256, None), (609, 129, None), (609, 128, (4, 84992)), (1024, 128, (4, 134144)), (1024, 129, None),
        (128, 32, (1, 5248))]


@pytest.mark.parametrize("dim,tq,want", PLAN)
def test_i8_plan_and_its_refusal(coll, dim, tq, want):
    import lynsedb_amd._lib as lb

    tiles, waves, lds = C.c_uint32(0), C.c_uint32(0), C.c_uint64(0)
    rc = lb.lib.lynse_hip_multivec_plan_i8(dim, tq, C.byref(tiles), C.byref(waves), C.byref(lds))
    coll.add_multi_vectors([1], [np.ones((2, dim), f32)], dtype="i8")   # the store can always exist
    if want is None:
        assert rc == UNSUPPORTED and "do not fit in LDS" in lb.last_error()
        with pytest.raises(NotImplementedError, match="do not fit in LDS"):   # the query is what is refused, before a device is touched
            coll.search_multi_vector(np.ones((tq, dim), f32), 3)
    else:
        assert rc == 0 and (tiles.value, waves.value, lds.value) == (want[0], 4, want[1]) and lds.value <= 160 * 1024
        assert len(coll.search_multi_vector(np.ones((tq, dim), f32), 0)) == 0


def test_c_abi_refusals_without_a_handle():
    import lynsedb_amd._lib as lb

    h = C.c_void_p()
    assert lb.lib.lynse_hip_multivec_create_i8(0, 8, None) == INVALID
    assert lb.lib.lynse_hip_multivec_create_i8(0, 0, C.byref(h)) == INVALID and not h
    assert lb.lib.lynse_hip_multivec_create_i8(0, 1025, C.byref(h)) == UNSUPPORTED and "above 1024" in lb.last_error() and not h
    assert lb.lib.lynse_hip_multivec_plan_i8(0, 1, None, None, None) == INVALID
    assert lb.lib.lynse_hip_multivec_plan_i8(1025, 1, None, None, None) == UNSUPPORTED and "above 1024" in lb.last_error()
    assert lb.lib.lynse_hip_multivec_plan_i8(8, 0, None, None, None) == INVALID
    assert lb.lib.lynse_hip_multivec_plan_i8(8, 257, None, None, None) == UNSUPPORTED


def test_i8_kernels_have_no_scratch():
    import lynsedb_amd

    rep = Path(lynsedb_amd.__file__).parent / "csrc" / "resource_usage.txt"
    assert rep.exists(), "the build writes csrc/resource_usage.txt"
    blocks = re.findall(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", rep.read_text(), flags=re.S)
    mine = sorted((n, int(s)) for n, s in blocks if "k_maxsim_i8" in n)
    assert [n for n, _ in mine] == [f"_ZN5lynse11k_maxsim_i8ILi{t}EEEvNS_12MaxSimI8ArgsE" for t in (1, 2, 4, 8)] and all(s == 0 for _, s in mine), mine
