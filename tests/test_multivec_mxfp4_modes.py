"""MXFP4 token storage of multi-vector search without a GPU (include/lynse_hip.h, MXFP4 TOKEN STORAGE): the dtype argument, the plan of
rule 7''' and its refusals, the C refusals that need no handle, and the new kernels' entries in the build's resource report."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import lynsedb_amd as L

f32, lib = np.float32, L._lib.lib
INVALID, UNSUPPORTED = 1, 9


@pytest.fixture()
def coll():
    """a collection that never opened a device: ids 1 .. 5 are known, nothing else of it is touched before the device"""
    c = L.Collection.__new__(L.Collection)
    c._id_arrays, c._pending_ids, c._tombstone = [np.arange(1, 6, dtype=np.int64)], [], set()
    c._mv_reset()
    return c


@pytest.mark.parametrize("spelling", ["mxfp4", "fp4", " MXFP4 ", "Fp4"])
def test_dtype_spellings_and_mode(coll, spelling):
    coll.add_multi_vectors([1], [np.ones((2, 8), np.float16)], dtype=spelling)
    assert coll.multi_vector_dtype() == "mxfp4" and coll._mv_pending[0].dtype == f32   # halves are widened, the device quantises
    assert coll.search_multi_vector(np.ones((3, 8), f32), 0).index_mode() == "MULTIVEC-MAXSIM-IP-MXFP4"   # k = 0: no device


@pytest.mark.parametrize("first,other", [("mxfp4", "f32"), ("mxfp4", "f16"), ("mxfp4", "i8"), ("f32", "mxfp4"), ("f16", "fp4"), ("i8", "mxfp4")])
def test_first_call_fixes_the_dtype(coll, first, other):
    coll.add_multi_vectors([1, 2], [np.ones((2, 8), f32), []], dtype=first)
    with pytest.raises(RuntimeError, match=f"holds {first} tokens"):
        coll.add_multi_vectors([3], [np.ones((1, 8), f32)], dtype=other)
    coll.add_multi_vectors([3], [np.ones((1, 8), f32)])   # None: whatever the store has
    assert coll.multi_vector_len() == 3 and coll.multi_vector_dtype() == first


# (dim_mv, Tq) -> (query tiles, LDS bytes) or None: DESIGN.md §33's table, both sides of each boundary of rule 7'''
@pytest.mark.parametrize("dim,tq,want", [(576, 256, (8, 156672)), (577, 256, None), (577, 129, None), (577, 128, (4, 82816)), (1024, 128, (4, 137728)),
                                         (1024, 129, None), (128, 32, (1, 5248)), (1, 64, (2, 3648))])
def test_mxfp4_plan_and_its_refusal(coll, dim, tq, want):
    tiles, waves, lds = C.c_uint32(0), C.c_uint32(0), C.c_uint64(0)
    rc = lib.lynse_hip_multivec_plan_mxfp4(dim, tq, C.byref(tiles), C.byref(waves), C.byref(lds))
    coll.add_multi_vectors([1], [np.ones((2, dim), f32)], dtype="mxfp4")   # the store can always exist
    if want is None:
        assert rc == UNSUPPORTED and "of MXFP4 tokens" in L._lib.last_error() and "do not fit in LDS" in L._lib.last_error()
        with pytest.raises(NotImplementedError, match="do not fit in LDS"):   # the query is what is refused, before a device is touched
            coll.search_multi_vector(np.ones((tq, dim), f32), 3)
    else:
        assert rc == 0 and (tiles.value, waves.value, lds.value) == (want[0], 4, want[1]) and lds.value <= 160 * 1024
        assert len(coll.search_multi_vector(np.ones((tq, dim), f32), 0)) == 0


def test_c_abi_refusals_without_a_handle():
    h, err = C.c_void_p(), L._lib.last_error
    assert lib.lynse_hip_multivec_create_mxfp4(0, 8, None) == INVALID
    assert lib.lynse_hip_multivec_create_mxfp4(0, 0, C.byref(h)) == INVALID and not h
    assert lib.lynse_hip_multivec_create_mxfp4(0, 1025, C.byref(h)) == UNSUPPORTED and "above 1024" in err() and not h
    assert lib.lynse_hip_multivec_plan_mxfp4(0, 1, None, None, None) == INVALID
    assert lib.lynse_hip_multivec_plan_mxfp4(1025, 1, None, None, None) == UNSUPPORTED and "above 1024" in err()
    assert lib.lynse_hip_multivec_plan_mxfp4(8, 0, None, None, None) == INVALID and lib.lynse_hip_multivec_plan_mxfp4(8, 257, None, None, None) == UNSUPPORTED
    for dtype in (2, 3):   # the public dtype ids stay 0 and 1: the int8 and MXFP4 stores have entries of their own
        assert lib.lynse_hip_multivec_create_dtype(0, 8, dtype, C.byref(h)) == INVALID and "0 (f32) or 1 (f16)" in err() and not h
        assert lib.lynse_hip_multivec_plan_dtype(8, 1, dtype, None, None, None) == INVALID
    assert lib.lynse_hip_multivec_append_f16(None, None, None, 1) == INVALID and "handle is NULL" in err()


def test_mx4_kernels_have_no_scratch():
    rep = Path(L.__file__).parent / "csrc" / "resource_usage.txt"
    blocks = re.findall(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", rep.read_text(), flags=re.S)
    mine = sorted((n, int(s)) for n, s in blocks if "k_maxsim_mx4" in n or "k_maxsim_store_mx4" in n)
    names = [f"_ZN5lynse12k_maxsim_mx4ILi{t}EEEvNS_13MaxSimMx4ArgsE" for t in (1, 2, 4, 8)] + ["_ZN5lynse18k_maxsim_store_mx4EPKfPjPhmjj"]
    assert [n for n, _ in mine] == names and all(s == 0 for _, s in mine), mine
