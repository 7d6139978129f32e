"""f16 token storage of multi-vector search without a GPU (include/lynse_hip.h, F16 TOKEN STORAGE): the dtype argument, the plan of
rule 7' and its refusals, the C refusals that need no handle, and the new kernel's entries in the build's resource report."""
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


@pytest.mark.parametrize("spelling,want", [(None, "f32"), ("f32", "f32"), ("float32", "f32"), ("f16", "f16"), ("float16", "f16"), (" F16 ", "f16")])
def test_dtype_spellings_and_mode(coll, spelling, want):
    assert coll.multi_vector_dtype() is None
    coll.add_multi_vectors([1], [np.ones((2, 8), f32)], dtype=spelling)
    assert coll.multi_vector_dtype() == want
    res = coll.search_multi_vector(np.ones((3, 8), f32), 0)   # k = 0: no device
    assert res.index_mode() == ("MULTIVEC-MAXSIM-IP-F16" if want == "f16" else "MULTIVEC-MAXSIM-IP")


@pytest.mark.parametrize("first,other", [("f16", "f32"), ("f32", "float16"), (None, "f16")])
def test_first_call_fixes_the_dtype(coll, first, other):
    coll.add_multi_vectors([1, 2], [np.ones((2, 8), f32), []], dtype=first)
    fixed = coll.multi_vector_dtype()
    with pytest.raises(RuntimeError, match=f"holds {fixed} tokens"):
        coll.add_multi_vectors([3], [np.ones((1, 8), f32)], dtype=other)
    assert coll.multi_vector_len() == 2 and len(coll._mv_pending) == 2 and coll._mv_seen == {1, 2} and coll.multi_vector_dtype() == fixed
    coll.add_multi_vectors([3], [np.ones((1, 8), np.float16)])   # None: whatever the store has
    coll.add_multi_vectors([4], [np.ones((1, 8), f32)], dtype=fixed)
    assert coll.multi_vector_len() == 4 and coll.multi_vector_dtype() == fixed
    assert coll._mv_pending[2].dtype == (np.float16 if fixed == "f16" else f32)   # raw halves stay halves in an f16 store only


@pytest.mark.parametrize("dim", [417, 1024])
def test_f16_store_accepts_what_f32_refuses(coll, dim):
    with pytest.raises(NotImplementedError, match="do not fit in LDS"):
        coll.add_multi_vectors([1], [np.ones((2, dim), f32)])
    assert coll.multi_vector_dtype() is None
    coll.add_multi_vectors([1], [np.ones((2, dim), f32)], dtype="f16")
    assert coll.multi_vector_len() == 1 and coll._mv_dim == dim


# (dim_mv, Tq) -> (query tiles, LDS bytes before the per-wave area) or None: each pair of lines is the two sides of a boundary of rule 7'
PLAN = [(288, 256, (8, 151552)), (289, 256, None), (289, 128, (4, None)), (512, 128, (4, 133120)), (512, 129, None),
        (1024, 64, (2, 132096)), (1024, 65, None), (520, 65, (4, None)), (128, 32, (1, 8704))]


@pytest.mark.parametrize("dim,tq,want", PLAN)
def test_f16_plan_and_its_refusal(coll, dim, tq, want):
    import lynsedb_amd._lib as lb

    tiles, waves, lds = C.c_uint32(0), C.c_uint32(0), C.c_uint64(0)
    rc = lb.lib.lynse_hip_multivec_plan_dtype(dim, tq, 1, C.byref(tiles), C.byref(waves), C.byref(lds))
    coll.add_multi_vectors([1], [np.ones((2, dim), f32)], dtype="f16")   # the store can always exist
    if want is None:
        assert rc == UNSUPPORTED and "do not fit in LDS" in lb.last_error()
        with pytest.raises(NotImplementedError, match="do not fit in LDS"):   # the query is what is refused, before a device is touched
            coll.search_multi_vector(np.ones((tq, dim), f32), 3)
    else:
        assert rc == 0 and tiles.value == want[0] and waves.value == 4 and lds.value <= 160 * 1024
        assert want[1] is None or want[1] <= lds.value <= want[1] + 512
        assert len(coll.search_multi_vector(np.ones((tq, dim), f32), 0)) == 0


def test_c_abi_refusals_without_a_handle():
    import lynsedb_amd._lib as lb

    z = np.zeros(4, np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    h = C.c_void_p()
    assert lb.lib.lynse_hip_multivec_create_dtype(0, 8, 2, C.byref(h)) == INVALID and "dtype" in lb.last_error() and not h
    assert lb.lib.lynse_hip_multivec_create_dtype(0, 8, 1, None) == INVALID
    assert lb.lib.lynse_hip_multivec_create_dtype(0, 0, 1, C.byref(h)) == INVALID and not h
    assert lb.lib.lynse_hip_multivec_create_dtype(0, 1025, 1, C.byref(h)) == UNSUPPORTED and "above 1024" in lb.last_error() and not h
    assert lb.lib.lynse_hip_multivec_create_dtype(0, 417, 0, C.byref(h)) == UNSUPPORTED and "do not fit in LDS" in lb.last_error() and not h
    assert lb.lib.lynse_hip_multivec_plan_dtype(8, 1, 2, None, None, None) == INVALID
    assert lb.lib.lynse_hip_multivec_plan_dtype(8, 0, 1, None, None, None) == INVALID
    assert lb.lib.lynse_hip_multivec_plan_dtype(8, 257, 1, None, None, None) == UNSUPPORTED
    assert lb.lib.lynse_hip_multivec_append_f16(None, p(z), p(z), 1) == INVALID and lb.last_error() == "handle is NULL"


def test_h16_kernels_have_no_scratch():
    import lynsedb_amd

    rep = Path(lynsedb_amd.__file__).parent / "csrc" / "resource_usage.txt"
    assert rep.exists(), "the build writes csrc/resource_usage.txt"
    blocks = re.findall(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", rep.read_text(), flags=re.S)
    mine = [(n, int(s)) for n, s in blocks if "k_maxsim_h16" in n]
    assert len(mine) == 4 and all(s == 0 for _, s in mine), mine
