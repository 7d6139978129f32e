"""Multi-vector rerank without a GPU: the refusals that precede device work, the ids that drop out, results that need no device."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

f32, u64 = np.float32, np.uint64
INVALID, UNSUPPORTED = 1, 9


@pytest.fixture()
def coll():
    """a collection that never opened a device: ids 1 .. 5 are known, 1 .. 4 hold token sets (3 none, 4 is deleted)"""
    import lynsedb_amd as L

    c = L.Collection.__new__(L.Collection)
    c._id_arrays, c._pending_ids, c._tombstone = [np.arange(1, 6, dtype=np.int64)], [], set()
    c._mv_reset()
    c.add_multi_vectors([1, 2, 3, 4], [np.ones((2, 1024), f32), np.ones((1, 1024), f32), [], np.ones((1, 1024), f32)], dtype="f16")
    c._tombstone.add(4)
    return c


def p(a):
    return np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)


# (q_ptr, cand_rows, cand_ptr, NULL out_counts) -> (code, message); all of it is checked before the handle, which is NULL throughout
C_CASES = [([0, 1], [0, 1], [0, 2], True, INVALID, "NULL argument"),
           ([1, 2], [0, 1], [0, 2], False, INVALID, "q_ptr must start at 0"),
           ([0, 0], [0, 1], [0, 2], False, INVALID, "at least one token"),
           ([0, 257], [0, 1], [0, 2], False, UNSUPPORTED, "more than 256 tokens"),
           ([0, 1], [0, 1], None, False, INVALID, "NULL argument"),
           ([0, 1], [0, 1], [1, 2], False, INVALID, "cand_ptr must start at 0"),
           ([0, 1, 2], [0, 1], [0, 2, 1], False, INVALID, "must not descend"),
           ([0, 1], None, [0, 2], False, INVALID, "NULL argument"),
           ([0, 1], [3, 1], [0, 2], False, INVALID, "strictly ascending"),
           ([0, 1], [1, 1], [0, 2], False, INVALID, "strictly ascending"),
           ([0, 1, 2], [5, 1], [0, 1, 2], False, INVALID, "handle is NULL")]   # (each list ascends: only the handle is left to refuse)


@pytest.mark.parametrize("q_ptr,rows,c_ptr,no_counts,code,msg", C_CASES)
def test_c_refusals_before_the_handle(q_ptr, rows, c_ptr, no_counts, code, msg):
    import lynsedb_amd._lib as lb

    nq = len(q_ptr) - 1
    tokens, out = np.ones((300, 8), f32), np.zeros(8, u64)
    rc = lb.lib.lynse_hip_multivec_rerank_f32(None, p(tokens), p(np.array(q_ptr, u64)), nq, 2, None if rows is None else p(np.array(rows, u64)),
                                              None if c_ptr is None else p(np.array(c_ptr, u64)), p(out), p(out.view(f32)),
                                              None if no_counts else p(np.zeros(4, np.uint32)))
    assert rc == code and msg in lb.last_error(), lb.last_error()


@pytest.mark.parametrize("tq,exc,msg", [(0, ValueError, "at least one token"), (257, NotImplementedError, "more than 256"),
                                        (65, NotImplementedError, "do not fit in LDS")])   # (f16 at dim_mv 1024 serves 64 query tokens)
def test_python_refuses_the_query_before_a_device(coll, tq, exc, msg):
    with pytest.raises(exc, match=msg):
        coll.rerank_multi_vector(np.ones((tq, 1024), f32), [1, 2])
    with pytest.raises(RuntimeError, match="Dimension mismatch"):
        coll.rerank_multi_vector(np.ones((1, 8), f32), [1, 2])
    with pytest.raises(RuntimeError, match="must match the queries"):
        coll.batch_rerank_multi_vector([np.ones((1, 1024), f32)], [[1], [2]])
    with pytest.raises(OverflowError):
        coll.rerank_multi_vector(np.ones((1, 1024), f32), [1], k=-1)


@pytest.mark.parametrize("ids,k", [([], None), ([9, 4, 4, -1, 2], None), ([1, 3], 0), ([4, 2], 3)])
def test_nothing_to_score_needs_no_handle(coll, ids, k):
    """unknown (9, -1), tombstoned (4), compacted-away (2) and repeated ids drop out; k = 0 and an empty list return empty results"""
    coll._mv_dead.add(2)
    res = coll.rerank_multi_vector(np.ones((3, 1024), f32), ids, k)
    assert len(res) == 0 and res.index_mode() == "MULTIVEC-MAXSIM-IP-F16" and coll._mv_index is None
    assert [len(r) for r in coll.batch_rerank_multi_vector([np.ones((1, 1024), f32)] * 2, [ids, []], k)] == [0, 0] and coll._mv_index is None


def test_candidate_kernels_have_no_scratch():
    import lynsedb_amd

    rep = Path(lynsedb_amd.__file__).parent / "csrc" / "resource_usage.txt"
    blocks = re.findall(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", rep.read_text(), flags=re.S)
    mine = sorted((n, int(s)) for n, s in blocks if "k_maxsim_cand" in n)
    assert len(mine) == 8 and all(s == 0 for _, s in mine), mine
