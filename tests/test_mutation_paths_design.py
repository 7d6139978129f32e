"""The properties of the inputs of tests/test_gpu_mutation_paths.py (tests/mutation_common.py), on the CPU and with the oracle alone: a derived
copy that survived a mutation would be noticed.  Such a copy describes the stale layout — the old rows at their old positions, cut at the new
length.  For every case and every metric it searches:
  - every planted query of kinds (a) and (b) has another best row, or other distance bits, over the stale layout than over the final rows;
  - every (b) query's best row over the final rows no longer holds the content the query copies, every (c) query's best row is its appended source;
  - of the unplanted queries of the 40-query batch at least half differ somewhere in the top-10.
The share is a condition on the committed seeds, not on any kernel.  No GPU; if a seed or a generator changes, this file reports the lost
coverage instead of the GPU file going quietly soft."""
import numpy as np
import pytest

import mutation_common as M
import oracle as O
from conftest import oracle_for_every_query

f32 = np.float32


def test_metric_ids_are_the_oracles():
    assert M.METRIC_IDS == {"ip": O.IP, "l2": O.L2, "cosine": O.COS, "hamming": O.HAMMING}


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


@pytest.fixture(scope="module")
def report():
    lines = []
    yield lines
    print("\n" + "\n".join(lines))


@pytest.mark.parametrize("name", sorted(M.SPECS))
def test_a_stale_layout_would_be_noticed(oracle, name, report):
    c = M.case(name)
    s = c.spec
    n_after = c.after.shape[0]
    assert c.stale.shape == c.after.shape and not np.array_equal(c.stale, c.after)
    if s.kind == "compact":
        assert not c.keep[0] and n_after == int(c.keep.sum()) < s.n0
        assert c.keep[c.src_a].all() and not c.keep[c.src_b].any() and (c.src_b < n_after).all()
        new_at = np.cumsum(c.keep) - 1
        assert (new_at[c.src_a] != c.src_a).all()                                    # (a): the index shifted
        assert np.array_equal(c.after[new_at[c.src_a]], c.q_a)
    else:
        assert n_after == s.n0 and np.isin(c.src_b, c.rows_changed).all() and np.unique(c.rows_changed).size == s.n_change
        norms = (c.before.astype(np.float64) ** 2).sum(axis=1)
        assert {int(norms.argmax()), int(norms.argmin())} <= set(c.rows_changed.tolist())
        after_norms = (c.after.astype(np.float64) ** 2).sum(axis=1)
        assert after_norms.max() < norms.max() and after_norms.min() > norms.min()   # the collection maximum falls, the minimum rises
    if s.n_append:
        assert n_after + s.n_inside <= s.n0 < n_after + s.n_append or s.kind == "update"   # the short append fits what the compaction freed, the long one does not
        final = c.final(s.n_inside)
        assert final.shape[0] == n_after + s.n_inside and np.array_equal(final[c.src_c], c.q_c) and (c.src_c >= n_after).all()
    q = c.batch(40)
    n_planted = len(c.q_a) + len(c.q_b) + (len(c.q_c) if c.q_c is not None else 0)
    assert np.array_equal(q[:len(c.q_a)], c.q_a) and np.array_equal(q[len(c.q_a):len(c.q_a) + len(c.q_b)], c.q_b)
    assert np.array_equal(c.batch(256)[:n_planted], q[:n_planted])                    # every batch size plants the same queries
    for metric in s.metrics:
        stale = oracle_for_every_query(lambda i: M.oracle_topk(oracle, q[i], c.stale, 10, metric, s.f16), 40)
        after = oracle_for_every_query(lambda i: M.oracle_topk(oracle, q[i], c.after, 10, metric, s.f16), 40)
        for kind in "ab":
            for i in c.slots(kind):
                assert not (stale[i][0][0] == after[i][0][0] and stale[i][1][:1].view(np.uint32) == after[i][1][:1].view(np.uint32)), (name, metric, kind, i)
        for i in c.slots("b"):
            assert not np.array_equal(c.after[int(after[i][0][0])], q[i]), (name, metric, i)
            if s.kind == "update" or metric != "ip":
                assert np.array_equal(c.stale[int(stale[i][0][0])], q[i]), (name, metric, i)      # ... while the stale layout still finds it
        for j, i in enumerate(c.slots("a")):
            assert int(after[i][0][0]) == int(np.cumsum(c.keep)[c.src_a[j]] - 1), (name, metric, i)   # (a) finds its row at the new index
        if s.n_append:
            for j, i in enumerate(c.slots("c")):
                ids, _ = M.oracle_topk(oracle, q[i], final, 10, metric, s.f16)
                assert int(ids[0]) == int(c.src_c[j]), (name, metric, i)
        differ = sum(not same(stale[i], after[i]) for i in range(n_planted, 40))
        report.append(f"{name:20s} {metric:7s} unplanted queries whose top-10 differs over the stale layout: {differ} of {40 - n_planted}")
        assert 2 * differ >= 40 - n_planted, (name, metric, differ)


@pytest.mark.parametrize("shape", sorted(M.SEQ_SHAPES))
@pytest.mark.parametrize("seed", M.SEQ_SEEDS)
def test_every_sequence_mutates_and_searches_afterwards(seed, shape):
    n0, dim, f16 = M.SEQ_SHAPES[shape]
    first, ops = M.draw_ops(seed, n0, dim, f16)
    again = M.draw_ops(seed, n0, dim, f16)
    assert np.array_equal(first, again[0]) and M.describe(ops) == M.describe(again[1]) and len(ops) == M.SEQ_STEPS
    kinds = [op[0] for op in ops]
    assert {"write", "update", "compact"} <= set(kinds) and kinds[-1] == "search"
    reads = {"search", "filtered", "range", "aux"}
    for mutation in ("write", "update", "compact"):                                  # each is followed by a read of the shard
        at = kinds.index(mutation)
        assert reads & set(kinds[at + 1:]), (seed, mutation, M.describe(ops))
    # the model replays to a shard that is never empty and that every argument addresses
    model = M.RowModel(dim, f16)
    model.write(first)
    for op in ops:
        n = len(model)
        if op[0] == "write":
            model.write(op[1])
        elif op[0] == "update":
            assert op[1].max() < n and np.unique(op[1]).size == op[1].size
            model.update(op[1], op[2])
        elif op[0] == "compact":
            assert op[1].size == n and not op[1][0]
            model.compact(op[1])
        elif op[0] == "filtered":
            assert op[3].max() < n
        assert len(model) >= 100
    print(f"seed {seed} {shape}: {M.describe(ops)}")
