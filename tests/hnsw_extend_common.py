"""Shared by tests/test_gpu_hnsw_extend.py and tests/test_hnsw_extend_modes.py: the pattern of the incremental-insert tests (rule 7 of
the HNSW block of include/lynse_hip.h).  The expected graph after an extend is the restatement's build over all rows
(hnsw_common.ref_build with the levels of hnsw_common.levels_py): there is no second restatement."""
import numpy as np

import hnsw_common as H

f32 = np.float32


def extend_steps(L, ref, data, sizes, metric, m, efc, seed=42, max_level=None, mode=0, ef_search=50, path=0, plan=None, what=""):
    """Build over data[:sizes[0]], then for each further size append up to it and extend; after every step the exported graph equals the
    restatement's build over the rows held.  -> (the handle, the last expected graph, the stats of every extend)"""
    idx = L.FlatIndex(None, data.shape[1], device=0)
    idx.write(data[:sizes[0]])
    if plan:
        idx.set_plan(*plan)
    idx.build_hnsw(metric, m, efc, ef_search, max_level, seed)
    stats, g = [], None
    for a, b in zip(sizes[:-1], sizes[1:]):
        idx.write(data[a:b])
        idx.extend_hnsw(mode)
        st = idx.hnsw_extend_stats()
        stats.append(st)
        assert (st["rows_before"], st["rows_after"]) == (a, b), (what, st)
        if path is not None:
            assert st["path"] == path, (what, a, b, st)
        g = H.ref_build(ref, data[:b], metric, m, efc, H.levels_py(seed, m, max_level, b))
        p = idx.hnsw_params()
        assert (p["metric"], p["m"], p["ef_search"], p["n"]) == (metric, m, ef_search, b), (what, p["n"])
        H.assert_same_graph(p, g, (what, H.NAME[metric], a, b))
    return idx, g, stats


def same_as_fresh_build(L, idx, data, metric, m, efc, seed=42, max_level=None, ef_search=50):
    """every array of hnsw_params equal to a build over the same rows on a second handle"""
    other = L.FlatIndex(None, data.shape[1], device=0)
    other.write(data)
    other.build_hnsw(metric, m, efc, ef_search, max_level, seed)
    p, e = idx.hnsw_params(), other.hnsw_params()
    assert p.keys() == e.keys()
    for key in e:
        assert np.array_equal(p[key], e[key]), key


# ---------------------------------------------------------------------- the flag rule, as a numpy model ----
def score(metric, a, b):
    """the raw metric value in float64 (exact for the small integers the model is run on): l2 smaller is better, ip larger"""
    return float(((a - b) ** 2).sum()) if metric == H.L2 else float((a * b).sum())


def ask_list(metric, data, i, n, ask):
    """what the exact search returns for row i over rows [0, n): the best `ask` by (d, row), d = the score negated for ip"""
    sgn = -1.0 if metric == H.IP else 1.0
    order = sorted(range(n), key=lambda r: (sgn * score(metric, data[i], data[r]), r))
    return order[:ask]


def flagged(metric, data, i, n0, n1, ask):
    """rule 7 step b for old row i: the threshold is the score of the last of the `ask` entries over [0, n0) ("short" when fewer came
    back); flagged when short or some new row is not strictly worse than it"""
    lst = ask_list(metric, data, i, n0, ask)
    if len(lst) < ask:
        return True
    thr = score(metric, data[i], data[lst[-1]])
    for x in range(n0, n1):
        s = score(metric, data[i], data[x])
        if not (s < thr if metric == H.IP else s > thr):
            return True
    return False
