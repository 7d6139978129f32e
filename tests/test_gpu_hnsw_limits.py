"""HNSW-{IP,L2,COS} at its limits: the code paths of csrc/hnsw.h and csrc/hnsw_host.inc, and of the beam and the search driver they
share with DiskANN (csrc/graph.h, csrc/graph_host.inc), that the shapes of tests/test_gpu_hnsw.py never reach — builds whose candidate lists come from the staged plan, a build level in more than one pass, beams beyond 64 KiB of LDS up to the
160 KiB limit and the refusal behind it, m = 31 / 32, the tie-keeping compaction of the bounded candidate set, the count of distances
scored, the widest row the select kernel holds, and level 52.  The method is that of tests/test_gpu_hnsw.py: levels, adjacency, entry
point, result ids, f32 distance bits and counts are compared exactly with the restatement (tests/hnsw_ref/hnsw_ref.c); the designed
graphs (tests/hnsw_common.py) are also held to the answers written out by hand there.  No tolerances."""
import numpy as np
import pytest

import hnsw_common as H
from hnsw_common import COS, IP, L2, NAME, assert_same_graph, check, combos_for, load, make_data, scored_sweep

pytestmark = pytest.mark.gpu
f32 = np.float32
LDS_MAX = 160 * 1024   # the LDS a workgroup of gfx950 can be given


@pytest.fixture(scope="module")
def L():
    import lynsedb_amd as L_

    assert L_._lib.device_count() >= 1
    return L_


@pytest.fixture(scope="module")
def ref(tmp_path_factory, oracle):
    return H.build_ref(tmp_path_factory.mktemp("hnsw_ref"), oracle)


def flat(L, data):
    idx = L.FlatIndex(None, data.shape[1], device=0)
    idx.write(data)
    return idx


# ------------------------------------------------------------------------- 1. the staged plan ----
@pytest.mark.parametrize("m,kind", [(m, kind) for m in (2, 4) for kind in ("gauss", "dup", "int")])
def test_build_through_the_staged_plan(L, ref, m, kind):
    """hnsw_build_level -> search_impl over n = 600 > cap = 256 rows: the candidate lists come from the staged plan (stages [0, 256),
    [256, 512), [512, 600): coarse pass, certificate, rerank), the path every build over more than 16,384 rows takes at the default
    plan.  ask = ef_construction + 1 = 64 = cap / 4 is the largest such a build accepts (`n > h->cap && ef_construction + 1 >
    h->cap / 4` refuses 65).  With m = 2 level 1 holds more than 256 rows too: the masked search of an upper level is staged as well.
    "dup": tie classes of 15 rows across every stage's cut."""
    n, dim, efc = 600, 24, 63
    rng = np.random.default_rng(1000 * m + len(kind))
    data, queries = make_data(kind, rng, n, dim, 23)
    idx = flat(L, data)
    idx.set_plan(stage0_rows=256, growth=2, cap=256)
    idx.profile_enable(True)
    for metric in (IP, L2, COS):
        seed = 42 + metric
        levels = H.ref_levels(ref, seed, m, None, n)
        if m == 2:
            assert int((levels >= 1).sum()) > 256
        g = H.ref_build(ref, data, metric, m, efc, levels)
        idx.profile_get(reset=True)
        idx.build_hnsw(metric, m, efc, 50, None, seed)
        plan = int(idx.profile_get(reset=True)["last_plan"])
        # bits 8..15: the scan stages of the last exact search of the build; bit 5: the fused single-launch search (include/lynse_hip.h)
        assert (plan >> 8) & 0xFF >= 2 and not plan & 32, hex(plan)
        what = (NAME[metric], m, kind)
        assert_same_graph(idx.hnsw_params(), g, what)
        for k, efq, nq in [(10, 0, 23), (1, 1, 5), (n + 3, n + 5, 2)]:
            q = queries[np.arange(nq) % 23]
            check(idx.search_hnsw_batch_arrays(q, k, metric, efq), H.ref_search(ref, data, metric, g, q, k, max(efq or 50, k)), k, metric, what)
        with pytest.raises(NotImplementedError, match="a quarter of the scan's candidate capacity"):
            idx.build_hnsw(metric, m, efc + 1, 50, None, seed)
        assert_same_graph(idx.hnsw_params(), g, (what, "after the refused build"))


# ------------------------------------------------- 2. a level in two passes, beams beyond 64 KiB ----
@pytest.fixture(scope="module")
def deep(L, ref):
    """5500 x 4, L2, m = 2, ef_construction = 4096, seed 42: built once, with the restatement's graph"""
    n = 5500
    rng = np.random.default_rng(2)
    data, queries = make_data("gauss", rng, n, 4, 5)
    levels = H.ref_levels(ref, 42, 2, None, n)
    g = H.ref_build(ref, data, L2, 2, 4096, levels)
    idx = flat(L, data)
    idx.build_hnsw(L2, 2, 4096, 50, None, 42)
    return idx, data, queries, g


def test_build_level_in_two_passes(deep):
    """hnsw_build_level: qc = min(ns, 256 MiB / (12 (ef_construction + 1)), 128 MiB / (4 D)) = min(5500, 5460, 8388608): level 0 runs
    its 5500 items in passes of 5460 and 40, the second reading d_items + 5460 and writing d_fid + 5460 cap.  (n <= cap = 16384: the
    ask of 4097 is answered by the one-pass plan.)  Top level 13: fourteen levels are built."""
    idx, data, queries, g = deep
    assert (256 << 20) // (12 * 4097) == 5460 and int(g.levels.max()) == 13
    p = idx.hnsw_params()
    assert np.array_equal(p["adj0"][5460:], g.adj0[5460:]), ("the rows of the second pass", np.nonzero((p["adj0"][5460:] != g.adj0[5460:]).any(axis=1))[0][:5] + 5460)
    assert_same_graph(p, g, "5500 x 4, ef_construction 4096")


def test_beams_beyond_64_kib(deep, ref):
    """lynse_hip_flat_search_hnsw_f32: lds = GraphSearchLds::bytes(ef, hnsw_c_cap(ef), D) = 24 ef + 320 + 4 D with ef = min(max(ef, k), n).  (k 10, ef 4096): 98,640 B, the first beam that
    needs the raised LDS attribute (launch_lds -> ensure_lds beyond 64 KiB); (k 5400, the index's ef): ef = 5400, 129,936 B.  The descent
    runs from level 13.  The scored count of both batches equals the restatement's."""
    idx, data, queries, g = deep
    assert 24 * 4096 + 320 + 16 == 98_640 > 65_536 and 24 * 5400 + 320 + 16 == 129_936
    scored_sweep(idx, ref, data, g, L2, queries, [(10, 4096, 5), (5400, 0, 2)])


# ---------------------------------------------------------- 3. the largest beam, and the refusal ----
def test_largest_beam_and_the_refusal(L, ref):
    """lynse_hip_flat_search_hnsw_f32: `lds > PoolRerank::LDS_MAX` refuses.  R holds ef keys and C 2 ef + 8 keys of 8 bytes, the
    expansion list 64 ids of 4 bytes, the query D floats: 24 ef + 64 + 256 + 4 D bytes.  With D = 4 and 160 KiB = 163,840 bytes the
    largest ef is floor((163840 - 320 - 16) / 24) = 6812 (163,824 bytes); 6813 needs 163,848.  n = 7000 keeps min(ef, n) out of it."""
    n, dim = 7000, 4
    k_max = (LDS_MAX - (64 + 256) - 4 * dim) // 24
    assert k_max == 6812 and 24 * k_max + 320 + 4 * dim == 163_824 and 24 * (k_max + 1) + 320 + 4 * dim > LDS_MAX
    rng = np.random.default_rng(3)
    data, queries = make_data("gauss", rng, n, dim, 2)
    g = H.random_graph(rng, n, 32)
    idx = flat(L, data)
    for metric in (IP, L2, COS):
        load(idx, g, metric)
        check(idx.search_hnsw_batch_arrays(queries, k_max, metric), H.ref_search(ref, data, metric, g, queries, k_max, k_max), k_max, metric, (NAME[metric], k_max))
        with pytest.raises(NotImplementedError, match="do not fit in LDS"):
            idx.search_hnsw_batch_arrays(queries, k_max + 1, metric)
        check(idx.search_hnsw_batch_arrays(queries, 10, metric), H.ref_search(ref, data, metric, g, queries, 10, 50), 10, metric, (NAME[metric], "after the refusal"))


# ------------------------------------------------------------------------------ 4. m at its ends ----
@pytest.mark.parametrize("n,dim,m,fill,p_up,kind", [(65, 8, 3, 0.8, None, "gauss"), (65, 3, 5, 1.0, None, "int"), (65, 20, 31, 0.8, None, "dup"),
                                                    (65, 128, 32, 1.0, None, "gauss"), (600, 20, 3, 1.0, None, "dup"), (600, 8, 5, 0.8, None, "nonfinite"),
                                                    (600, 3, 31, 1.0, None, "int"), (600, 24, 32, 0.8, None, "gauss"), (600, 8, 32, 1.0, 0.5, "gauss")])
def test_search_at_the_ends_of_m(L, ref, n, dim, m, fill, p_up, kind):
    """k_hnsw_search with 2 m = 62 / 64 stored level-0 neighbours (graph_beam, csrc/graph.h, `lane < width` with width = 2 m: one per lane,
    all 64 lanes at m = 32) and upper lists
    of 31 / 32 scored in four steps of 8 (`lane < a.m`), beside the odd m = 3 / 5 whose lists end inside a step.  fill = 1.0: every
    level-0 list holds 2 m ids; with p_up = 0.5 half the nodes of a level are on the next, so every upper list holds 32 too.  Every batch's
    scored count is compared as well."""
    rng = np.random.default_rng(n * 1000 + dim * 7 + m)
    data, queries = make_data(kind, rng, n, dim, 37)
    g = H.random_graph(rng, n, m, max_level=3 if p_up else None, fill=fill, p_up=p_up)
    if fill == 1.0:
        assert (g.adj0 != H.PAD).all()
    if p_up:
        assert (g.upper_adj != H.PAD).all() and g.upper_adj.shape[0] > 300
    idx = flat(L, data)
    for metric in (IP, L2, COS):
        load(idx, g, metric)
        scored_sweep(idx, ref, data, g, metric, queries, combos_for(n))


@pytest.mark.parametrize("n,dim,m,efc,kind", [(1500, 16, 32, 128, "gauss"), (600, 8, 31, 8, "dup"), (600, 8, 32, 128, "int")])
def test_build_at_the_ends_of_m(L, ref, n, dim, m, efc, kind):
    """k_hnsw_select with cap = 2 m = 62 / 64 at level 0: kept_id[64] / kept_d[64] fill to the last slot, the fill of free slots
    (`slot < cap`) and the final write (`lane < cap`) use every lane; cap = m = 31 / 32 above."""
    rng = np.random.default_rng(n + dim + m + efc)
    data, queries = make_data(kind, rng, n, dim, 23)
    idx = flat(L, data)
    for metric in (IP, L2, COS):
        seed = 42 + metric
        g = H.ref_build(ref, data, metric, m, efc, H.ref_levels(ref, seed, m, None, n))
        idx.build_hnsw(metric, m, efc, 50, None, seed)
        what = (NAME[metric], n, dim, m, efc, kind)
        assert_same_graph(idx.hnsw_params(), g, what)
        for k, efq, nq in [(10, 0, 23), (1, 1, 5), (n + 3, n + 5, 2)]:
            q = queries[np.arange(nq) % 23]
            check(idx.search_hnsw_batch_arrays(q, k, metric, efq), H.ref_search(ref, data, metric, g, q, k, max(efq or 50, k)), k, metric, what)


# ------------------------------------------------------------------------ 5. the designed graphs ----
def run_designed(L, ref, case):
    """the answer written out by hand (rows, distance bits, distances scored), then parity and the scored count under all three metrics"""
    idx = flat(L, case.data)
    load(idx, case.g, L2)
    idx.profile_enable(True)
    idx.hnsw_stage_times(reset=True)
    rows, dists, counts = idx.search_hnsw_batch_arrays(case.query, case.k, L2, case.ef)
    t = idx.hnsw_stage_times(reset=True)
    c = int(counts[0])
    assert c == case.rows.size and rows[0, :c].tolist() == case.rows.tolist(), (case.name, rows[0, :c], case.rows)
    assert np.array_equal(dists[0, :c].view(np.uint32), case.dists.view(np.uint32)), (case.name, dists[0, :c], case.dists)
    assert t["scored"] == case.scored, (case.name, t["scored"], case.scored)
    queries = np.array([[0.25], [1.5], [-40.0]], f32)
    for metric in (IP, L2, COS):
        load(idx, case.g, metric)
        scored_sweep(idx, ref, case.data, case.g, metric, queries, [(case.k, case.ef, 3)])


def test_compaction_keeps_ties(L, ref):
    """k_hnsw_search's beam (graph_beam, csrc/graph.h), `if (Cn + 8 > c_cap)` -> graph_compact with `(kx >> 32) <= wd`: with ef = 3 (c_cap = 14) the ninth neighbour of the
    entry finds C at 8 entries and forces the compaction while rows 5 and 6, out of R, tie with worst.dist; row 10 is reachable through
    row 6 only.  `<` for `<=` answers [8, 7, 4] (tests/test_hnsw_modes.py shows it on a model)."""
    run_designed(L, ref, H.tie_bridge())


@pytest.mark.parametrize("kind", ["descending", "ascending", "ties"])
def test_fans(L, ref, kind):
    """k_hnsw_search's beam (graph_beam, csrc/graph.h), admission, `!full || (key >> 32) < (worst >> 32)`, over one expansion of 64 (m = 32): descending distances — every
    neighbour is admitted and, with c_cap = 2 ef + 8 <= 26, every scoring step after the first compacts; ascending — nothing is admitted
    once R is full; 64 neighbours at exactly worst.dist — none is admitted (strict, on the distance alone).  ef = k on both sides of 8."""
    for ef in H.FAN_EFS:
        run_designed(L, ref, H.fan(kind, ef))


def test_all_ties(L, ref):
    """k_hnsw_search's beam (graph_beam, csrc/graph.h), `Rn >= ef && (best >> 32) > (worst >> 32)`: with every distance equal nothing is ever beyond worst.dist, so the
    loop `while (Cn && !broken)` ends by C running empty, after each admitted node was popped and expanded.  600 copies of one row on
    the path graph, and a NaN query (every distance +inf at once) over Gaussian rows on the path graph and on a random graph."""
    for k, ef in H.ALL_TIES:
        run_designed(L, ref, H.all_ties(k, ef))
    rng = np.random.default_rng(3)
    data = rng.standard_normal((600, 8)).astype(f32)
    q = np.full((2, 8), np.nan, f32)
    q[1, 3] = 1.0
    idx = flat(L, data)
    for g in (H.path_graph(600), H.random_graph(rng, 600, 4)):
        for metric in (IP, L2, COS):
            load(idx, g, metric)
            scored_sweep(idx, ref, data, g, metric, q, [(k, ef, 2) for k, ef in H.ALL_TIES])
    load(idx, H.path_graph(600), IP)
    rows, dists, counts = idx.search_hnsw_batch_arrays(q, 10, IP, 50)
    assert counts.tolist() == [10, 10] and (rows == np.arange(10, dtype=np.uint64)).all() and (dists == -np.inf).all()


@pytest.mark.parametrize("kind", ["slot 31", "equal", "same list", "level 52"])
def test_descent(L, ref, kind):
    """k_hnsw_search, the greedy descent: `for (b = 0; b < deg; b += 8)` over a list of 32 whose only improvement is slot 31; `dt < cd`
    strict (a node at exactly the current distance does not move cur); a pass keeps scanning the list it started from after cur
    moved (`list` is taken before the loop); `for (lvl = a.top_level; lvl >= 1; --lvl)` from level 52, the highest the level rule
    yields (lynse_hip_flat_load_hnsw accepts `levels[i] <= HNSW_LEVEL_MAX`)."""
    run_designed(L, ref, H.descent(kind))


def test_level_53_is_refused(L):
    """lynse_hip_flat_load_hnsw: `levels[i] > HNSW_LEVEL_MAX` -> "a level beyond 52"; the graph loaded before stays"""
    ok, bad = H.descent("level 52"), H.descent("level 53")
    idx = flat(L, ok.data)
    load(idx, ok.g, L2)
    with pytest.raises(ValueError, match="beyond 52"):
        load(idx, bad.g, L2)
    p = idx.hnsw_params()
    assert p["top_level"] == 52 and p["n_upper"] == 52 * 53 // 2
    assert_same_graph(p, ok.g, "level 52")


@pytest.mark.parametrize("n", H.VISITED_NS)
def test_visited_words(L, ref, n):
    """k_hnsw_search's beam (graph_beam, csrc/graph.h), `atomicOr(&vis[nb >> 5], 1u << (nb & 31u))` with vis_words = (n + 31) / 32: one expansion marks rows 31 | 32, 63 |
    64 — two lanes on one word, words 0, 1 and 2 — at n = 32 / 33 / 64 / 65, where the last word is full or holds one bit; rows named
    again by later lists are not scored twice (the scored count)."""
    run_designed(L, ref, H.visited_words(n))


# --------------------------------------------------------------------- 6b. the chunks of a search ----
def test_search_in_two_chunks(L):
    """graph_search (csrc/graph_host.inc): qc = min(nq, 256 MiB / (4 vis_words), ...).  n = 2^22 rows give vis_words = 131,072 (512 KiB of
    visited bits per query) and qc = 512, so 513 queries go as chunks of 512 and 1: the second uploads `queries + q0 * D` and copies
    back to `out_rows + q0 * k`, `out_dists + q0 * k` and `out_counts + q0`.  Every list is pads and every level 0 (m = 2): the entry is row 0,
    each query scores it alone and answers it with its own distance — integer coordinates, so every L2 distance is exact in f32."""
    n, nq, k = 1 << 22, 513, 3
    assert (256 << 20) // (4 * ((n + 31) // 32)) == nq - 1
    rng = np.random.default_rng(22)
    data = rng.integers(-8, 9, (n, 2)).astype(f32)
    queries = np.stack([np.arange(nq) % 32 - 16, np.arange(nq) // 32 - 8], axis=1).astype(f32)
    assert np.unique(queries, axis=0).shape[0] == nq
    idx = flat(L, data)
    g = H.Graph(2, np.zeros(n, np.uint32), np.full((n, 4), H.PAD, np.uint32), np.zeros((0, 2), np.uint32), 0)
    load(idx, g, L2)
    idx.profile_enable(True)
    idx.hnsw_stage_times(reset=True)
    rows, dists, counts = idx.search_hnsw_batch_arrays(queries, k, L2)
    t = idx.hnsw_stage_times(reset=True)
    idx.profile_enable(False)
    exp = ((queries - data[0]) ** 2).sum(axis=1, dtype=f32)
    assert counts.tolist() == [1] * nq, np.nonzero(counts != 1)[0][:5]
    assert (rows[:, 0] == 0).all() and (rows[:, 1:] == np.uint64(0xFFFFFFFFFFFFFFFF)).all()
    assert np.array_equal(dists[:, 0].view(np.uint32), exp.view(np.uint32)), np.nonzero(dists[:, 0] != exp)[0][:5]
    assert (dists[:, 1:] == np.inf).all()
    assert (t["searches"], t["scored"]) == (1, nq), t


# -------------------------------------------------------------------------------- 7. the widest row ----
def test_widest_row(L, ref):
    """lynse_hip_flat_build_hnsw / _load_hnsw: `dim * 4 + 512 > PoolRerank::LDS_MAX` refuses.  k_hnsw_select holds kept_id[64], kept_d[64]
    (512 bytes) and the candidate's row: D = (163840 - 512) / 4 = 40,832 fills the 160 KiB exactly, 40,833 is refused.  The exact
    searches of the build take the staged plan at this width (the fused search holds rows of up to 5,616 floats), whose kernels read
    the rows in pieces and size no LDS by D; the beam of the search needs 24 ef + 320 + 4 D = 163,768 bytes at ef = min(50, n) = 5."""
    dim = (LDS_MAX - 512) // 4
    assert dim == 40_832 and 4 * dim + 512 == LDS_MAX and 24 * 5 + 320 + 4 * dim <= LDS_MAX
    rng = np.random.default_rng(7)
    data, queries = make_data("gauss", rng, 5, dim + 1, 2)
    idx = flat(L, np.ascontiguousarray(data[:, :dim]))
    levels = H.ref_levels(ref, 42, 2, None, 5)
    g = H.ref_build(ref, data[:, :dim], COS, 2, 8, levels)
    idx.build_hnsw(COS, 2, 8, 50, None, 42)
    assert_same_graph(idx.hnsw_params(), g, "D = 40,832")
    q = np.ascontiguousarray(queries[:, :dim])
    check(idx.search_hnsw_batch_arrays(q, 3, COS), H.ref_search(ref, data[:, :dim], COS, g, q, 3, 50), 3, COS, "D = 40,832")
    wide = flat(L, data)
    with pytest.raises(NotImplementedError, match="does not fit in LDS"):
        wide.build_hnsw(COS, 2, 8, 50, None, 42)
    with pytest.raises(NotImplementedError, match="does not fit in LDS"):
        load(wide, g, COS)
    assert wide.hnsw_params()["m"] == 0
