"""`-m gpu` tests of the CARRIED step tail of the 16x16x64 int8 scan (scan_qs.h, CARRY): a wave holds the last seven fragments of
a tile in registers across the barrier, runs their MFMAs behind it and only then the tile's epilogue; a workgroup's last tile drains after
the loop with no barrier.  The order only ever changes speed: every case is compared, ids and f32 distance bits, with the CPU oracle (or
the planted answers) and with the same batch on the 32x32x32 form (`LYNSE_HIP_QS_M16=0`), whose order is the plain one.

Shapes, on a grid of one workgroup per CU (W = 256, asserted).  A shard of 65,536 rows is the one size that has both the int8 pass
(>= 65,536 rows) and the contiguous plan (<= 4 x cap rows, cap <= 16,384): stages [0, s0) [s0, g s0) [g s0, g^2 s0) ... with s0 a multiple of 256.
  * default plan (s0 = 256, g = 8): [256, 2048) and [2048, 16384) have 28 and 224 tiles — every workgroup has exactly ONE tile (open, no held
    MFMAs, drain after the loop); [16384, 65536) has 768 tiles — three per workgroup: first tile, steady state, drain;
  * `set_plan(4864, 2, 16384)`: [4864, 9728) 76 tiles, [9728, 19456) 152 tiles, [19456, 38912) 304 tiles — 48 workgroups with TWO tiles beside
    208 with ONE —, [38912, 65536) 416 tiles — 160 with two beside 96 with one: a drain straight after a first tile next to workgroups with
    one steady-state step.  Five scan launches per batch pin that the plan took effect.
After an append to 65,536 + 30,757 rows the sampled plan scans the shard in one stage of 1,505 tiles, the last of them ragged (37 rows):
workgroups with six tiles beside workgroups with five.  The ties case lives there: a private segment (32 keys at 1,024 segments) overflows
only from a workgroup's third tie tile on, which no two-tile stage can reach.
Not reachable: a stage of fewer than 64 rows past its start.  Contiguous plan: n must be exactly 65,536 (below it the int8 pass is off, above
it n > 4 x cap selects the sampled plan), every stage edge is s0 g^j with s0 a multiple of 256, so the last stage [s0 g^j, 65536) is a
multiple of 256 rows long.  Sampled plan: stage edges are rounded up to 256 rows and a last stage shorter than an eighth of the rows before
it is folded into its predecessor (`make_plan`: "do not leave a sliver"), so a last stage holds at least a ninth of the shard (n - b >= b / 8): 7,281 rows at n >= 65,536; the stages before it at least double from 256-row edges.  The shortest stages that exist are the 28-tile one above and the ragged 37-row TILE that ends the appended shard.
The other tests of the form (tests/test_gpu_qs16_scan.py: 327,717 rows, batches in flight; tests/test_gpu_planted_sweeps.py: every row at
every query slot) run the same kernel and stay as they are.
"""
import os

import numpy as np
import pytest

import oracle as O
import planted_common as P
from conftest import oracle_for_every_query

pytestmark = pytest.mark.gpu
f32 = np.float32

PLAN_I8C = 4
PLAN_SQ7 = 1 << 26
PLAN_M16 = 1 << 27
K = 10
EDGE = 16_384              # the last stage edge of the contiguous plan
N_FIRST = 65_536          # the first size: the contiguous plan


@pytest.fixture(scope="module")
def L():
    import lynsedb_amd as L_

    assert L_._lib.device_count() >= 1
    return L_


@pytest.fixture(scope="module")
def W():
    import torch

    w = torch.cuda.get_device_properties(0).multi_processor_count
    assert w == 256, f"the tile counts per workgroup of this file are those of a 256-CU grid, not of {w} CUs"
    return w


N_APPENDED = N_FIRST + 30_757      # rows after the append: 1,505 tiles of 64 rows, the last of them ragged (37 rows)


def search(idx, queries, metric, m16, sq7=None):
    want = {"LYNSE_HIP_QS_M16": str(m16)}
    if sq7 is not None:
        want["LYNSE_HIP_SQ7"] = str(sq7)
    old = {name: os.environ.get(name) for name in want}
    os.environ.update(want)
    try:
        idx.profile_enable(True)
        idx.profile_get(reset=True)
        r, d, c = idx.search_batch_arrays(queries, K, metric)
        return r, d, c, idx.profile_get(reset=True)
    finally:
        for name, v in old.items():
            if v is None:
                os.environ.pop(name, None)
            else:
                os.environ[name] = v


def assert_exact(want, rows, dists, counts, tag):
    for qi, (e_ids, e_d) in enumerate(want):
        c = int(counts[qi])
        assert c == len(e_ids), (tag, qi, c, len(e_ids))
        assert np.array_equal(dists[qi, :c].view(np.uint32), e_d.view(np.uint32)), (tag, qi, dists[qi, :c], e_d)
        assert np.array_equal(rows[qi, :c].astype(np.uint64), e_ids.astype(np.uint64)), (tag, qi, rows[qi, :c], e_ids)


def both_forms(idx, q, metric, sq7, tag):
    """The batch on the 16x16x64 form (pinned by the plan word) and on the 32x32x32 form: bit-identical ids, distances, counts and pool."""
    r16 = search(idx, q, metric, 1, sq7)
    lp = int(r16[3]["last_plan"])
    assert lp & PLAN_M16 and lp & PLAN_I8C and (lp >> 16) & 0xff == 0x81 and r16[3]["fallback_queries"] == 0, (tag, hex(lp), r16[3])
    if sq7 is not None:
        assert bool(lp & PLAN_SQ7) == bool(sq7), (tag, hex(lp))
    r32 = search(idx, q, metric, 0, sq7)
    lp32 = int(r32[3]["last_plan"])
    assert (lp32 ^ lp) == PLAN_M16 and r32[3]["fallback_queries"] == 0, (tag, hex(lp), hex(lp32))
    assert np.array_equal(r16[0], r32[0]) and np.array_equal(r16[1].view(np.uint32), r32[1].view(np.uint32)) and np.array_equal(r16[2], r32[2]), tag
    assert r16[3]["pool_entries"] == r32[3]["pool_entries"], (tag, r16[3], r32[3])
    return r16


def new_index(L, data, plan=None):
    idx = L.FlatIndex(None, data.shape[1])
    if plan:
        idx.set_plan(*plan)
    idx.write(data)
    idx.finalize()
    return idx


_cases = {}


def case(W, kind, dim):
    """Rows, queries near rows of every stage (the first tile, the stage edges, the appended part) — once per (kind, width)."""
    key = (kind, dim)
    if key not in _cases:
        n = N_APPENDED
        rng = np.random.default_rng(3100 + dim + (0 if kind == "nonneg" else 1))
        data = rng.random((n, dim), dtype=f32) if kind == "nonneg" else rng.standard_normal((n, dim)).astype(f32)
        pins = np.array([0, 63, 255, 256, 2047, 2048, EDGE - 1, EDGE, EDGE + 64 * W - 1, EDGE + 64 * W, N_FIRST - 1, N_FIRST, n - 38, n - 37, n - 1])
        q_rows = np.sort(np.concatenate([pins, rng.integers(0, n, 256 - len(pins))]))
        noise = f32(0.03) if kind == "nonneg" else f32(0.3)
        queries = (data[q_rows] + noise * rng.standard_normal((256, dim)).astype(f32)).astype(f32)
        _cases[key] = {"data": data, "queries": queries, "want": {}}
    return _cases[key]


def wanted(oracle, cs, metric, n, nq):
    if (metric, n) not in cs["want"]:
        m = O.IP if metric == "ip" else O.COS
        rows = cs["data"][:n]
        cs["want"][(metric, n)] = oracle_for_every_query(lambda qi: oracle.canonical_topk(cs["queries"][qi], rows, K, m), 256)
    return cs["want"][(metric, n)][:nq]


# (kind, columns, metric, sq7): SQ8 and SQ7 codes, IP and cosine, six slabs and two (two slabs: seven of a step's sixteen fragments are held)
FORMS = [("gauss", 768, "ip", 0), ("gauss", 768, "cosine", None), ("nonneg", 768, "ip", 1), ("gauss", 256, "ip", 0), ("nonneg", 256, "ip", 1)]


@pytest.mark.parametrize("kind,dim,metric,sq7", FORMS)
def test_one_tile_per_workgroup_then_append(L, W, oracle, kind, dim, metric, sq7):
    """One tile per workgroup and three per workgroup, then — after an append — one stage with a ragged last tile.
    256 / 200 / 130 queries: every wave live; a dead wave and a dead 16-query block; a block with two live lanes."""
    cs = case(W, kind, dim)
    n = N_APPENDED
    idx = new_index(L, cs["data"][:N_FIRST])
    for nq in (256, 130):
        r = both_forms(idx, cs["queries"][:nq], metric, sq7, (kind, dim, metric, "first", nq))
        assert_exact(wanted(oracle, cs, metric, N_FIRST, nq), *r[:3], (kind, dim, metric, "first", nq))
    idx.write(cs["data"][N_FIRST:])
    idx.finalize()
    for nq in (256, 200, 130):
        r = both_forms(idx, cs["queries"][:nq], metric, sq7, (kind, dim, metric, "appended", nq))
        assert_exact(wanted(oracle, cs, metric, n, nq), *r[:3], (kind, dim, metric, "appended", nq))


@pytest.mark.parametrize("kind,dim,metric,sq7", FORMS)
def test_workgroups_with_one_tile_beside_workgroups_with_two(L, W, oracle, kind, dim, metric, sq7):
    """`set_plan(4864, 2, 16384)` on 65,536 rows (module docstring): stages of 304 and 416 tiles on 256 workgroups."""
    cs = case(W, kind, dim)
    idx = new_index(L, cs["data"][:N_FIRST], plan=(4864, 2, 16384))
    for nq in (256, 130):
        tag = (kind, dim, metric, "one beside two", nq)
        r = both_forms(idx, cs["queries"][:nq], metric, sq7, tag)
        assert r[3]["scan_launches"] == 5, (tag, r[3])          # [0, 4864) [.., 9728) [.., 19456) [.., 38912) [.., 65536)
        assert_exact(wanted(oracle, cs, metric, N_FIRST, nq), *r[:3], tag)


def test_massive_ties_overflow_a_private_segment_behind_the_barrier_and_in_the_drain(L, W, oracle):
    """One row, duplicated into whole tiles of the appended shard's single stage (1,505 tiles; workgroup b has tiles b, b + W, ...):
    tiles 223, 479, 735 and 1503 — the first, two middle and the LAST (full) tile of workgroup 223 — and tiles 224, 480, 736, 992, 1248 and
    the ragged 1504 — the first ... last tile of workgroup 224.  Every tie tile gives each lane of the duplicate's query 16 passing keys
    (the ragged one up to 16), a private segment holds 32: from the third tie tile on the keys go through the overflow branch of the epilogue
    (count / candidate addresses formed on the spot) — behind a barrier and the held MFMAs for the middle tiles, after the loop exit for the
    last ones.  All duplicates tie at the best score: the answer is the ten lowest of their rows."""
    dim, nq, n = 768, 130, N_APPENDED
    tiles = (n + 63) // 64
    assert tiles == 1505 and (tiles - 1) % W == 224 and n - 64 * (tiles - 1) == 37
    tie_tiles = [223, 223 + W, 223 + 2 * W, 1503, 224, 224 + W, 224 + 2 * W, 224 + 3 * W, 224 + 4 * W, 1504]
    rng = np.random.default_rng(3111)
    data = rng.standard_normal((n, dim)).astype(f32)
    dup = (f32(1.5) * rng.standard_normal(dim)).astype(f32)
    for t in tie_tiles:
        data[64 * t: min(n, 64 * t + 64)] = dup
    queries = rng.standard_normal((nq, dim)).astype(f32)
    queries[7] = dup
    idx = new_index(L, data)
    r16 = both_forms(idx, queries, "ip", 0, "ties")
    want = oracle_for_every_query(lambda qi: oracle.canonical_topk(queries[qi], data, K, O.IP), nq)
    assert_exact(want, *r16[:3], "ties")
    assert [int(x) for x in r16[0][7]] == list(range(64 * 223, 64 * 223 + 10)), r16[0][7]


def test_planted_rows_of_the_straddling_tiles(L, W, oracle):
    """Planted neighbours on the 768-column form: one pass of the sweep asks for every group of the shard once, so every row of the shard's
    last tile and of each workgroup's first and last tile of every stage — the tiles whose MFMAs straddle a barrier or the loop exit — is
    demanded at some query slot (asserted from the coverage before any GPU call)."""
    n, nq = N_APPENDED, 256
    data, centres = P.make_float_shard("gauss", n, 768, 4768)
    M = P.max_centre_gram(centres)
    assert P.separation_gap("gauss", "ip", M) >= P.MIN_GAP, M
    sweep, cov = P.Sweep(n, nq), P.Coverage(n, nq, 64, W)
    cov.add(sweep, 0)
    assert cov.a() == 1.0                                   # every row, hence every row of the tiles named above
    form = O.IPFORM_BATCH8
    planted = P.planted_answers(n, K, lambda g, local: oracle.canonical_topk(centres[g], data[P.G * g + local], K, O.IP, form))
    for g in (0, P.n_groups(n) - 1, EDGE // P.G):           # the construction itself, against the full-shard oracle
        P.check_construction(planted, g, *oracle.canonical_topk(centres[g], data, K, O.IP))
    idx = new_index(L, data)
    for bi, groups in enumerate(sweep.pass_batches(0)):
        q = np.ascontiguousarray(centres[groups])
        r16 = search(idx, q, "ip", 1, 0)
        lp = int(r16[3]["last_plan"])
        assert lp & PLAN_M16 and (lp >> 16) & 0xff == 0x81 and r16[3]["fallback_queries"] == 0, (bi, hex(lp), r16[3])
        bad = P.mismatches(planted, groups, *r16[:3], n)
        assert bad.size == 0, (bi, [(int(s), int(groups[s]), r16[0][s], planted.ids[groups[s]]) for s in bad[:P.MAX_DIAGNOSED]])
