"""`-m gpu` planted-neighbour sweeps: every row of a shard is demanded as a true neighbour, at every query slot and at every workgroup
residue of each scan tiling, by construction (tests/planted_common.py; the properties of the construction itself are in
tests/test_planted_design.py).

The scan kernels are hand-written maps from (row in tile, query slot, wave, lane, workgroup, stage) to an MFMA accumulator and a
key-emission slot.  The other GPU files check them end to end where random data happens to put a true neighbour: 2,560 (row, query)
pairs of the 16,384 accumulator positions of one k_scan_qs tile.  Here the exact top-10 of query g is rows [10 g, 10 g + 10) — proved
on the CPU from the centre Gram matrix before the shard goes to the device —, and a sweep walks the groups through the slots so that
(a) every row, (b) every (slot, row mod 256) pair and (c) every (slot, tile mod workgroups) pair is demanded.  A fragment map that is
wrong for one lane group, an epilogue that loses one 16-row block, a segment index that is wrong for one (workgroup, query) pair or a
stage that skips its ragged last tile loses a planted row, and the failure names the row, its slot, tile and stage.

Every batch is profiled and pinned to the path the case is about (`last_plan`, include/lynse_hip.h) with `fallback_queries == 0`; the
constants are those of test_gpu_qs16_scan.py, test_gpu_sq7_scan.py, test_gpu_i8c_hostile.py, test_gpu_qh.py and
test_gpu_binary_widths.py.  Ids and f32 distance bits are compared exactly.  The runs of a case (the A/B forms of one path) must agree
bit for bit on every batch.  When a query disagrees, the full-shard oracle is run for that query (at most 8 per case): "the kernel
lost row r" is a finding about the library, "the construction is wrong" a bug of this test.  32 fixed queries per case are compared
with the full-shard oracle whatever the sweep says.  Knobs are read per call by the library and restored in a `finally`.
"""
import gc
import os
import time

import numpy as np
import pytest

import oracle as O
import planted_common as P
from conftest import oracle_for_every_query

pytestmark = pytest.mark.gpu
f32 = np.float32

PLAN_I8C, PLAN_SMALL, PLAN_FUSED, PLAN_I8C_STARTED = 4, 16, 32, 64
PLAN_SQ7, PLAN_M16 = 1 << 26, 1 << 27
N1 = 327_680 + 37       # the int8 query-stationary plan with a ragged last tile (test_gpu_qs16_scan.py); row 262,144 is a stage boundary
N2 = 70_003
N3 = 262_144 + 37       # the <= 32-query int8 tiling starts at 262,144 rows
STAGE_EDGES = {N1: (262_144,)}
METRIC = {"ip": O.IP, "l2": O.L2, "cosine": O.COS, "hamming": O.HAMMING}


@pytest.fixture(scope="module")
def L():
    import lynsedb_amd as L_

    assert L_._lib.device_count() >= 1
    return L_


class Run:
    """One way to answer the batches of a case: knobs, and what `last_plan` must say."""

    def __init__(self, label, env=None, tiling=None, not_tiling=None, on=0, off=0, fused=None):
        self.label, self.env, self.tiling, self.not_tiling, self.on, self.off, self.fused = label, env or {}, tiling, not_tiling, on, off, fused


class Case:
    def __init__(self, name, shard, metric, nq, T, runs, wmul=1, k=P.G, masked=False, max_passes=None, matrix_path=False):
        self.name, self.shard, self.metric, self.nq, self.T, self.runs, self.wmul = name, shard, metric, nq, T, runs, wmul
        self.k, self.masked, self.max_passes, self.matrix_path = k, masked, max_passes, matrix_path
        self.m16_pair = [r.label for r in runs] == ["m16", "m32"]


def both_m16(sq7=None):
    """The 16x16x64 and the 32x32x32 form of k_scan_qs; sq7 = 1 / 0: the stages read the 7-bit / the 8-bit codes (None: cosine, no choice)."""
    env = {} if sq7 is None else {"LYNSE_HIP_SQ7": str(sq7)}
    on, off = (PLAN_SQ7, 0) if sq7 == 1 else (0, PLAN_SQ7)
    return [Run("m16", dict(env, LYNSE_HIP_QS_M16="1"), tiling=0x81, on=PLAN_I8C | PLAN_M16 | on, off=off),
            Run("m32", dict(env, LYNSE_HIP_QS_M16="0"), tiling=0x81, on=PLAN_I8C | on, off=PLAN_M16 | off)]


GAUSS768 = ("gauss", N1, 768)
CASES = [
    # 1, 2: k_scan_qs over int8 codes, both MFMA shapes; 200 queries: a dead wave and a dead 16-query block, 130: a block with two live lanes
    Case("qs-ip-768-q256", GAUSS768, "ip", 256, 64, both_m16(0)),
    Case("qs-ip-768-q200", GAUSS768, "ip", 200, 64, both_m16(0)[:1]),
    Case("qs-ip-768-q130", GAUSS768, "ip", 130, 64, both_m16(0)[:1]),
    # 4: cosine reads the unit-row code set
    Case("qs-cos-768-q256", GAUSS768, "cosine", 256, 64, both_m16()),
    # 7: squared L2 on the plain codes: k_scan_qs<MET = 1>, and the <4,2,2,4> tile of k_scan_h16 with LYNSE_HIP_QS=0
    Case("qs-l2-768-q256", GAUSS768, "l2", 256, 64, [Run("qs", tiling=0x81, on=PLAN_I8C), Run("h16", {"LYNSE_HIP_QS": "0"}, tiling=0x42, on=PLAN_I8C)]),
    # 8: the row bitmask clears row 10 g + (g mod 10) of every group; k = 9: a masked row that comes back fails
    Case("qs-masked-768-q130", GAUSS768, "ip", 130, 64,
         [Run("qs", {"LYNSE_HIP_FILTER_STRATEGY": "2"}, tiling=0x81, on=PLAN_I8C | PLAN_I8C_STARTED),
          Run("dense", {"LYNSE_HIP_FILTER_STRATEGY": "2", "LYNSE_HIP_QS_MASKED": "0"}, tiling=0x24, on=PLAN_I8C | PLAN_I8C_STARTED)], k=9, masked=True),
    # 3: non-negative rows on the 7-bit copy of the codes
    Case("qs-sq7-768-q256", ("nonneg", N1, 768), "ip", 256, 64, both_m16(1)),
    # 5: the other widths of the 16x16x64 form; 6: 1,024 columns run 32-row tiles on the 32x32x32 form
    Case("qs-ip-256-q256", ("gauss", N1, 256), "ip", 256, 64, both_m16(0)),
    Case("qs-ip-512-q256", ("gauss", N1, 512), "ip", 256, 64, both_m16(0)),
    Case("qs-ip-640-q256", ("gauss", N1, 640), "ip", 256, 64, both_m16(0)),
    Case("qs-ip-1024-q256", ("gauss", N1, 1024), "ip", 256, 32, [Run("qs", tiling=0x81, on=PLAN_I8C, off=PLAN_M16)]),
    # 9: the mid tilings of k_scan_h16 over the codes; 10: its <= 32-query tiling
    Case("mid-ip-256-q40", ("gauss", N2, 256), "ip", 40, 128, [Run("mid64", tiling=0x14, on=PLAN_I8C)], wmul=2),
    # (65 .. 128 queries over whole 128-column slabs go to k_scan_qs by default — qs_mid, lynse_hip.hip —: LYNSE_HIP_QS_MID=0 is the 256 x 128 tile)
    Case("mid-ip-256-q100", ("gauss", N2, 256), "ip", 100, 256,
         [Run("mid128", {"LYNSE_HIP_QS_MID": "0"}, tiling=0x24, on=PLAN_I8C, off=PLAN_M16), Run("qs", tiling=0x81, on=PLAN_I8C)]),
    Case("small-ip-256-q32", ("gauss", N3, 256), "ip", 32, 128, [Run("small", tiling=0x14, on=PLAN_I8C | PLAN_SMALL)], wmul=2),
    # 11: the float path of k_scan_h16: the 256 x 256 tiles <4,2,2,4> (L2) and <2,4,4,2> (IP; 60,003 rows are under the int8 pass's 65,536) and
    # the 128 x 32 tile of <= 32 queries (under 262,144 rows those stay on the float pass) — the tilings the pipeline reports for these shapes
    Case("h16-l2-200-q256", ("gauss", N2, 200), "l2", 256, 256, [Run("h16", tiling=0x42, off=PLAN_I8C)]),
    Case("h16-l2-200-q32", ("gauss", N2, 200), "l2", 32, 128, [Run("h16", tiling=0x14, on=PLAN_SMALL, off=PLAN_I8C)], wmul=2),
    Case("h16-ip-200-q256", ("gauss", 60_003, 200), "ip", 256, 256, [Run("h16", tiling=0x24, off=PLAN_I8C)]),
    Case("h16-ip-200-q32", ("gauss", 60_003, 200), "ip", 32, 128, [Run("h16", tiling=0x14, on=PLAN_SMALL, off=PLAN_I8C)], wmul=2),
    # 13: the fused few-query search and the staged pipeline
    Case("fused-ip-96-q4", ("gauss", 20_003, 96), "ip", 4, 64, [Run("fused", on=PLAN_FUSED), Run("staged", off=PLAN_FUSED, fused=False)]),
]
# 12: k_scan_qh (64-row tiles, two workgroups per CU) and the same batches on k_scan_h16
for _dim in (128, 64):
    for _metric in ("ip", "l2"):
        for _nq in (256, 40):
            CASES.append(Case(f"qh-{_metric}-{_dim}-q{_nq}", ("gauss", N2, _dim), _metric, _nq, 64,
                              [Run("qh", tiling=0x82), Run("h16", {"LYNSE_HIP_QH": "0"}, not_tiling=0x82)], wmul=2))
# 14: Hamming.  1,024-bit rows, 256 queries: the FP4 form of k_scan_qs, and k_scan_h16 with LYNSE_HIP_QS_F4=0; 40 queries: the popcount rows
# kernel (256-row blocks, eight workgroups per CU; the popcount scans record no plan: nothing to pin).  512 bits: two slabs, k_scan_qs; 200 bits:
# one slab, the 256 x 256 tile of k_scan_h16.  Every run equals the planted answers bit for bit, hence each other.
CASES += [
    Case("ham-1024-q256", ("binary", N2, 1024), "hamming", 256, 64, [Run("f4", tiling=0x81, on=PLAN_I8C), Run("h16", {"LYNSE_HIP_QS_F4": "0"}, tiling=0x24, on=PLAN_I8C)], matrix_path=True),
    Case("ham-1024-q40", ("binary", N2, 1024), "hamming", 40, 256, [Run("popcount")], wmul=8),
    Case("ham-512-q130", ("binary", N2, 512), "hamming", 130, 64, [Run("f4", tiling=0x81, on=PLAN_I8C)], matrix_path=True),
    Case("ham-200-q130", ("binary", N2, 200), "hamming", 130, 256, [Run("matrix", tiling=0x24, on=PLAN_I8C)], matrix_path=True),
]


# ---- one shard per (kind, n, dim); at most one of the 327,717-row shards (1 GB at 768 columns) is alive at a time
_shards = {}


def get_shard(L, key):
    kind, n, dim = key
    if key in _shards:
        return _shards[key]
    if n >= 200_000:
        for other in [o for o in _shards if o[1] >= 200_000]:
            del _shards[other]
        gc.collect()
    sh = {"planted": {}, "full": {}, "n": n}
    if kind == "binary":
        sh["data"], sh["centres"] = P.make_binary_shard(n, dim, 4100)
        sh["min_centre_distance"] = P.min_centre_hamming(sh["centres"], dim)
        sh["gap"] = {"hamming": P.hamming_gap(sh["min_centre_distance"])}
        assert sh["gap"]["hamming"] >= P.MIN_GAP_BITS, (key, sh)          # the inputs meet the condition, before any GPU call
        idx = L.FlatIndex(None, dim)
        idx.write_packed(sh["data"])
    else:
        sh["data"], sh["centres"] = P.make_float_shard(kind, n, dim, 4000 + dim)
        sh["M"] = P.max_centre_gram(sh["centres"])
        sh["gap"] = {m: P.separation_gap(kind, m, sh["M"]) for m in ("ip", "cosine", "l2")}
        assert min(sh["gap"].values()) >= P.MIN_GAP, (key, sh["M"], sh["gap"])
        idx = L.FlatIndex(None, dim)
        idx.write(sh["data"])
    idx.finalize()
    idx.profile_enable(True)
    sh["idx"] = idx
    _shards[key] = sh
    return sh


def subset_of(n):
    """Row 10 g + (g mod 10) of every group is outside the subset -> (dropped[g], member ids u64, bitset words u64)."""
    g = np.arange(P.n_groups(n))
    out = P.G * g + g % P.G
    member = np.ones(n, bool)
    member[out[out < n]] = False
    ids = np.nonzero(member)[0].astype(np.uint64)
    words = np.zeros((n + 63) // 64, np.uint64)
    np.bitwise_or.at(words, (ids // np.uint64(64)).astype(np.int64), np.uint64(1) << (ids % np.uint64(64)))
    return g % P.G, ids, words


def answers(oracle, sh, case):
    """(planted answers of every group, full-shard oracle answers of the fixed groups), once per (shard, metric, k, subset)."""
    key = (case.metric, case.k, case.masked)
    if key in sh["planted"]:
        return sh["planted"][key], sh["full"][key]
    n, data, centres, m, k = sh["n"], sh["data"], sh["centres"], METRIC[case.metric], case.k
    fixed = P.fixed_groups(n)
    if case.metric == "hamming":
        planted = P.planted_answers(n, k, lambda g, local: oracle.canonical_topk_packed(centres[g], data[P.G * g + local], k, m))
        full = oracle_for_every_query(lambda i: oracle.canonical_topk_packed(centres[fixed[i]], data, k, m), len(fixed))
    elif case.masked:
        dropped, ids, sh["words"] = subset_of(n)
        sh["n_live"] = len(ids)
        # a subset search scores every row with the single-row kernels
        planted = P.planted_answers(n, k, lambda g, local: oracle.canonical_topk(centres[g], data[P.G * g + local], k, m, O.IPFORM_SINGLE), dropped)
        full = oracle_for_every_query(lambda i: oracle.canonical_topk_filtered(centres[fixed[i]], data, k, m, ids), len(fixed))
    else:
        # the inner-product form of a shard of >= 4,096 rows is the batch-8 kernel (the oracle's own rule, applied to the SHARD's size)
        form = O.IPFORM_BATCH8 if n >= 4096 else O.IPFORM_SINGLE
        planted = P.planted_answers(n, k, lambda g, local: oracle.canonical_topk(centres[g], data[P.G * g + local], k, m, form))
        full = oracle_for_every_query(lambda i: oracle.canonical_topk(centres[fixed[i]], data, k, m), len(fixed))
    full = dict(zip(fixed, full))
    for g in fixed:                      # raises ConstructionError: a bug of this test, before any kernel is asked
        P.check_construction(planted, g, *full[g])
    sh["planted"][key], sh["full"][key] = planted, full
    return planted, full


def search(sh, case, run, queries):
    """One profiled blocking batch under the run's knobs -> (rows, dists, counts, profile)."""
    idx = sh["idx"]
    old = {name: os.environ.get(name) for name in run.env}
    os.environ.update(run.env)
    if run.fused is not None:
        idx.set_fused_search(run.fused)
    try:
        idx.profile_get(reset=True)
        if case.metric == "hamming":
            r, d, c = idx.search_packed_arrays(queries, case.k, "hamming")
        elif case.masked:
            r, d, c = idx.search_filtered_bitset_batch_arrays(queries, case.k, case.metric, sh["words"])
        else:
            r, d, c = idx.search_batch_arrays(queries, case.k, case.metric)
        return r, d, c, idx.profile_get(reset=True)
    finally:
        if run.fused is not None:
            idx.set_fused_search(True)
        for name, v in old.items():
            if v is None:
                os.environ.pop(name, None)
            else:
                os.environ[name] = v


def check_pins(case, run, p, tag):
    lp = int(p["last_plan"])
    tiling = (lp >> 16) & 0xff
    assert p["fallback_queries"] == 0, (tag, hex(lp), p)
    assert (lp & run.on) == run.on and not (lp & run.off), (tag, hex(lp), hex(run.on), hex(run.off), p)
    if run.tiling is not None:
        assert tiling == run.tiling, (tag, hex(lp), hex(run.tiling), p)
    if run.not_tiling is not None:
        assert tiling != run.not_tiling, (tag, hex(lp), p)
    return lp


def full_oracle_of(oracle, sh, case, g):
    m = METRIC[case.metric]
    if case.metric == "hamming":
        return oracle.canonical_topk_packed(sh["centres"][g], sh["data"], case.k, m)
    if case.masked:
        return oracle.canonical_topk_filtered(sh["centres"][g], sh["data"], case.k, m, subset_of(sh["n"])[1])
    return oracle.canonical_topk(sh["centres"][g], sh["data"], case.k, m)


def fail_with_diagnosis(oracle, sh, case, W, tag, groups, slots, r, d, c, full=None):
    lines = []
    for s in list(slots)[:P.MAX_DIAGNOSED]:
        g = int(groups[s])
        f_ids, f_d = full[g] if full is not None else full_oracle_of(oracle, sh, case, g)
        planted = sh["planted"][(case.metric, case.k, case.masked)]
        lines.append(P.diagnose(planted, g, int(s), r[s], d[s], c[s], f_ids, f_d, case.T, W, STAGE_EDGES.get(sh["n"], ())))
    pytest.fail(f"{tag}: {len(slots)} queries disagree with the planted answers\n" + "\n".join(lines))


def sweep_case(L, oracle, case):
    import torch

    t0 = time.perf_counter()
    sh = get_shard(L, case.shard)
    n, nq, idx = sh["n"], case.nq, sh["idx"]
    planted, full = answers(oracle, sh, case)
    n_live = sh.get("n_live", n) if case.masked else n
    # conditions (a) - (c) for the device's own workgroup count: as many passes as they need
    W = case.wmul * torch.cuda.get_device_properties(0).multi_processor_count
    passes, cov = P.passes_needed(n, nq, case.T, W)
    if case.max_passes is not None and case.max_passes < passes:
        passes, sweep, cov = case.max_passes, P.Sweep(n, nq), P.Coverage(n, nq, case.T, W)
        for p in range(passes):
            cov.add(sweep, p)
    assert cov.a() == 1.0 and cov.b() == 1.0, (case.name, cov.a(), cov.b())
    batches = P.Sweep(n, nq).batches(passes)
    fixed = set(full)
    got = {}
    plans = {}
    for bi, groups in enumerate(batches):
        queries = sh["centres"][groups]
        first = None
        for run in case.runs:
            tag = (case.name, run.label, "batch", bi)
            r, d, c, p = search(sh, case, run, queries)
            lp = check_pins(case, run, p, tag)
            plans.setdefault(run.label, set()).add(lp)
            if case.matrix_path:
                assert idx.coarse_state()["bpm_rows"] == n, tag          # the +-1 copy was built: the matrix path ran
            bad = P.mismatches(planted, groups, r, d, c, n_live)
            if bad.size:
                fail_with_diagnosis(oracle, sh, case, W, tag, groups, bad, r, d, c)
            if first is None:
                first = (r, d, c, p, lp)
                for s in np.nonzero(np.isin(groups, list(fixed)))[0]:
                    got[int(groups[s])] = (int(s), r[s].copy(), d[s].copy(), int(c[s]))
            else:
                assert np.array_equal(first[0], r) and np.array_equal(first[1].view(np.uint32), d.view(np.uint32)) and np.array_equal(first[2], c), tag
                if case.m16_pair:      # identical key sets: the same rows were rescored; the same plan but for the MFMA shape
                    assert first[3]["pool_entries"] == p["pool_entries"], (tag, first[3], p)
                    assert (first[4] ^ lp) == PLAN_M16, (tag, hex(first[4]), hex(lp))
    # the fixed queries against the full-shard oracle, every entry (the ragged group's rows from outside the group among them)
    assert set(got) == fixed, (case.name, sorted(fixed - set(got)))
    for g, (s, r, d, c) in got.items():
        f_ids, f_d = full[g]
        if not (c == len(f_ids) and np.array_equal(r[:c].astype(np.uint64), f_ids.astype(np.uint64)) and np.array_equal(d[:c].view(np.uint32), f_d.view(np.uint32))):
            fail_with_diagnosis(oracle, sh, case, W, (case.name, "fixed query"), {s: g}, [s], {s: r}, {s: d}, {s: c}, full)
    wall = time.perf_counter() - t0
    gap = sh["gap"][case.metric]
    print(f"\nplanted sweep {case.name}: {len(batches)} batches x {len(case.runs)} runs of {nq} queries in {passes} passes, rows demanded "
          f"{int(cov.row_hits.sum())} (every row >= {int(cov.row_hits.min())} times), coverage a {cov.a():.3f} b {cov.b():.3f} c {cov.c():.3f} "
          f"(T {case.T}, W {cov.W}), gap {gap:.3f}" + (f" (M {sh['M']:.3f})" if "M" in sh else f" (centres >= {sh['min_centre_distance']} bits apart)") +
          f", plans {({k: sorted(hex(x) for x in v) for k, v in plans.items()})}, {wall:.2f} s")
    assert cov.c() == 1.0 or case.max_passes is not None, (case.name, cov.c())
    return wall


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_planted_sweep(L, oracle, case):
    sweep_case(L, oracle, case)
