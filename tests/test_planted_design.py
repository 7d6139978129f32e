"""The properties of the planted-neighbour construction itself (tests/planted_common.py), on the CPU: what tests/test_gpu_planted_sweeps.py
relies on when it says that the top-10 of query g is rows [10 g, 10 g + 10) and that its batches demand every row at every query slot of
every workgroup residue.  The workgroup count is taken as 256 here (times the workgroups per CU of the tiling); the GPU file repeats
condition (c) with the device's own.
"""
import math

import numpy as np
import pytest

import oracle as O
import planted_common as P
import test_gpu_planted_sweeps as S

f32 = np.float32
CUS = 256
SHAPES = sorted({(c.shard[1], c.nq, c.T, c.wmul * CUS) for c in S.CASES})


def test_the_assignment_of_the_256_query_sweep_is_the_documented_one():
    sw = P.Sweep(S.N1, 256)
    assert (sw.groups, sw.B, sw.main, sw.a, sw.c, sw.d, sw.batches_per_pass) == (32_772, 128, 32_768, 7, 37, 820, 129)
    b, s = np.meshgrid(np.arange(128), np.arange(256), indexing="ij")
    for p in (0, 1):
        assert np.array_equal(sw.pass_batches(p)[:128], (7 * b + 128 * 37 * s + 820 * p) % 32_768)
    one = P.Coverage(S.N1, 256, 64, 256).add(sw, 0)
    assert one.a() == 1.0 and one.b() == 1.0 and 0.54 < one.c() < 0.56          # one pass: every row, every (slot, row mod 256), 54.9 % of (c)
    passes, two = P.passes_needed(S.N1, 256, 64, 256)
    assert passes == 2 and two.complete()


@pytest.mark.parametrize("n,nq,T,W", SHAPES)
def test_coverage_of_every_sweep(n, nq, T, W):
    sw = P.Sweep(n, nq)
    passes, cov = P.passes_needed(n, nq, T, W)
    # every pass is a bijection: each group exactly once among the first B batches and the groups beyond B nq, and every batch is full
    for p in (0, passes - 1):
        pb = sw.pass_batches(p)
        assert pb.shape == (sw.batches_per_pass, nq) and pb.min() >= 0 and pb.max() < sw.groups
        assert np.array_equal(np.sort(pb[:sw.B].ravel()), np.arange(sw.main))
        if sw.groups > sw.main:
            assert set(range(sw.main, sw.groups)) <= set(pb[sw.B].tolist()) and len(set(pb[sw.B].tolist())) == nq
    assert cov.a() == 1.0 and cov.row_hits.min() >= passes                         # (a)
    assert cov.b() == 1.0                                                           # (b)
    assert cov.c() == 1.0 and cov.W == min(W, (n + T - 1) // T)                     # (c)
    assert cov.min_regions >= P.regions_floor(n, nq), (cov.min_regions, P.regions_floor(n, nq))          # (d)
    if cov.min_regions_tail is not None:
        assert cov.min_regions_tail >= P.tail_regions_floor(n, nq), (cov.min_regions_tail, P.tail_regions_floor(n, nq))
    edge = [0, n - 1] + ([262_143, 262_144] if n > 262_144 else [])                 # (e)
    assert (cov.row_hits[edge] > 0).all()
    if n > 262_144:
        assert 262_144 // P.G * P.G == 262_140 and 262_144 // P.G in P.fixed_groups(n)     # one group straddles the stage boundary
    print(f"(n, nq, T, W) = {(n, nq, T, W)}: {passes} passes, {passes * sw.batches_per_pass} batches, regions per batch >= {cov.min_regions}")


def test_fixed_groups():
    for n in sorted({c.shard[1] for c in S.CASES}):
        fixed = P.fixed_groups(n)
        assert len(fixed) == len(set(fixed)) == P.N_FIXED and fixed[0] == 0 and fixed[-1] == P.n_groups(n) - 1
        assert P.group_len(n, fixed[-1]) == n % P.G != 0                            # every shard of the sweeps has a ragged last group


@pytest.mark.parametrize("kind,n,dim", [("gauss", S.N2, 64), ("gauss", 20_003, 96), ("nonneg", 20_003, 256)])
def test_float_shard_and_its_separation(oracle, kind, n, dim):
    data, centres = P.make_float_shard(kind, n, dim, 4000 + dim)
    again, _ = P.make_float_shard(kind, n, dim, 4000 + dim, chunk_groups=1024)
    assert np.array_equal(data, again)
    ng = P.n_groups(n)
    assert data.shape == (n, dim) and centres.shape == (ng, dim) and data.dtype == centres.dtype == f32
    assert np.allclose(np.linalg.norm(centres.astype(np.float64), axis=1), 1.0, atol=1e-6)
    off = data.astype(np.float64) - np.repeat(centres.astype(np.float64), P.G, axis=0)[:n]
    assert np.allclose(np.linalg.norm(off, axis=1), P.NOISE, atol=1e-6)
    if kind == "nonneg":
        assert data.min() >= 0.0 and ((centres > 0).sum(axis=1) == P.NONNEG_SUPPORT).all()
    M = P.max_centre_gram(centres, block=1000)
    g64 = centres.astype(np.float64) @ centres.astype(np.float64).T
    np.fill_diagonal(g64, -np.inf)
    assert abs(M - g64.max()) < 1e-6                                                # the chunked GEMM sees every pair
    gaps = {m: P.separation_gap(kind, m, M) for m in ("ip", "cosine", "l2")}
    print(f"{kind} {n} x {dim}: M {M:.3f}, gaps {gaps}")
    assert min(gaps.values()) >= P.MIN_GAP, (M, gaps)
    # the bounds against the real thing: every out-of-group row of a few hundred queries, in f64
    rows64 = data.astype(np.float64)
    norms = np.linalg.norm(rows64, axis=1)
    for g in list(range(0, ng, max(1, ng // 200))) + [ng - 1]:
        q = centres[g].astype(np.float64)
        ip = rows64 @ q
        l2 = ((rows64 - q) ** 2).sum(axis=1)
        cos = ip / norms
        inside = np.zeros(n, bool)
        inside[P.G * g:P.G * g + P.G] = True
        lo = 1.0 if kind == "nonneg" else 1.0 - P.NOISE
        assert ip[inside].min() >= lo - 1e-6 and ip[~inside].max() <= M + P.NOISE + 1e-6
        assert cos[inside].min() >= 1.0 - P.NOISE and cos[~inside].max() <= (M + P.NOISE) / (1.0 - P.NOISE) + 1e-6
        assert l2[inside].max() <= P.NOISE ** 2 + 1e-6 and l2[~inside].min() >= (math.sqrt(2.0 - 2.0 * M) - P.NOISE) ** 2 - 1e-6
    # the planted answers are the full-shard oracle's, for every metric, at the fixed groups (the ragged last one among them)
    for name, m in (("ip", O.IP), ("l2", O.L2), ("cosine", O.COS)):
        form = O.IPFORM_BATCH8 if n >= 4096 else O.IPFORM_SINGLE
        planted = P.planted_answers(n, P.G, lambda g, local: oracle.canonical_topk(centres[g], data[P.G * g + local], P.G, m, form))
        assert planted.known[-1] == n % P.G and (planted.known[:-1] == P.G).all()
        for g in P.fixed_groups(n):
            P.check_construction(planted, g, *oracle.canonical_topk(centres[g], data, P.G, m))
    # ... and a wrong one is reported as a bug of the construction, never as a lost row
    planted.ids[0, 0] += 1
    with pytest.raises(P.ConstructionError, match="the construction is wrong"):
        P.check_construction(planted, 0, *oracle.canonical_topk(centres[0], data, P.G, O.COS))


@pytest.mark.parametrize("bits", [1024, 512, 200])
def test_binary_shard_and_its_separation(oracle, bits):
    n = S.N2
    words, centres = P.make_binary_shard(n, bits, 4100)
    ng, W = P.n_groups(n), (bits + 63) // 64
    assert words.shape == (n, W) and centres.shape == (ng, W) and words.dtype == np.uint64
    if bits % 64:
        assert not (words[:, -1] >> np.uint64(bits % 64)).any()                   # tail bits are zero
    dist = np.unpackbits((words ^ np.repeat(centres, P.G, axis=0)[:n]).view(np.uint8), axis=1).sum(axis=1)
    assert np.array_equal(dist, (np.arange(n) % P.G))                               # row j of a group: exactly j bits from its centre
    between = np.unpackbits((words[70:80] ^ words[79]).view(np.uint8), axis=1).sum(axis=1)
    assert np.array_equal(between, 9 - np.arange(10))                               # ... and the flipped positions are nested
    d = P.min_centre_hamming(centres, bits)
    sample = np.unpackbits((centres[:500, None, :] ^ centres[None, :500, :]).view(np.uint8), axis=2).sum(axis=2)
    np.fill_diagonal(sample, bits)
    assert d <= sample.min()
    print(f"binary {n} x {bits}: centres >= {d} bits apart, gap {P.hamming_gap(d)} bits")
    assert P.hamming_gap(d) >= P.MIN_GAP_BITS
    planted = P.planted_answers(n, P.G, lambda g, local: oracle.canonical_topk_packed(centres[g], words[P.G * g + local], P.G, O.HAMMING))
    for g in P.fixed_groups(n):
        P.check_construction(planted, g, *oracle.canonical_topk_packed(centres[g], words, P.G, O.HAMMING))
        m = int(planted.known[g])
        assert np.array_equal(planted.ids[g, :m], P.G * g + np.arange(m)) and np.array_equal(planted.dist[g, :m], np.arange(m, dtype=f32))


def test_mismatches_and_diagnosis_tell_a_lost_row_from_a_wrong_construction(oracle):
    n, dim = 20_003, 96
    data, centres = P.make_float_shard("gauss", n, dim, 4000 + dim)
    planted = P.planted_answers(n, P.G, lambda g, local: oracle.canonical_topk(centres[g], data[P.G * g + local], P.G, O.IP, O.IPFORM_BATCH8))
    groups = P.Sweep(n, 4).pass_batches(0)[17]
    full = [oracle.canonical_topk(centres[g], data, P.G, O.IP) for g in groups]
    rows = np.stack([f[0] for f in full]).astype(np.uint64)
    dists = np.stack([f[1] for f in full])
    counts = np.full(4, P.G, np.uint32)
    assert P.mismatches(planted, groups, rows, dists, counts, n).size == 0
    lost = int(rows[2, 3])
    rows[2, 3:-1], dists[2, 3:-1] = rows[2, 4:].copy(), dists[2, 4:].copy()        # a kernel that lost one row: the others move up, a stranger follows
    rows[2, -1], dists[2, -1] = (lost + 5000) % n, f32(0.3)
    dists[1, 0] = np.nextafter(dists[1, 0], f32(2))                                 # one distance off by one ulp
    counts[3] = 9
    assert P.mismatches(planted, groups, rows, dists, counts, n).tolist() == [1, 2, 3]
    msg = P.diagnose(planted, int(groups[2]), 2, rows[2], dists[2], counts[2], *full[2], 64, 256, (8192,))
    assert f"the kernel lost row {lost} (slot 2, r mod 256 = {lost % 256}, tile {lost // 64} = workgroup residue {(lost // 64) % 256} of 256, stage {int(lost >= 8192)})" in msg
    assert "another order or with other distance bits" in P.diagnose(planted, int(groups[1]), 1, rows[1], dists[1], counts[1], *full[1], 64, 256)
    planted.ids[groups[2], 0] += 1
    with pytest.raises(P.ConstructionError):
        P.diagnose(planted, int(groups[2]), 2, rows[2], dists[2], counts[2], *full[2], 64, 256)
