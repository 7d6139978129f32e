"""Shared by tests/test_planted_design.py and tests/test_gpu_planted_sweeps.py: shards whose exact top-k is known BY CONSTRUCTION, the
assignment of their queries to the slots of a sequence of batches, the proof that the construction holds for a given shard, and the
comparison of a batch's results with the planted answers.  TEST INFRASTRUCTURE.

The shard.  Rows come in groups of G = 10 consecutive rows; group g is rows [10 g, 10 g + 10) (the last group may be ragged) and has a
unit centre c_g.  Row r of the group is c_g + 0.05 e_r with |e_r| = 1, the query of the group is c_g itself, and k = G.  With M the
largest inner product of two different centres (max_centre_gram), Cauchy-Schwarz gives for the query of group g
    inner product   in-group >= 1 - 0.05 (`gauss`) or >= 1 (`nonneg`: c . e >= 0);   any other row <= M + 0.05
    cosine          in-group >= 0.95 (the angle is at most asin 0.05);                any other row <= (M + 0.05) / 0.95   (|row| >= 0.95)
    squared L2      in-group <= 0.05^2;                                               any other row >= (sqrt(2 - 2 M) - 0.05)^2
so while the gap between the two sides is wide (separation_gap; the tests ask for 0.2, six orders of magnitude above the f32 roundings of
the rows and of any scoring kernel) the exact top-10 of query g IS its group, and its order and f32 distance bits are those of the
oracle run over the ten rows alone.  The binary shard: c_g is random bits, row j of a group is c_g with j fixed distinct bits flipped
(in-group Hamming distances 0 .. 9, all different); any other row is at least (the smallest distance of two centres) - 9 away.

The sweep.  A pass visits every group once, in batches of nq queries; which group sits in which slot of which batch is the bijection
    pass p, batch b in [0, B), slot s in [0, nq)   ->   group (a b + B c s + d p) mod (B nq)        B = groups div nq, gcd(a, B) = gcd(c, nq) = 1
(mod B the group gives b, the quotient gives s).  Within a batch the slots sit B groups apart — all over the shard —, within a slot the
batches of a pass walk through every residue mod B.  The groups beyond B nq (the ragged one among them) go into one more batch per pass,
filled up to nq queries with groups spread over the shard, so every batch of a sweep has the SAME number of queries and runs the same kernels.
"""
import bisect
import math
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

f32, u64 = np.float32, np.uint64
G = 10                       # rows per group = k
NOISE = 0.05                 # |row - centre|
NONNEG_SUPPORT = 96          # non-zero coordinates of a `nonneg` centre
MIN_GAP, MIN_GAP_BITS = 0.2, 20
N_FIXED = 32                 # queries per case that are compared with the full-shard oracle whatever the sweep says
MAX_DIAGNOSED = 8


def host_threads():
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    return max(1, min(16, n))


def pool_map(fn, items):
    with ThreadPoolExecutor(max_workers=host_threads()) as ex:
        return list(ex.map(fn, items))


def n_groups(n):
    return (n + G - 1) // G


def group_len(n, g):
    return min(G, n - G * g)


# ------------------------------------------------------------------------------------------------------------------ the shards

def _unit(x):
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x


def make_float_shard(kind, n, dim, seed, chunk_groups=1024):
    """-> (rows f32[n, dim], centres f32[groups, dim]).  Every chunk of groups has a generator of its own (seed, first group): the shard does
    not depend on how many threads build it."""
    assert kind in ("gauss", "nonneg") and (kind == "gauss" or dim >= NONNEG_SUPPORT)
    ng = n_groups(n)
    data, centres = np.empty((n, dim), f32), np.empty((ng, dim), f32)

    def fill(g0):
        g1 = min(ng, g0 + chunk_groups)
        m = g1 - g0
        rng = np.random.default_rng([seed, g0])
        if kind == "gauss":
            c = _unit(rng.standard_normal((m, dim), dtype=f32))
            e = _unit(rng.standard_normal((m * G, dim), dtype=f32))
        else:
            pick = np.argsort(rng.random((m, dim), dtype=f32), axis=1)[:, :NONNEG_SUPPORT]
            c = np.zeros((m, dim), f32)
            np.put_along_axis(c, pick, f32(1.0 / math.sqrt(NONNEG_SUPPORT)), axis=1)
            e = _unit(np.abs(rng.standard_normal((m * G, dim), dtype=f32)))
        centres[g0:g1] = c
        rows = np.repeat(c, G, axis=0)
        rows += f32(NOISE) * e
        r0, r1 = G * g0, min(n, G * g1)
        data[r0:r1] = rows[:r1 - r0]

    pool_map(fill, range(0, ng, chunk_groups))
    return data, centres


def pack_bits(bits01):
    """u8 0/1 [n, bits] -> u64[n, ceil(bits / 64)], LSB first, tail bits zero."""
    n, bits = bits01.shape
    words = (bits + 63) // 64
    padded = np.zeros((n, words * 64), np.uint8)
    padded[:, :bits] = bits01
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little")).view("<u8").astype(u64).reshape(n, words)


def make_binary_shard(n, bits, seed):
    """-> (rows u64[n, W], centres u64[groups, W]): row j of a group is its centre with the first j of nine bit positions (distinct, fixed per
    group) flipped."""
    ng = n_groups(n)
    rng = np.random.default_rng([seed, bits])
    c = (rng.random((ng, bits), dtype=f32) < 0.5).astype(np.uint8)
    flips = np.argsort(rng.random((ng, bits), dtype=f32), axis=1)[:, :G - 1]          # nine distinct positions per group
    rows = np.repeat(c[:, None, :], G, axis=1)                                          # [groups, 10, bits]
    gi = np.arange(ng)[:, None]
    for j in range(1, G):
        rows[gi, j, flips[:, :j]] ^= 1
    return pack_bits(rows.reshape(ng * G, bits)[:n]), pack_bits(c)


# ------------------------------------------------------------------------------------------------------------------ separation

def max_centre_gram(centres, block=4096):
    """The largest inner product of two DIFFERENT centres, by a chunked f32 GEMM over the upper triangle of the Gram matrix."""
    c = np.ascontiguousarray(centres, f32)
    best = -np.inf
    for i in range(0, len(c), block):
        for j in range(i, len(c), block):
            gram = c[i:i + block] @ c[j:j + block].T
            if i == j:
                np.fill_diagonal(gram, -np.inf)
            best = max(best, float(gram.max()))
    return best


def separation_gap(kind, metric, M):
    """Worst in-group score minus best out-of-group score (similarities), or the reverse (squared L2), from M alone."""
    if metric == "l2":
        return (math.sqrt(max(0.0, 2.0 - 2.0 * M)) - NOISE) ** 2 - NOISE ** 2
    inside = 1.0 if (kind == "nonneg" and metric == "ip") else 1.0 - NOISE
    outside = (M + NOISE) / (1.0 - NOISE) if metric == "cosine" else M + NOISE
    return inside - outside


def min_centre_hamming(centre_words, bits, block=4096):
    """The smallest Hamming distance of two different centres: distance = (bits - <+-1 images>) / 2, exact in f32 below 2^24 bits."""
    b = np.unpackbits(np.ascontiguousarray(centre_words).view(np.uint8), axis=1, bitorder="little")[:, :bits]
    s = np.ascontiguousarray(b.astype(f32) * f32(2) - f32(1))
    return int(round((bits - max_centre_gram(s, block)) / 2))


def hamming_gap(min_centre_distance):
    return (min_centre_distance - (G - 1)) - (G - 1)


# ------------------------------------------------------------------------------------------------------------------ the slot assignment

def _coprime_from(start, m):
    a = start
    while math.gcd(a, m) != 1:
        a += 1
    return a


class Sweep:
    """The batches of a sweep of `nq`-query batches over the groups of an n-row shard (module docstring)."""

    def __init__(self, n, nq):
        self.n, self.nq, self.groups = n, nq, n_groups(n)
        self.B = self.groups // nq
        assert self.B >= 1, "a sweep needs at least one full batch of groups"
        self.main = self.B * nq
        self.a, self.c, self.d = _coprime_from(7, self.B), _coprime_from(37, nq), 820
        self.batches_per_pass = self.B + (1 if self.groups > self.main else 0)

    def pass_batches(self, p):
        """i32[batches_per_pass, nq]: the group of every slot of every batch of pass p."""
        b = np.arange(self.B, dtype=np.int64)[:, None]
        s = np.arange(self.nq, dtype=np.int64)[None, :]
        out = [(self.a * b + self.B * self.c * s + self.d * p) % self.main]
        left = np.arange(self.main, self.groups, dtype=np.int64)
        if left.size:
            fill = self.nq - left.size
            spread = (np.arange(fill, dtype=np.int64) * self.main // max(fill, 1) + 3 * p) % self.main
            out.append(np.roll(np.concatenate([left, spread]), 61 * p)[None, :])
        return np.concatenate(out).astype(np.int32)

    def batches(self, passes):
        return np.concatenate([self.pass_batches(p) for p in range(passes)])


class Coverage:
    """What a set of batches demands of an n-row shard scanned in tiles of T rows by W workgroups (tile t falls to workgroup t mod W)."""

    def __init__(self, n, nq, T, W):
        self.n, self.nq, self.T = n, nq, T
        self.W = min(W, (n + T - 1) // T)            # a shard of fewer tiles than workgroups only has that many residues
        self.row_hits = np.zeros(n, np.int64)
        self.slot_mod256 = np.zeros((nq, 256), bool)
        self.slot_wg = np.zeros((nq, self.W), bool)
        self.min_regions, self.min_regions_tail = None, None

    def add(self, sweep, p):
        """Adds pass p of the sweep."""
        batches = sweep.pass_batches(p)
        nb, nq = batches.shape
        rows = batches.astype(np.int64)[:, :, None] * G + np.arange(G)
        slot = np.broadcast_to(np.arange(nq)[None, :, None], rows.shape)
        live = rows < self.n
        r, s = rows[live], slot[live]
        self.row_hits += np.bincount(r, minlength=self.n)
        self.slot_mod256[s, r % 256] = True
        self.slot_wg[s, (r // self.T) % self.W] = True
        per_batch = [len(np.unique(b // 128)) for b in batches]          # 128 groups = 1,280 rows
        self.min_regions = min(per_batch[:sweep.B] + ([] if self.min_regions is None else [self.min_regions]))
        if nb > sweep.B:
            self.min_regions_tail = min(per_batch[sweep.B:] + ([] if self.min_regions_tail is None else [self.min_regions_tail]))
        return self

    def a(self):
        return float((self.row_hits > 0).mean())

    def b(self):
        return float(self.slot_mod256.mean())

    def c(self):
        return float(self.slot_wg.mean())

    def complete(self):
        return self.a() == 1.0 and self.b() == 1.0 and self.c() == 1.0


def passes_needed(n, nq, T, W, limit=64):
    """The number of passes after which conditions (a), (b) and (c) all hold, and the coverage then."""
    sweep, cov = Sweep(n, nq), Coverage(n, nq, T, W)
    for p in range(limit):
        cov.add(sweep, p)
        if cov.complete():
            return p + 1, cov
    raise AssertionError(f"(n, nq, T, W) = {(n, nq, T, W)}: coverage incomplete after {limit} passes: a {cov.a():.4f} b {cov.b():.4f} c {cov.c():.4f}")


def regions_floor(n, nq):
    """Condition (d): a batch spreads over at least this many 1,280-row regions — 128, or as many as the batch has queries or the shard has
    whole regions.  The one batch per pass that takes the groups beyond B nq holds those (consecutive) groups by necessity: it is held to
    the spread of its fill queries, tail_regions_floor."""
    return min(128, nq, (n_groups(n) // nq * nq) // 128)


def tail_regions_floor(n, nq):
    sweep = Sweep(n, nq)
    return min(regions_floor(n, nq), nq - (sweep.groups - sweep.main))


def fixed_groups(n):
    """The N_FIXED groups whose queries are compared with the full-shard oracle: the first, the last (ragged) one, the one that holds row
    262,144 where the shard has it, the others evenly spread."""
    ng = n_groups(n)
    must = {0, ng - 1}
    if n > 262_144:
        must.add(262_144 // G)
    spread = [int(x) for x in np.linspace(0, ng - 1, 4 * N_FIXED) if int(x) not in must]
    step = len(spread) / (N_FIXED - len(must))
    return sorted(must | {spread[int(i * step)] for i in range(N_FIXED - len(must))})


# ------------------------------------------------------------------------------------------------------------------ expected answers

class Planted:
    """ids i64[groups, k] (global rows, -1 where unknown), dist f32[groups, k], known[groups] = how many leading entries the construction
    gives (fewer than k only for the ragged last group)."""

    def __init__(self, ids, dist, known, k):
        self.ids, self.dist, self.known, self.k = ids, dist, known, k


def planted_answers(n, k, topk_of_group, dropped=None):
    """topk_of_group(g, local_rows) -> the oracle's (local indices, f32 distances) over rows `10 g + local_rows` of the shard.
    dropped[g]: a row of the group (local index) outside the subset, or None."""
    ng = n_groups(n)
    ids, dist, known = np.full((ng, k), -1, np.int64), np.zeros((ng, k), f32), np.zeros(ng, np.int64)

    def run(g0):
        for g in range(g0, min(ng, g0 + 256)):
            local = np.arange(group_len(n, g))
            if dropped is not None:
                local = local[local != dropped[g]]
            e_ids, e_d = topk_of_group(g, local)
            m = len(e_ids)
            assert m == min(k, len(local)), (g, m, len(local))
            ids[g, :m] = G * g + local[e_ids.astype(np.int64)]
            dist[g, :m] = e_d
            known[g] = m

    pool_map(run, range(0, ng, 256))
    return Planted(ids, dist, known, k)


def mismatches(planted, groups, rows, dists, counts, n_live):
    """Slots of one batch whose results differ from the planted answers in count, ids or f32 distance bits.  n_live: rows the search can
    return (the shard, or the subset of a masked search)."""
    k = planted.k
    want_ids, want_d, known = planted.ids[groups], planted.dist[groups], planted.known[groups]
    lead = np.arange(k)[None, :] < known[:, None]
    ok = np.asarray(counts).astype(np.int64) == min(k, n_live)
    ok &= ((np.asarray(rows).astype(np.int64) == want_ids) | ~lead).all(axis=1)
    ok &= ((np.ascontiguousarray(dists).view(np.uint32) == want_d.view(np.uint32)) | ~lead).all(axis=1)
    return np.nonzero(~ok)[0]


class ConstructionError(AssertionError):
    """The planted answer of a query is not what the full-shard oracle says: a bug of the TEST, never of a kernel."""


def check_construction(planted, g, full_ids, full_d):
    m = int(planted.known[g])
    if not (np.array_equal(full_ids[:m].astype(np.int64), planted.ids[g, :m]) and
            np.array_equal(full_d[:m].view(np.uint32), planted.dist[g, :m].view(np.uint32))):
        raise ConstructionError(f"the construction is wrong for group {g}: planted {planted.ids[g, :m]} {planted.dist[g, :m]}, "
                                f"full-shard oracle {full_ids} {full_d}")


def diagnose(planted, g, slot, got_rows, got_d, got_count, full_ids, full_d, T, W, stage_edges=()):
    """One line that tells a kernel failure from a test bug, for a query whose results disagree.  full_*: the full-shard oracle's answer."""
    check_construction(planted, g, full_ids, full_d)                  # raises: "the construction is wrong"
    c = int(got_count)
    got = [int(x) for x in np.asarray(got_rows)[:c]]
    lost = [int(r) for r in full_ids if int(r) not in got]
    where = [f"the kernel lost row {r} (slot {slot}, r mod 256 = {r % 256}, tile {r // T} = workgroup residue {(r // T) % W} of {W}, "
             f"stage {bisect.bisect_right(list(stage_edges), r)})" for r in lost]
    if not where:
        where = [f"every row of the answer came back, in another order or with other distance bits (slot {slot})"]
    return f"group {g}: " + "; ".join(where) + f"; got {got} {np.asarray(got_d)[:c]}, oracle {full_ids} {full_d}"
