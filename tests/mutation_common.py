"""Shared by tests/test_gpu_mutation_paths.py and tests/test_mutation_paths_design.py: the seeded shards, the model of what a shard holds
after an update, a compaction and an append ("the final rows"), the queries planted against a stale derived copy, and the operation lists of
the seeded sequences.  TEST INFRASTRUCTURE; numpy only.

A derived copy (row norms, f16 shadow, packed words, int8 codes) that survived a mutation describes the STALE LAYOUT: the old rows at their old
positions, cut at the new length.  Every case plants three kinds of query against it:
  (a) copies of kept rows whose index shifted under the compaction (row 0 is always dropped, so every index shifts);
  (b) copies of rows that were deleted, or overwritten by the update, and whose old position still lies inside the new length;
  (c) copies of rows appended after the mutation.
The sources of the planted queries are scaled by PLANT_SCALE, so that under the inner product too a planted query's best row is its own source
(centred rows: the other scores scatter around zero).  tests/test_mutation_paths_design.py proves, with the oracle alone, that the stale layout
answers every (a) and (b) query differently from the final rows."""
from dataclasses import dataclass

import numpy as np

f32 = np.float32
PLANT_SCALE = f32(1.5)
N_PLANT = 4   # queries of each kind in a batch
APPEND_INSIDE, APPEND_REGROW = 2_000, 9_000   # an append inside the capacity a compaction freed (or a reserve left) / across a regrow


def round_f16(a):
    """what an F16 shard keeps of f32 rows (round to nearest even), decoded"""
    return np.asarray(a, f32).astype(np.float16).astype(f32)


class RowModel:
    """The rows a shard holds, as read_rows returns them (an F16 shard: the decoded halves)."""

    def __init__(self, dim, f16=False):
        self.dim, self.f16 = dim, f16
        self.rows = np.zeros((0, dim), f32)

    def store(self, a):
        a = np.ascontiguousarray(a, f32)
        return round_f16(a) if self.f16 else a

    def write(self, a):
        self.rows = np.concatenate([self.rows, self.store(a)])

    def update(self, rows, new):
        self.rows = self.rows.copy()
        self.rows[np.asarray(rows, np.int64)] = self.store(new)

    def compact(self, keep):
        self.rows = self.rows[np.asarray(keep, bool)]

    def __len__(self):
        return self.rows.shape[0]


METRIC_IDS = {"ip": 0, "l2": 1, "cosine": 2, "hamming": 3}   # (oracle.IP, L2, COS, HAMMING)


def oracle_topk(orc, query, rows, k, metric, f16=False):
    """the oracle's canonical top-k of one query -> (ids u32, distances f32); an F16 shard: the sequential-sum kernels over the decoded rows"""
    if f16 and metric != "hamming":
        return orc.canonical_topk_f16(query, rows, k, METRIC_IDS[metric])
    return orc.canonical_topk(query, rows, k, METRIC_IDS[metric])


def centred(rng, n, dim):
    return rng.random((n, dim), dtype=f32) - f32(0.5)


@dataclass(frozen=True)
class Spec:
    """One seeded case.  kind "compact": n_after rows stay (row 0 and a random choice of the others leave; keep_p, when given, keeps each
    row with that probability instead).  kind "update": n_change rows are overwritten, among them the rows of largest and smallest norm."""
    name: str
    n0: int
    dim: int
    seed: int
    kind: str
    n_after: int = 0
    keep_p: float = 0.0
    n_change: int = 0
    n_append: int = 0      # rows drawn for the append after the mutation (0: the case does not append)
    n_inside: int = APPEND_INSIDE   # the short append; the sources of the (c) queries lie among these rows
    f16: bool = False
    metrics: tuple = ("ip", "l2", "cosine")
    data: str = "centred"   # "unit": uniform in [0, 1) — the binary metrics set a bit where x > 0.5


class Case:
    def __init__(self, spec: Spec):
        self.spec = s = spec
        rng = np.random.default_rng(s.seed)
        n0, dim = s.n0, s.dim
        draw = centred if s.data == "centred" else (lambda r, n, d: r.random((n, d), dtype=f32))
        base = draw(rng, n0, dim)
        if s.kind == "compact":
            if s.keep_p:
                keep = rng.random(n0) < s.keep_p
            else:
                keep = np.ones(n0, bool)
                keep[rng.choice(np.arange(1, n0), n0 - s.n_after - 1, replace=False)] = False
            keep[0] = False
            new_len = int(keep.sum())
            kept, gone = np.nonzero(keep)[0], np.nonzero(~keep)[0]
            gone = gone[(gone < new_len) & (gone > 0)]                 # the stale layout still holds them
            src_a = rng.choice(kept, N_PLANT, replace=False)
            src_b = rng.choice(gone, N_PLANT, replace=False)
            self.keep, self.rows_changed, self.new = keep, None, None
        else:
            src_b = rng.choice(n0, N_PLANT, replace=False)
            src_a = np.zeros(0, np.int64)
            self.keep = None
        base[np.concatenate([src_a, src_b])] *= PLANT_SCALE
        self.base = base
        before = RowModel(dim, s.f16)
        before.write(base)
        self.before = before.rows
        after = RowModel(dim, s.f16)
        after.rows = before.rows
        if s.kind == "compact":
            after.compact(self.keep)
        else:
            norms = (self.before.astype(np.float64) ** 2).sum(axis=1)
            fixed = np.unique(np.concatenate([src_b, [int(norms.argmax()), int(norms.argmin())]]))
            others = rng.choice(np.setdiff1d(np.arange(n0), fixed), s.n_change - fixed.size, replace=False)
            rows = np.concatenate([fixed, others])
            rng.shuffle(rows)
            self.rows_changed, self.new = rows, draw(rng, rows.size, dim)
            after.update(rows, self.new)
        self.after = after.rows
        self.src_a, self.src_b = src_a, src_b
        self.q_a, self.q_b = self.before[src_a].copy(), self.before[src_b].copy()
        self.stale = self.before[:len(after)]                      # old rows at their old positions, cut at the new length
        self.more = self.q_c = self.src_c = None
        if s.n_append:
            # rows appended after the mutation, from a stream of their own; the sources of the (c) queries lie among the first
            # n_inside of them, so a short and a long append plant the same queries
            rng_c = np.random.default_rng(s.seed + 1_000_003)
            more = draw(rng_c, s.n_append, dim)
            src = np.sort(rng_c.choice(min(s.n_append, s.n_inside), N_PLANT, replace=False))
            more[src] *= PLANT_SCALE
            self.more, self.src_c = more, len(after) + src
            self.q_c = after.store(more[src])

    def final(self, n_append):
        """the rows after the mutation and an append of the first n_append rows of `more`"""
        m = RowModel(self.spec.dim, self.spec.f16)
        m.rows = self.after
        m.write(self.more[:n_append])
        return m.rows

    def mutate(self, idx):
        """apply the mutation of the case to a FlatIndex -> the new length"""
        if self.spec.kind == "compact":
            return idx.compact(self.keep)
        idx.update_rows(self.rows_changed, self.new)
        return len(idx)

    def slots(self, kind):
        """the query slots of one planted kind in every batch of the case"""
        first = {"a": 0, "b": len(self.q_a), "c": len(self.q_a) + len(self.q_b)}[kind]
        return range(first, first + len({"a": self.q_a, "b": self.q_b, "c": self.q_c if self.q_c is not None else ()}[kind]))

    def batch(self, nq):
        """nq queries: the planted ones first ((a), (b), then (c) when the case appends), then near copies of rows — three in four of
        them of rows the mutation touched (an update: the new content and the content it replaced, alternating), the rest of any row left"""
        planted = [self.q_a, self.q_b] + ([self.q_c] if self.q_c is not None else [])
        planted = np.concatenate(planted)[:nq]
        rng = np.random.default_rng(self.spec.seed * 7919 + nq)
        n_rand = nq - planted.shape[0]
        src = self.after[rng.integers(0, self.after.shape[0], n_rand)].copy()
        if self.spec.kind == "update":
            touched = rng.integers(0, self.rows_changed.size, n_rand)
            new, old = self.after[self.rows_changed[touched]], self.before[self.rows_changed[touched]]
            which = np.arange(n_rand) % 4
            src[which == 1] = new[which == 1]
            src[which == 2] = old[which == 2]
            src[which == 3] = new[which == 3]
        noise = f32(0.02) * rng.standard_normal(src.shape).astype(f32)
        return np.ascontiguousarray(np.concatenate([planted, (src + noise).astype(f32)]), f32)


# The cases of tests/test_gpu_mutation_paths.py (the row counts are the thresholds of the paths; include/lynse_hip.h and the dispatch in
# lynsedb_amd/csrc/lynse_hip.hip: the certified int8 pass and the FP4 Hamming copy from 65,536 rows on, k_scan_qh at 64 / 128 halves per row)
SPECS = {s.name: s for s in [
    Spec("ip32_compact", 72_000, 32, 9101, "compact", n_after=66_000, n_append=APPEND_REGROW, metrics=("ip",)),
    Spec("ip32_update", 72_000, 32, 9102, "update", n_change=300, n_append=APPEND_REGROW, metrics=("ip",)),
    Spec("d256_compact", 72_000, 256, 9103, "compact", keep_p=0.92, n_append=APPEND_REGROW, metrics=("ip", "l2", "cosine")),
    Spec("d256_update", 72_000, 256, 9104, "update", n_change=200, n_append=APPEND_REGROW, metrics=("ip", "l2", "cosine")),
    Spec("ham256_compact", 72_000, 256, 9116, "compact", keep_p=0.92, n_append=APPEND_REGROW, metrics=("hamming",), data="unit"),
    Spec("ham256_update", 72_000, 256, 9117, "update", n_change=200, n_append=APPEND_REGROW, metrics=("hamming",), data="unit"),
    Spec("qh64_compact", 20_000, 64, 9105, "compact", n_after=17_000, metrics=("ip",)),
    Spec("qh100_compact", 20_000, 100, 9106, "compact", n_after=17_000, metrics=("ip",)),
    Spec("qh100_f16_compact", 20_000, 100, 9107, "compact", n_after=17_000, f16=True, metrics=("ip",)),
    Spec("small128_compact", 5_000, 128, 9108, "compact", n_after=4_200, n_append=3_000, n_inside=500),
    Spec("small128_update", 5_000, 128, 9109, "update", n_change=120, n_append=3_000, n_inside=500),
    Spec("range27_compact", 3_000, 27, 9110, "compact", n_after=2_400, metrics=("l2",)),
    Spec("range27_update", 3_000, 27, 9111, "update", n_change=100, metrics=("l2",)),
    Spec("range27_f16_compact", 3_000, 27, 9112, "compact", n_after=2_400, f16=True, metrics=("l2",)),
    Spec("range27_f16_update", 3_000, 27, 9113, "update", n_change=100, f16=True, metrics=("l2",)),
    Spec("submit_compact", 30_000, 32, 9114, "compact", n_after=26_000, metrics=("l2",)),
    Spec("submit_update", 30_000, 32, 9115, "update", n_change=150, metrics=("l2",)),
]}
# (d256_compact: "a random keep with p ~ 0.08" of the rows leaving: 72,000 x 0.92 = 66,240 +- 73 rows stay, above the 65,536 of the int8 pass)


_cases = {}


def case(name) -> Case:
    """the case of a spec, built once per process and never written to"""
    if name not in _cases:
        c = Case(SPECS[name])
        for a in (c.base, c.before, c.after, c.stale, c.q_a, c.q_b):
            a.setflags(write=False)
        _cases[name] = c
    return _cases[name]


# ---- the seeded operation sequences ---------------------------------------------------------------------------------------------------
SEQ_SEEDS = (9201, 9202, 9203)
SEQ_SHAPES = {"f32": (3_000, 24, False), "f16": (2_000, 40, True)}
SEQ_STEPS = 12
SEQ_METRICS = ("ip", "l2", "cosine", "hamming")


def draw_ops(seed, n0, dim, f16, steps=SEQ_STEPS):
    """-> (first rows, [(op, args...)]): the operation list of one sequence.  Every argument is drawn here, from the model's length at that
    step, so the list can be printed and replayed.  Every list holds a write, an update and a compaction, and ends with a search."""
    rng = np.random.default_rng(seed)
    model = RowModel(dim, f16)
    first = centred(rng, n0, dim)
    model.write(first)
    ops = []
    names = ["write", "update", "compact", "search", "search", "filtered", "range", "aux"]
    forced = {1: "update", 4: "compact", 7: "write", steps - 1: "search"}
    for step in range(steps):
        n = len(model)
        op = forced.get(step) or names[int(rng.integers(0, len(names)))]
        if op == "aux" and f16:   # (PQ and HNSW are f32-shard indexes)
            op = "filtered"
        if op == "write":
            a = centred(rng, int(rng.integers(1, 400)), dim)
            model.write(a)
            ops.append(("write", a))
        elif op == "update":
            rows = rng.choice(n, int(rng.integers(1, 60)), replace=False)
            new = centred(rng, rows.size, dim)
            model.update(rows, new)
            ops.append(("update", rows, new))
        elif op == "compact":
            keep = rng.random(n) < rng.uniform(0.5, 0.95)
            keep[0] = False
            model.compact(keep)
            ops.append(("compact", keep))
        elif op == "search":
            nq = int(rng.choice([3, 16, 40]))
            q = model.rows[rng.integers(0, n, nq)] + f32(0.02) * rng.standard_normal((nq, dim)).astype(f32)
            ops.append(("search", q.astype(f32), SEQ_METRICS[int(rng.integers(0, len(SEQ_METRICS)))]))
        elif op == "filtered":
            q = model.rows[rng.integers(0, n, 16)] + f32(0.02) * rng.standard_normal((16, dim)).astype(f32)
            ops.append(("filtered", q.astype(f32), ("ip", "l2", "cosine")[int(rng.integers(0, 3))], np.sort(rng.choice(n, min(n, 300), replace=False))))
        elif op == "range":
            q = model.rows[rng.integers(0, n, 5)] + f32(0.02) * rng.standard_normal((5, dim)).astype(f32)
            ops.append(("range", q.astype(f32), int(rng.integers(10, 60))))
        else:
            q = model.rows[rng.integers(0, n, 16)] + f32(0.02) * rng.standard_normal((16, dim)).astype(f32)
            ops.append(("aux", q.astype(f32), "pq" if rng.integers(0, 2) else "hnsw"))
    return first, ops


def describe(ops):
    out = []
    for op in ops:
        if op[0] == "write":
            out.append(f"write {op[1].shape[0]} rows")
        elif op[0] == "update":
            out.append(f"update {op[1].size} rows")
        elif op[0] == "compact":
            out.append(f"compact {op[1].size} -> {int(op[1].sum())}")
        elif op[0] == "search":
            out.append(f"search {op[1].shape[0]} x {op[2]}")
        elif op[0] == "filtered":
            out.append(f"filtered {op[2]} over {op[3].size} rows")
        elif op[0] == "range":
            out.append(f"range l2, the {op[2]}-th distance")
        else:
            out.append(f"build_{op[2]} + search")
    return "; ".join(out)
