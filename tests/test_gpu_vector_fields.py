"""Named vector fields on the device: the words and the count of k_bitset_remap against the per-bit model of
tests/vector_fields_common.py, what the remap refuses before a launch, field searches (unfiltered, `where=`, `subset=`, tombstones)
against the dict model with the oracle's distances, and the life cycle of a field."""
import ctypes as C

import numpy as np
import pytest

import fields_common as F
import vector_fields_common as V

pytestmark = pytest.mark.gpu

NONE = V.NONE
N_OUT = [0, 1, 63, 64, 65, 127, 129, 4_113]
N_SRC = [1, 64, 65, 4_113, 300_017]
DENSITIES = [0.0, 0.01, 0.5, 1.0]
N_TAIL = [0, 1, 64, 70]
KINDS = ["identity", "reversed", "permutation", "one in three", "one row", "sentinels at word edges"]


@pytest.fixture(scope="module")
def L():
    import lynsedb_amd as L

    return L


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def random_words(n, density, seed):
    """BitSet words over n rows, each bit set with probability `density`; zero beyond n.  (numpy makes the INPUT; the model decides.)"""
    rng = np.random.default_rng(seed)
    mask = np.ones(n, bool) if density >= 1.0 else np.zeros(n, bool) if density <= 0.0 else rng.random(n) < density
    pad = np.zeros((n + 63) // 64 * 64, np.uint8)
    pad[:n] = mask
    return np.packbits(pad, bitorder="little").view(np.uint64) if pad.size else np.zeros(0, np.uint64)


def make_row_of(kind, n_out, n_total, seed):
    """a Python list of n_out entries, each below n_total or NONE"""
    if kind == "identity":
        return [r if r < n_total else NONE for r in range(n_out)]
    if kind == "reversed":
        return [n_total - 1 - r if r < n_total else NONE for r in range(n_out)]
    if kind == "permutation":
        perm = np.random.default_rng(seed).permutation(n_total)[:n_out].tolist()
        return perm + [NONE] * (n_out - len(perm))
    if kind == "one in three":
        return [3 * r if 3 * r < n_total else NONE for r in range(n_out)]
    if kind == "one row":
        return [n_total - 1] * n_out
    out = [(r * 7919 + 13) % n_total for r in range(n_out)]
    for r in (0, 63, 64, n_out - 1):
        if 0 <= r < n_out:
            out[r] = NONE
    return out


_SRC_CACHE = {}


def source(n_src, density):
    key = (n_src, density)
    if key not in _SRC_CACHE:
        w = random_words(n_src, density, 1000 + n_src + int(density * 100))
        _SRC_CACHE[key] = (w, w.tolist())
    return _SRC_CACHE[key]


# ---- 1. the kernel against the model ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_out", N_OUT)
def test_remap_words_and_count_match_the_model(L, n_out):
    """every n_src, every shape of row_of, every tail and every source density at this n_out: the full cross, 480 remaps.  Under an
    all-ones source the tail is all ones too, so whole output words of ones meet the ballot, the count and the zero bits beyond n_out."""
    rm = L.RowMap()
    case = 0
    seen = set()
    for n_src in N_SRC:
        for kind in KINDS:
            for n_tail in N_TAIL:
                case += 1
                row_of = make_row_of(kind, n_out, n_src + n_tail, case)
                rm.set(np.array(row_of, dtype=np.uint32))
                for density in DENSITIES:
                    src, src_list = source(n_src, density)
                    tail = random_words(n_tail, 1.0 if density == 1.0 else 0.5, 77 + case)
                    want_words, want_count = V.remap_model(row_of, src_list, n_src, tail.tolist(), n_tail)
                    ptr, nw, count = rm.remap(src, n_src, tail, n_tail)
                    what = (n_out, n_src, kind, density, n_tail)
                    assert nw == (n_out + 63) // 64 == len(want_words) and bool(ptr.value) == (n_out > 0), what
                    assert count == want_count, what
                    got = rm.words().tolist()
                    assert got == want_words, (what, [i for i, (a, b) in enumerate(zip(got, want_words)) if a != b][:4])
                    if n_out % 64:
                        assert got[-1] >> (n_out % 64) == 0, what           # bits at and beyond n_out are zero
                    if density == 1.0:                                      # every mapped row passes: the count is the rows that are not NONE
                        assert count == sum(1 for j in row_of if j != NONE), what
                    seen.add((kind, density, n_tail))
    assert len(seen) == len(KINDS) * len(DENSITIES) * len(N_TAIL)           # each density met each tail under each shape


def test_remap_more_than_one_grid_pass(L):
    """300,017 field rows over 300,017 source rows, permuted: the grid-stride loop takes more than one pass"""
    n = 300_017
    src, src_list = source(n, 0.5)
    row_of = make_row_of("permutation", n, n, 5)
    want_words, want_count = V.remap_model(row_of, src_list, n)
    rm = L.RowMap()
    rm.set(np.array(row_of, dtype=np.uint32))
    ptr, nw, count = rm.remap(src, n)
    assert nw == (n + 63) // 64 and count == want_count
    assert rm.words().tolist() == want_words
    assert rm.hbm_bytes() >= n * 4 + 2 * nw * 8


@pytest.mark.parametrize("n", [1, 64, 65, 4_113, 300_017])
def test_identity_shortcut_and_kernel_give_the_same_words(L, n):
    """the source words left on the device by k_field_filter; row_of the identity over n_out == n_src, no tail: handed on without a
    launch — and the kernel, forced on the same input, writes the same words and the same count"""
    from lynsedb_amd import fields as W
    from lynsedb_amd._lib import FieldLeaf

    ff = W.FieldFilter()
    ff.set_column(0, np.full(n, W.TAG_INT, np.uint8), (np.arange(n) * 2654435761 % 1000).astype(np.uint64))
    leaf = (FieldLeaf * 1)(FieldLeaf(W.LEAF_NUM_RANGE, 0, W.OP_LT, 0, 0, 0, W.normalize_f64_bits(300.0), 0, 0))
    count = ff.run(n, False, leaf, np.zeros(0, np.uint64))
    d_src, nsw = ff.words_device()
    src = ff.words()
    rm = L.RowMap()
    rm.set(np.arange(n, dtype=np.uint32))
    assert rm.identity
    ptr, nw, c = rm.remap(d_src, n, src_count=count, n_src_words=nsw)
    assert rm.last_shortcut and ptr.value == d_src.value and (nw, c) == (nsw, count)
    ptr2, nw2, c2 = rm.remap(d_src, n, src_count=count, n_src_words=nsw, force_kernel=True)
    assert not rm.last_shortcut and ptr2.value != d_src.value and (nw2, c2) == (nsw, count)
    assert np.array_equal(rm.words(), src)
    want_words, want_count = V.remap_model(list(range(n)), src.tolist(), n)
    assert src.tolist() == want_words and count == want_count
    # anything but the identity over n_out == n_src without a tail goes through the kernel
    assert rm.remap(d_src, n, np.zeros(1, np.uint64), 1, src_count=count, n_src_words=nsw)[2] == count and not rm.last_shortcut
    if n > 1:
        rm.set(np.arange(n - 1, dtype=np.uint32))
        rm.remap(d_src, n, src_count=count, n_src_words=nsw)
        assert not rm.last_shortcut


# ---- 2. refusals before a launch --------------------------------------------------------------------------------------------------
def test_remap_refuses_what_the_kernel_could_not_bound(L):
    rm = L.RowMap()
    one = np.array([0b10110], np.uint64)
    with pytest.raises(ValueError, match="remap before set"):
        rm.remap(one, 5)
    rm.set(np.array([0, 5, NONE, 2], np.uint32))
    with pytest.raises(ValueError, match="beyond n_src"):                 # row_of out of range: 5 is not below 5 + 0
        rm.remap(one, 5)
    with pytest.raises(ValueError, match="n_src_words"):                  # two words for 64 bits
        rm.remap(np.zeros(2, np.uint64), 64)
    with pytest.raises(ValueError, match="n_src_words"):                  # no word for 6 bits
        rm.remap(np.zeros(0, np.uint64), 6)
    with pytest.raises(ValueError, match="n_tail_words"):                 # a tail word for no tail bit
        rm.remap(one, 6, np.zeros(1, np.uint64), 0)
    with pytest.raises(ValueError, match="n_tail_words"):                 # one word for 65 tail bits
        rm.remap(one, 6, np.zeros(1, np.uint64), 65)
    with pytest.raises(ValueError):                                        # the words of a refused remap are not there to read
        from lynsedb_amd._lib import check, lib

        check(lib.lynse_hip_rowmap_words(rm._h, np.zeros(1, np.uint64).ctypes.data_as(C.c_void_p), 1))
    # the next valid calls still answer: row 5 is the first tail row
    ptr, nw, count = rm.remap(one, 5, np.array([1], np.uint64), 1)
    assert (nw, count) == (1, 2) and rm.words().tolist() == [0b1010]
    ptr, nw, count = rm.remap(one, 6)
    assert (nw, count) == (1, 1) and rm.words().tolist() == [0b1000]
    rows, bound = C.c_uint64(0), C.c_uint64(0)
    from lynsedb_amd._lib import check, lib

    check(lib.lynse_hip_rowmap_len(rm._h, C.byref(rows), C.byref(bound)))
    assert (rows.value, bound.value) == (4, 6)


# ---- 3. search parity -------------------------------------------------------------------------------------------------------------
N_REC, N_PEND, DIM0 = 3_000, 17, 8
FIRST_ID = 1000


class World:
    pass


def record_fields(i, member):
    return {"g": i % 100, "lang": ("en", "de", "fr")[i % 3], "in_b": int(member["b"]), "in_c": int(member["c"]), "in_d": int(member["d"])}


@pytest.fixture(scope="module")
def additive_ref(tmp_path_factory):
    from additive_common import build_ref

    return build_ref(tmp_path_factory.mktemp("additive_ref"))


@pytest.fixture(scope="module")
def world(L, oracle, additive_ref):
    """3,000 records, the last 17 still pending.  Field a: 24-d ip over every id in insertion order; b: 40-d l2 f16 over a shuffled
    1-in-3 subset, the 17 pending ids among them; c: 128-bit hamming over every second id, backwards; d: 16-d l1 over a shuffled
    quarter.  `plain` is the same collection without a field.  The oracle's distances of every query to every field row are computed
    once; no test changes the world (tombstones are restored)."""
    import oracle as O
    from additive_common import L1

    w = World()
    rng = np.random.default_rng(2626)
    ids = np.arange(FIRST_ID, FIRST_ID + N_REC)
    pend = ids[N_REC - N_PEND:]
    b_ids = np.concatenate([rng.choice(ids[:N_REC - N_PEND], N_REC // 3 - N_PEND, replace=False), pend])
    rng.shuffle(b_ids)
    c_ids = ids[::2][::-1].copy()
    d_ids = rng.choice(ids, N_REC // 4, replace=False)
    w.field_ids = {"a": ids.copy(), "b": b_ids, "c": c_ids, "d": d_ids}
    sets = {n: set(v.tolist()) for n, v in w.field_ids.items()}
    w.rows = [record_fields(i, {n: (FIRST_ID + i) in sets[n] for n in "bcd"}) for i in range(N_REC)]
    w.primary = rng.standard_normal((N_REC, DIM0)).astype(np.float32)
    w.spec = {"a": (24, "ip", None, O.IP), "b": (40, "l2", "f16", O.L2), "c": (128, "hamming", None, O.HAMMING), "d": (16, "l1", None, L1)}
    w.data, w.queries, w.dists = {}, {}, {}
    for name, (dim, metric, dtype, oid) in w.spec.items():
        n = w.field_ids[name].size
        if metric == "hamming":
            w.data[name], w.queries[name] = (rng.random((n, dim)) < 0.5).astype(np.float32), (rng.random((5, dim)) < 0.5).astype(np.float32)
        else:
            w.data[name], w.queries[name] = rng.standard_normal((n, dim)).astype(np.float32), rng.standard_normal((5, dim)).astype(np.float32)
        q = w.queries[name]
        if metric == "l1":
            w.dists[name] = additive_ref.dists(L1, q, w.data[name])       # (the oracle has no additive metric: tests/additive_ref is theirs)
        elif dtype == "f16":
            dec = oracle.round_f16(w.data[name])
            w.dists[name] = np.stack([oracle.all_distances_f16(q[i], dec, oid) for i in range(5)])
        else:
            w.dists[name] = np.stack([oracle.all_distances(q[i], w.data[name], oid) for i in range(5)])

    def build(with_fields):
        c = L.Collection("vf", DIM0)
        cut = N_REC - N_PEND
        c.add_items(w.primary[:cut], ids[:cut].tolist(), fields=w.rows[:cut])
        c.commit()
        c.add_items(w.primary[cut:], ids[cut:].tolist(), fields=w.rows[cut:])
        assert c.pending_len() == N_PEND
        if with_fields:
            for name, (dim, metric, dtype, _) in w.spec.items():
                c.create_vector_field(name, dim, metric, None, dtype)
                half = w.field_ids[name].size // 2                        # two calls: the id map grows in chunks
                c.add_named_vectors(name, w.data[name][:half], w.field_ids[name][:half].tolist())
                c.add_named_vectors(name, w.data[name][half:], w.field_ids[name][half:].tolist())
            assert c.pending_len() == N_PEND                              # named vectors do not flush the primary rows
        return c

    w.c, w.plain = build(True), build(False)
    w.id_row = {FIRST_ID + i: i for i in range(N_REC)}
    return w


def allowed_ids(w, cond):
    return {FIRST_ID + i for i, r in enumerate(w.rows) if F.model_match(cond, r)}


def check_field_search(w, name, k, allowed, tombstones, what, **kw):
    """batch_search_vector_field and search_vector_field against the model: ids and distance bits"""
    ascending = w.spec[name][1] != "ip"
    q = w.queries[name]
    got = w.c.batch_search_vector_field(name, q, k, **kw)
    assert len(got) == 5
    field_ids = w.field_ids[name].tolist()
    for i in range(5):
        want_ids, want_rows = V.field_search_model(field_ids, w.dists[name][i].tolist(), allowed, tombstones, k, ascending)
        assert got[i].ids().tolist() == want_ids, (what, name, k, i, got[i].ids()[:8], want_ids[:8])
        assert np.array_equal(bits(got[i].distances()), bits(w.dists[name][i][want_rows])), (what, name, k, i)
        assert got[i].index_mode() == w.c._vfields[name].index_mode and got[i]._dim == w.spec[name][0]
    one = w.c.search_vector_field(name, q[0], k, **kw)
    assert one.ids().tolist() == got[0].ids().tolist() and np.array_equal(bits(one.distances()), bits(got[0].distances())), (what, name, k)


WHERE = {"1 %": F.rng("g", "<", "1"), "60 %": F.rng("g", "<", "60"), "nothing": F.rng("g", "<", "0"),
         "and": F.all_of(F.rng("g", ">=", "10"), F.eq("lang", "'en'"))}


@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_field_search_matches_the_model(L, world, name):
    w = world
    n_field = w.field_ids[name].size
    ks = (1, 10, n_field + 5)
    for k in ks:
        check_field_search(w, name, k, None, set(), "unfiltered")
        for label, (expr, cond) in WHERE.items():
            check_field_search(w, name, k, allowed_ids(w, cond), set(), label, where=expr)
        if name != "a":                                                    # a filter that selects only ids outside the field
            expr, cond = F.eq(f"in_{name}", "0")
            allowed = allowed_ids(w, cond)
            assert allowed and not allowed & set(w.field_ids[name].tolist())
            check_field_search(w, name, k, allowed, set(), "outside the field", where=expr)
            assert all(len(r) == 0 for r in w.c.batch_search_vector_field(name, w.queries[name], k, where=expr))
        rows = np.random.default_rng(k).choice(N_REC, 700, replace=False)   # collection rows, pending ones among them
        rows = np.concatenate([rows, [N_REC - 1, N_REC - N_PEND]])
        allowed = {FIRST_ID + int(r) for r in rows}
        check_field_search(w, name, k, allowed, set(), "subset rows", subset=rows)
        check_field_search(w, name, k, allowed, set(), "subset BitSet", subset=L.BitSet.from_rows(rows, N_REC))
    # 25 tombstones, 9 of them inside field b
    inside_b = w.field_ids["b"][:9].tolist()
    b_set = set(w.field_ids["b"].tolist())
    outside_b = [int(i) for i in w.field_ids["a"] if int(i) not in b_set][:16]
    dead = set(inside_b + outside_b)
    assert len(dead) == 25
    w.c.delete_items(dead)
    try:
        for k in ks:
            check_field_search(w, name, k, None, dead, "tombstones")
            expr, cond = WHERE["60 %"]
            check_field_search(w, name, k, allowed_ids(w, cond), dead, "tombstones + where", where=expr)
    finally:
        w.c.restore_items(dead)
    assert w.c.list_deleted_ids() == []


@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_device_hand_off_equals_the_standalone_filtered_scan(L, world, name):
    """the filtered field search through k_field_filter -> k_bitset_remap -> the device-words entry, against a FlatIndex of the field's
    rows alone given the model's row subset: rows, distance bits and counts"""
    w = world
    dim, metric, dtype, _ = w.spec[name]
    alone = L.FlatIndex(None, dim, dtype=dtype or "f32")
    alone.write(w.data[name])
    field_ids = w.field_ids[name].tolist()
    for label in ("1 %", "60 %", "and"):
        expr, cond = WHERE[label]
        allowed = allowed_ids(w, cond)
        sub = np.array([r for r, i in enumerate(field_ids) if i in allowed], dtype=np.uint64)
        for k in (1, 10):
            got = w.c.batch_search_vector_field(name, w.queries[name], k, where=expr)
            rows, dists, counts = alone.search_filtered_batch_arrays(w.queries[name], k, metric, sub)
            for i in range(5):
                c = int(counts[i])
                assert got[i].ids().tolist() == [field_ids[int(r)] for r in rows[i, :c]], (name, label, k, i)
                assert np.array_equal(bits(got[i].distances()), bits(dists[i, :c])), (name, label, k, i)
    f = w.c._vfields[name]
    assert f.rowmap is not None and not f.rowmap.last_shortcut and f.rowmap.last_kernel_us > 0.0   # pending rows: the kernel ran


def test_a_collection_without_fields_is_unchanged(L, world):
    """`search` on the primary vector: the collection that carries four fields and the one that never created any"""
    w = world
    q = np.random.default_rng(9).standard_normal((5, DIM0)).astype(np.float32)
    for kw in ({}, {"where": WHERE["60 %"][0]}, {"subset": np.arange(0, N_REC, 7)}):
        a, b = w.c.batch_search(q, 10, **kw), w.plain.batch_search(q, 10, **kw)
        for x, y in zip(a, b):
            assert np.array_equal(x.ids(), y.ids()) and np.array_equal(bits(x.distances()), bits(y.distances())) and x.index_mode() == y.index_mode()
    assert w.plain._vfields == {} and w.plain.list_vector_fields() == [
        {"name": "default", "dimension": DIM0, "metric": "ip", "index_mode": "FLAT-IP", "dtypes": "float32"}]
    # `default` and a blank name delegate to the primary search
    for blank in ("default", "", "  "):
        d = w.c.batch_search_vector_field(blank, q, 10, where=WHERE["60 %"][0])
        p = w.plain.batch_search(q, 10, where=WHERE["60 %"][0])
        assert all(np.array_equal(x.ids(), y.ids()) and np.array_equal(bits(x.distances()), bits(y.distances())) for x, y in zip(d, p))
        assert np.array_equal(w.c.search_vector_field(blank, q[0], 3).ids(), w.plain.search(q[0], 3).ids())
        assert w.c.vector_field_shape(blank) == w.c.shape()


# ---- 4. life cycle ----------------------------------------------------------------------------------------------------------------
N_SMALL = 600


def small(L, oracle, seed=4):
    """600 flushed records; field a: 24-d l2 over every id in order, field b: 40-d l2 f16 over a shuffled third"""
    import oracle as O

    w = World()
    rng = np.random.default_rng(seed)
    ids = np.arange(FIRST_ID, FIRST_ID + N_SMALL)
    w.rows = [{"g": i % 100, "lang": ("en", "de", "fr")[i % 3]} for i in range(N_SMALL)]
    w.primary = rng.standard_normal((N_SMALL, DIM0)).astype(np.float32)
    w.field_ids = {"a": ids.copy(), "b": rng.permutation(ids)[:N_SMALL // 3]}
    w.spec = {"a": (24, "l2", None, O.L2), "b": (40, "l2", "f16", O.L2)}
    w.data = {n: rng.standard_normal((w.field_ids[n].size, w.spec[n][0])).astype(np.float32) for n in w.spec}
    w.queries = {n: rng.standard_normal((5, w.spec[n][0])).astype(np.float32) for n in w.spec}
    w.c = L.Collection("life", DIM0)
    w.c.add_items(w.primary, ids.tolist(), fields=w.rows)
    w.c.commit()
    for n, (dim, metric, dtype, _) in w.spec.items():
        w.c.create_vector_field(n, dim, metric, None, dtype)
        w.c.add_named_vectors(n, w.data[n], w.field_ids[n].tolist())
    refresh_dists(w, oracle)
    return w


def refresh_dists(w, oracle, metric_of=None):
    import oracle as O

    w.dists = {}
    for n, (dim, metric, dtype, oid) in w.spec.items():
        oid = (metric_of or {}).get(n, oid)
        q = w.queries[n]
        if dtype == "f16":
            dec = oracle.round_f16(w.data[n])
            w.dists[n] = np.stack([oracle.all_distances_f16(q[i], dec, oid) for i in range(5)])
        else:
            w.dists[n] = np.stack([oracle.all_distances(q[i], w.data[n], oid) for i in range(5)])
    return O


def test_add_named_vectors_errors_in_the_reference_order(L, oracle):
    w = small(L, oracle)
    c = w.c
    free = [int(i) for i in w.field_ids["a"] if int(i) not in set(w.field_ids["b"].tolist())]
    have = int(w.field_ids["b"][0])
    vec = lambda n, d=40: np.ones((n, d), np.float32)   # noqa: E731
    before = c.batch_search_vector_field("b", w.queries["b"], 10)
    cases = [
        ("zz", vec(1), [free[0]], "Invalid argument: vector field 'zz' does not exist"),
        ("a b", vec(1), [free[0]], "Invalid argument: vector field name may only contain ASCII letters, digits, '_' and '-'"),
        ("b", vec(2, 39), [free[0]], "Dimension mismatch: expected 40, got 39"),                       # the dimension before the length
        ("b", vec(3), free[:2], "Invalid argument: ids length (2) must match n_vectors (3)"),
        ("b", vec(3), [free[0], free[0], 5], "Invalid argument: duplicate id %d within named vector batch" % free[0]),   # per id, in order
        ("b", vec(3), [free[0], 5, free[0]], "Invalid argument: cannot add named vector for unknown id 5"),
        ("b", vec(2), [have, 5], "Invalid argument: id %d already has a vector for field 'b'" % have),
        ("b", vec(2), [5, have], "Invalid argument: cannot add named vector for unknown id 5"),
        ("b", vec(3), [free[0], free[1], have], "Invalid argument: id %d already has a vector for field 'b'" % have),     # the last id fails: nothing is added
    ]
    for field, v, ids, msg in cases:
        with pytest.raises(RuntimeError) as e:
            c.add_named_vectors(field, v, ids)
        assert str(e.value) == msg
        assert c.vector_field_shape("b") == (N_SMALL // 3, 40) and len(c._vfields["b"].flat) == N_SMALL // 3
    after = c.batch_search_vector_field("b", w.queries["b"], 10)
    assert all(np.array_equal(x.ids(), y.ids()) and np.array_equal(bits(x.distances()), bits(y.distances())) for x, y in zip(before, after))
    c.add_named_vectors("b", np.zeros((0, 40), np.float32), [])           # an empty batch is accepted and adds nothing
    assert c.vector_field_shape("b") == (N_SMALL // 3, 40)
    # pending ids count as known
    c.add_items(np.ones((1, DIM0), np.float32), [77])
    assert c.pending_len() == 1
    c.add_named_vectors("b", vec(1), [77])
    assert c.vector_field_shape("b") == (N_SMALL // 3 + 1, 40) and c.pending_len() == 1


def test_create_list_and_shape(L, oracle):
    c = L.Collection("cfg", DIM0)
    assert c.create_vector_field(" title ", 24) == {"name": "title", "dimension": 24, "metric": "ip", "index_mode": "FLAT-IP", "dtypes": "float32"}
    assert c.create_vector_field("img", 40, "l2", None, "half")["dtypes"] == "float16"
    assert c.create_vector_field("Bits", 128, None, "flat-hamming") == {"name": "Bits", "dimension": 128, "metric": "hamming",
                                                                        "index_mode": "FLAT-HAMMING", "dtypes": "float32"}
    assert c.create_vector_field("city", 16, "manhattan")["index_mode"] == "FLAT-L1"
    assert c.create_vector_field("graph", 8, "l2", "HNSW-L2")["index_mode"] == "HNSW-L2"   # built by build_vector_field_index, as in the reference
    assert [f["name"] for f in c.list_vector_fields()] == ["default", "Bits", "city", "graph", "img", "title"]   # default first, then by name
    assert c.list_vector_fields()[0] == {"name": "default", "dimension": DIM0, "metric": "ip", "index_mode": "FLAT-IP", "dtypes": "float32"}
    assert c.list_vector_fields()[4] == {"name": "img", "dimension": 40, "metric": "l2", "index_mode": "FLAT-L2", "dtypes": "float16"}
    # again with the same config: a no-op; with another one: refused
    assert c.create_vector_field("img", 40, "euclidean", "FLAT-L2", "f16") == c.list_vector_fields()[4]
    for args in (("img", 41, "l2", None, "f16"), ("img", 40, "ip", None, "f16"), ("img", 40, "l2", None, "f32"), ("img", 40, "l2", "HNSW-L2", "f16")):
        with pytest.raises(RuntimeError) as e:
            c.create_vector_field(*args)
        assert str(e.value) == "Invalid argument: vector field 'img' already exists with a different configuration"
    assert len(c.list_vector_fields()) == 6
    for args, msg in ((("z", 0), "Invalid argument: vector field dimension must be greater than zero"),
                      (("default", 4), "Invalid argument: 'default' is reserved for the primary collection vector"),
                      (("z", 4, "ip", "FLAT-L2"), "Invalid argument: vector field metric 'ip' does not match index mode 'FLAT-L2'"),
                      (("z", 4, None, "flat-ip-pq"), "Invalid argument: unknown vector field index mode 'FLAT-IP-PQ'"),
                      (("z", 4, None, None, "bf16"), "Invalid argument: unsupported vector dtype 'bf16'; expected float32/f32 or float16/f16")):
        with pytest.raises(RuntimeError) as e:
            c.create_vector_field(*args)
        assert str(e.value) == msg
    with pytest.raises(NotImplementedError, match="§26"):
        c.create_vector_field("z", 4, None, "IVF-L2")
    assert c.vector_field_shape("img") == (0, 40) and c.vector_field_shape("default") == (0, DIM0)
    with pytest.raises(RuntimeError, match="vector field 'nope' does not exist"):
        c.vector_field_shape("nope")
    assert len(c.search_vector_field("img", np.zeros(40, np.float32), 5)) == 0          # an empty field answers nothing
    with pytest.raises(RuntimeError, match="Dimension mismatch: expected 40, got 39"):
        c.search_vector_field("img", np.zeros(39, np.float32), 5)
    with pytest.raises(ValueError, match="not both"):
        c.search_vector_field("img", np.zeros(40, np.float32), 5, where="g < 1", subset=[0])
    with pytest.raises(NotImplementedError):
        c.search_vector_field("img", np.zeros(40, np.float32), 5, where_expr="g < 1")
    with pytest.raises(ValueError, match="Empty database"):
        c.build_vector_field_index("img", "HNSW-L2")


def test_flat_mode_change_and_the_refused_modes(L, oracle):
    import oracle as O

    w = small(L, oracle)
    c = w.c
    check_field_search(w, "b", 10, None, set(), "l2")
    c.build_vector_field_index("b", "flat-cos")
    assert c.list_vector_fields()[2] == {"name": "b", "dimension": 40, "metric": "cosine", "index_mode": "FLAT-COS", "dtypes": "float16"}
    w.spec["b"] = (40, "cosine", "f16", O.COS)
    refresh_dists(w, oracle)
    check_field_search(w, "b", 10, None, set(), "cosine")
    expr, cond = WHERE["60 %"]
    check_field_search(w, "b", 10, allowed_ids(w, cond), set(), "cosine where", where=expr)
    c.build_vector_field_index("a", "FLAT-IP")
    w.spec["a"] = (24, "ip", None, O.IP)
    refresh_dists(w, oracle)
    check_field_search(w, "a", 10, allowed_ids(w, cond), set(), "ip where", where=expr)
    # field a carries every flushed row in order and nothing is pending: the Collection path hands the filter's words on (no launch);
    # field b is a shuffled third: the kernel ran
    assert c._vfields["a"].rowmap.identity and c._vfields["a"].rowmap.last_shortcut
    assert not c._vfields["b"].rowmap.identity and not c._vfields["b"].rowmap.last_shortcut and c._vfields["b"].rowmap.last_kernel_us > 0.0
    for mode in ("FLAT-IP-SQ8", "IVF-L2", "SPANN-COS", "DISKANN-L2", "HNSW-L2-SQ8", "DISKANN-IP-PQ8", "IVF-HAMMING-BINARY"):
        with pytest.raises(NotImplementedError, match="§26"):
            c.build_vector_field_index("a", mode)
    for mode in ("FLAT-IP-PQ", "bogus", "FLAT", "HNSW-HAMMING"):
        with pytest.raises(RuntimeError) as e:
            c.build_vector_field_index("a", mode)
        assert str(e.value) == f"Invalid argument: unknown vector field index mode '{mode.upper()}'"
    with pytest.raises(RuntimeError, match="vector field 'nope' does not exist"):
        c.build_vector_field_index("nope", "FLAT-IP")
    with pytest.raises(ValueError, match="unknown index build parameter"):
        c.build_vector_field_index("a", "HNSW-L2", {"bogus": 1})
    assert c.list_vector_fields()[1]["index_mode"] == "FLAT-IP"           # the refused calls changed nothing
    # `default` delegates to build_index / remove_index
    c.build_vector_field_index("default", "FLAT-L2")
    assert c.list_vector_fields()[0]["index_mode"] == "FLAT-L2" and c.list_vector_fields()[0]["metric"] == "l2"
    c.remove_vector_field_index("")
    assert c.list_vector_fields()[0]["index_mode"] == "FLAT-IP" and c.list_vector_fields()[0]["metric"] == "ip"


def test_hnsw_on_a_field(L, oracle):
    from lynsedb_amd.core import HNSW_SEED

    w = small(L, oracle)
    c, q = w.c, w.queries["a"]
    f = c._vfields["a"]

    def alone(rows):
        idx = L.FlatIndex(None, 24)
        idx.write(rows)
        idx.build_hnsw("l2", 16, 128, 40, None, HNSW_SEED)
        return idx

    def same_as(idx, got, k):
        rows, dists, counts = idx.search_hnsw_batch_arrays(q, k, "l2", 0)
        ids = f.id_map()
        for i in range(5):
            n = int(counts[i])
            assert got[i].ids().tolist() == ids[rows[i, :n].astype(np.int64)].tolist(), i
            assert np.array_equal(bits(got[i].distances()), bits(dists[i, :n])), i
            assert got[i].index_mode() == "HNSW-L2"

    c.build_vector_field_index("a", "hnsw-l2", {"ef_search": 40})
    assert c.list_vector_fields()[1]["index_mode"] == "HNSW-L2" and f.hnsw and f.flat.hnsw_params(arrays=False)["ef_search"] == 40
    same_as(alone(w.data["a"]), c.batch_search_vector_field("a", q, 10), 10)
    # bypassed under a filter and under a tombstone: the exact answers of the model
    expr, cond = WHERE["60 %"]
    check_field_search(w, "a", 10, allowed_ids(w, cond), set(), "hnsw + where", where=expr)
    dead = {int(w.field_ids["a"][3])}
    c.delete_items(dead)
    check_field_search(w, "a", 10, None, dead, "hnsw + tombstone")
    c.restore_items(dead)
    # rebuilt by the first search after more vectors were added
    new_ids = [5000, 5001, 5002]
    c.add_items(np.ones((3, DIM0), np.float32), new_ids)
    more = np.random.default_rng(1).standard_normal((3, 24)).astype(np.float32)
    c.add_named_vectors("a", more, new_ids)
    assert f.hnsw_rows == N_SMALL
    got = c.batch_search_vector_field("a", q, 10)
    assert f.hnsw_rows == N_SMALL + 3
    same_as(alone(np.concatenate([w.data["a"], more])), got, 10)
    # dropped by remove_vector_field_index: the exact scan again, the mode the metric's flat mode
    c.remove_vector_field_index("a")
    assert not f.hnsw and f.flat.hnsw_params(arrays=False)["m"] == 0 and c.list_vector_fields()[1]["index_mode"] == "FLAT-L2"
    w.field_ids["a"] = np.concatenate([w.field_ids["a"], new_ids])
    w.data["a"] = np.concatenate([w.data["a"], more])
    refresh_dists(w, oracle)
    check_field_search(w, "a", 10, None, set(), "after remove")


def test_compact_and_upsert_keep_the_fields_in_step(L, oracle):
    w = small(L, oracle)
    c = w.c
    c.build_vector_field_index("a", "HNSW-L2")
    b_list = w.field_ids["b"].tolist()
    dead = set(b_list[:10] + [int(i) for i in w.field_ids["a"] if int(i) not in set(b_list)][:20])
    c.delete_items(dead)
    assert c.compact() == 30
    assert c.vector_field_shape("a") == (N_SMALL - 30, 24) and c.vector_field_shape("b") == (N_SMALL // 3 - 10, 40)
    assert c._vfields["a"].hnsw and c._vfields["a"].hnsw_rows == N_SMALL - 30          # the graph was built again
    for n in ("a", "b"):
        keep = np.array([int(i) not in dead for i in w.field_ids[n]])
        w.field_ids[n], w.data[n] = w.field_ids[n][keep], w.data[n][keep]
        assert c._vfields[n].id_map().tolist() == w.field_ids[n].tolist()
    kept = [i for i in range(N_SMALL) if FIRST_ID + i not in dead]
    w.rows = [w.rows[i] for i in kept]
    w.ids_now = [FIRST_ID + i for i in kept]
    refresh_dists(w, oracle)

    def allowed(cond):
        return {i for i, r in zip(w.ids_now, w.rows) if F.model_match(cond, r)}

    c.remove_vector_field_index("a")
    for n in ("a", "b"):
        check_field_search(w, n, 10, None, set(), "after compact")
        for label in ("1 %", "60 %"):
            expr, cond = WHERE[label]
            check_field_search(w, n, 10, allowed(cond), set(), "after compact " + label, where=expr)
    # upsert: an existing id gets a new primary vector and new fields, a new id is appended; the named vectors are untouched
    target = int(w.field_ids["b"][5])
    at = w.ids_now.index(target)
    was = w.rows[at]["g"]
    w.rows[at] = {"g": 0 if was >= 1 else 50, "lang": "en"}
    w.rows.append({"g": 0, "lang": "de"})
    w.ids_now.append(9000)
    c.upsert_items(np.full((2, DIM0), 0.5, np.float32), [target, 9000], fields=[w.rows[at], w.rows[-1]])
    assert c.vector_field_shape("b") == (N_SMALL // 3 - 10, 40)
    for n in ("a", "b"):
        for label in ("1 %", "60 %"):
            expr, cond = WHERE[label]
            check_field_search(w, n, 10, allowed(cond), set(), "after upsert " + label, where=expr)
    expr, cond = WHERE["1 %"]
    assert (target in allowed(cond)) != (was < 1)                          # the upsert moved the id across the 1 % filter
    c.update_items(np.full((1, DIM0), 0.25, np.float32), [target])
    check_field_search(w, "b", 10, allowed(cond), set(), "after update", where=expr)


def test_an_id_stored_twice_resolves_to_its_first_row(L):
    """This mirror's add_items accepts an id twice (update_items refuses such an id).  A named vector of that id follows the id's FIRST
    row under a filter, pending or flushed, and the search answers instead of raising."""
    c = L.Collection("dup", DIM0)
    c.add_items(np.ones((3, DIM0), np.float32), [1, 2, 3], fields=[{"g": 0}, {"g": 5}, {"g": 9}])
    c.commit()
    c.add_items(np.ones((1, DIM0), np.float32), [2], fields=[{"g": 0}])       # id 2 again: collection row 3, pending
    c.create_vector_field("f", 4, "l2")
    c.add_named_vectors("f", np.eye(3, 4, dtype=np.float32), [3, 2, 1])
    q = np.zeros(4, np.float32)
    for flushed in (False, True):
        if flushed:
            c.commit()
        assert c.pending_len() == (0 if flushed else 1)
        assert sorted(c.search_vector_field("f", q, 3, where="g < 1").ids().tolist()) == [1]        # not 2: its first row has g = 5
        assert sorted(c.search_vector_field("f", q, 3, where="g >= 5").ids().tolist()) == [2, 3]
        assert sorted(c.search_vector_field("f", q, 3, subset=[3]).ids().tolist()) == []             # the second row of id 2 maps to no field row
        assert sorted(c.search_vector_field("f", q, 3, subset=[1]).ids().tolist()) == [2]
    with pytest.raises(RuntimeError, match="stored in more than one row"):
        c.update_items(np.ones((1, DIM0), np.float32), [2])
