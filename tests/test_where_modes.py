"""The `where=` dialect on the host (lynsedb_amd/fields.py): the parser against cases written out by hand — the strings of
the reference's own unit tests (src/storage/field_store.rs:2511-2598) among them — and the host evaluator (the one the pending rows go
through) against the per-row model of tests/fields_common.py.  No GPU."""
import numpy as np
import pytest

import fields_common as F
from lynsedb_amd import fields as W

INT, FLOAT, STR, BOOL, NULL = W.TAG_INT, W.TAG_FLOAT, W.TAG_STR, W.TAG_BOOL, W.TAG_NULL
nb = W.normalize_f64_bits


def leaves(expr):
    p = W.parse_where(expr)
    return p.any, [(l.kind, l.field, l.key, l.keys, l.op, l.rkey) for l in p.leaves]


def test_the_references_own_parser_strings():
    want = (False, [(W.LEAF_EQ, "status", (STR, "active"), None, 0, None), (W.LEAF_NUM_RANGE, "score", None, None, W.OP_GE, ("num", nb(10.0)))])
    assert leaves("status = 'active' AND score >= 10") == want
    assert leaves("`status` = 'active' AND `score` >= 10") == want
    assert leaves("\"status\" = 'active' AND \"score\" >= 10") == want
    assert leaves("city IN ('shanghai', \"beijing\", 42)") == (False, [(W.LEAF_KEYSET, "city", None, [(STR, "shanghai"), (STR, "beijing"), (INT, 42)], 0, None)])
    assert leaves("`city` IN ('a')") == (False, [(W.LEAF_KEYSET, "city", None, [(STR, "a")], 0, None)])
    assert leaves("city = 'shanghai' OR city = 'beijing'") == (False, [(W.LEAF_KEYSET, "city", None, [(STR, "shanghai"), (STR, "beijing")], 0, None)])
    assert leaves("city = 'shanghai' OR country = 'cn'") == (True, [(W.LEAF_EQ, "city", (STR, "shanghai"), None, 0, None),
                                                                     (W.LEAF_EQ, "country", (STR, "cn"), None, 0, None)])
    assert leaves("tags CONTAINS 'red' AND n < 3.5") == (False, [(W.LEAF_CONTAINS, "tags", (STR, "red"), None, 0, None),
                                                                  (W.LEAF_NUM_RANGE, "n", None, None, W.OP_LT, ("num", nb(3.5)))])


def test_quotes_keep_keywords_and_commas_together():
    assert leaves("name = 'x AND y' AND note = \"p OR q\"") == (False, [(W.LEAF_EQ, "name", (STR, "x AND y"), None, 0, None),
                                                                        (W.LEAF_EQ, "note", (STR, "p OR q"), None, 0, None)])
    assert leaves("name = 'p OR q' OR name = 'r'")[1][0][3] == [(STR, "p OR q"), (STR, "r")]
    assert leaves("x IN ('a, b', \"c,d\", 'e')")[1][0][3] == [(STR, "a, b"), (STR, "c,d"), (STR, "e")]
    assert leaves("`a AND b` = 1 AND c = 2") == (False, [(W.LEAF_EQ, "a AND b", (INT, 1), None, 0, None), (W.LEAF_EQ, "c", (INT, 2), None, 0, None)])
    assert W.split_on_and("a = 1 AND b = ' AND ' and c = 3") == ["a = 1", "b = ' AND '", "c = 3"]
    assert W.split_on_or("a = 1 or b = \" OR \" Or c = 3") == ["a = 1", "b = \" OR \"", "c = 3"]
    assert W.split_on_and("a = 1  AND  b = 2") == ["a = 1", "b = 2"]          # (the blanks around the keyword's single spaces are trimmed)
    assert W.split_on_and("a = 1\tAND\tb = 2") == ["a = 1\tAND\tb = 2"]          # a tab is not the separator
    assert W.split_csv_tokens(" 1, ,2,, '3,4' ,") == ["1", "2", "'3,4'"]


def test_keyword_case():
    assert leaves("a = 1 and b = 2") == leaves("a = 1 AND b = 2") == leaves("a = 1 aNd b = 2")
    assert leaves("a = 1 or b = 2") == leaves("a = 1 OR b = 2")
    assert leaves("a in (1, 2)") == leaves("a IN (1, 2)") == leaves("a In (1,2)")
    assert leaves("t contains 'x'") == leaves("t CONTAINS 'x'")
    assert leaves("a = TRUE")[1][0][2] == (BOOL, 1) and leaves("a = False")[1][0][2] == (BOOL, 0) and leaves("a = NULL")[1][0][2] == (NULL, 0)
    assert W.starts_with_keyword("  in (1)", "IN") and not W.starts_with_keyword("inner", "IN") and W.starts_with_keyword("IN", "IN")
    assert not W.starts_with_keyword("I", "IN")


def test_trailing_text_after_a_literal_is_dropped():
    assert leaves("a = 1 trailing words") == leaves("a = 1")
    assert leaves("a = 'x' trailing") == leaves("a = 'x'")
    assert leaves("a >= 5 or so AND b = 2") == leaves("a >= 5 AND b = 2")
    assert leaves("a = 1 OR b = 2 AND c = 3") == leaves("a = 1 OR b = 2")      # the OR forms come first; `AND c = 3` follows the literal 2
    assert leaves("a = 1 AND b = 2 OR c = 3") == leaves("a = 1 OR c = 3")
    # ... which makes these legal, as they are in the reference: an OR that is not an OR of equalities is text after the first literal,
    # and `<>` is `<` followed by the literal `>`
    assert leaves("a > 1 OR a < 0") == leaves("a > 1") and leaves("a = 1 OR b > 2") == leaves("a = 1")
    assert leaves("a <> 1") == (False, [(W.LEAF_NUM_RANGE, "a", None, None, W.OP_LT, ("text", ">"))])
    assert W.extract_value_literal("  12 rest") == "12" and W.extract_value_literal("'a b' rest") == "'a b'"
    assert W.extract_value_literal("'open") is None and W.extract_value_literal("   ") is None


def test_literal_typing():
    key = lambda lit: leaves(f"x = {lit}")[1][0][2]   # noqa: E731
    assert key("'1'") == (STR, "1") and key('"1"') == (STR, "1") and key("1") == (INT, 1) and key("1.0") == (FLOAT, nb(1.0))
    assert key("+7") == (INT, 7) and key("-7") == (INT, -7)
    assert key("true") == (BOOL, 1) and key("null") == (NULL, 0)
    assert key("1e3") == (FLOAT, nb(1000.0)) and key("1000") == (INT, 1000)
    assert key("9223372036854775807") == (INT, (1 << 63) - 1) and key("9223372036854775808") == (FLOAT, nb(float(1 << 63)))
    assert key("-0.0") == (FLOAT, nb(-0.0)) and key("0.0") == (FLOAT, nb(0.0)) and nb(-0.0) != nb(0.0) and nb(-0.0) < nb(0.0)
    assert key(".5") == (FLOAT, nb(0.5)) and key("5.") == (FLOAT, nb(5.0)) and key("inf") == (FLOAT, nb(float("inf")))
    assert key("''") == (STR, "")
    with pytest.raises(NotImplementedError):
        key("abc")          # neither quoted, nor a keyword, nor a number
    with pytest.raises(NotImplementedError):
        key("1_000")        # (Rust's parsers take no underscores)
    rk = lambda lit: leaves(f"x > {lit}")[1][0][5]   # noqa: E731
    assert rk("'abc'") == ("text", "abc") and rk("abc") == ("text", "abc")
    assert rk("'12'") == ("num", nb(12.0)) and rk("12") == ("num", nb(12.0)) and rk("1e3") == ("num", nb(1000.0))
    assert rk("inf") == ("text", "inf") and rk("1e400") == ("text", "1e400") and rk("nan") == ("text", "nan")   # a Number is finite
    assert rk("true") == ("text", "true")
    assert [leaves(f"x {op} 1")[1][0][4] for op in ("<", "<=", ">", ">=")] == [W.OP_LT, W.OP_LE, W.OP_GT, W.OP_GE]


def test_field_references():
    assert W.parse_field_ref("abc_1 = 2") == ("abc_1", "= 2") and W.parse_field_ref("_x>1") == ("_x", ">1")
    assert W.parse_field_ref("`my field` = 2") == ("my field", "= 2") and W.parse_field_ref('"q"=2') == ("q", "=2")
    assert W.parse_field_ref("1abc = 2") is None and W.parse_field_ref("`open = 2") is None and W.parse_field_ref("") is None
    assert W.parse_field_ref("é = 2") is None
    assert leaves("a=1 AND b>=2") == leaves("a = 1 AND b >= 2")


@pytest.mark.parametrize("expr", [
    "a != 1", "a LIKE 'x%'", "NOT a = 1", "(a = 1)", "(a = 1) AND b = 2", "lower(a) = 'x'", "a IN (1, 2) AND b = 3", "b = 3 AND a IN (1, 2)",
    "a IN (1) OR b IN (2)", "a IN ()", "a IN 1, 2", "a IN (1, x)", "a = ", "a", "", "   ", "= 1", "a == 1", "a = x",
    "a BETWEEN 1 AND 2", "a IS NULL", "a CONTAINS", "a = 1 AND ", "1 = a", "a = 1 AND b != 2", "a = 'open",
])
def test_refused_forms(expr):
    with pytest.raises(NotImplementedError, match="ApexBase SQL"):
        W.parse_where(expr)


def test_where_must_be_a_string():
    with pytest.raises(TypeError):
        W.parse_where(7)


def test_leaf_and_key_limits():
    assert len(W.parse_where(" AND ".join(f"f{i} = {i}" for i in range(32))).leaves) == 32
    with pytest.raises(NotImplementedError, match="32"):
        W.parse_where(" AND ".join(f"f{i} = {i}" for i in range(33)))
    assert len(W.parse_where(" OR ".join(f"f{i} = {i}" for i in range(32))).leaves) == 32
    with pytest.raises(NotImplementedError, match="32"):
        W.parse_where(" OR ".join(f"f{i} = {i}" for i in range(33)))
    assert len(W.parse_where("x IN (" + ", ".join(str(i) for i in range(65536)) + ")").leaves[0].keys) == 65536
    with pytest.raises(NotImplementedError, match="65536"):
        W.parse_where("x IN (" + ", ".join(str(i) for i in range(65537)) + ")")
    assert len(W.parse_where(" OR ".join(f"x = {i}" for i in range(40))).leaves[0].keys) == 40      # an OR list on ONE field is a key list


@pytest.fixture(scope="module")
def generated():
    """6,000 rows drawn from the pool of tests/fields_common.py (every pool row at least once, in shuffled order), ingested the way a
    Collection does it: several appends, one of them without fields."""
    rng = np.random.default_rng(25)
    pick = np.concatenate([rng.permutation(len(F.POOL)), rng.integers(0, len(F.POOL), 6000 - len(F.POOL))])
    rows = [F.POOL[i] for i in pick]
    t = W.FieldTable()
    for lo in range(0, 6000, 1500):
        t.append([r or {} for r in rows[lo:lo + 1500]], 1500)
    t.append(None, 17)
    return t, rows + [F.POOL[0]] * 17


def test_host_evaluator_matches_the_model(generated):
    t, rows = generated
    assert t.n == len(rows)
    index_of = {id(r): i for i, r in enumerate(F.POOL)}
    for name, expr, cond in F.expressions():
        got = t.evaluate(W.parse_where(expr))
        by_pool = [F.model_match(cond, r) for r in F.POOL]          # the model once per distinct row, then row by row
        want = [by_pool[index_of[id(r)]] for r in rows]
        assert got.tolist() == want, (name, expr, [i for i in range(len(rows)) if bool(got[i]) != want[i]][:5])
    # a sub-range of rows (what the pending rows of a collection are)
    p = W.parse_where("a >= 0 AND s > 'abc'")
    assert t.evaluate(p, 100, 4000).tolist() == t.evaluate(p).tolist()[100:4000]


def test_table_rows_follow_set_row_keep_and_take(generated):
    t0, rows = generated
    n = 300
    t = t0.take(np.arange(n))
    rows = list(rows[:n])
    exprs = [e for e in F.expressions() if not e[0].startswith("in 65536")]

    def check(what):
        for name, expr, cond in exprs:
            assert t.evaluate(W.parse_where(expr)).tolist() == [F.model_match(cond, r) for r in rows], (what, name)

    check("take")
    for r, f in ((5, {"a": 1, "t": ["x"]}), (6, {}), (7, {"s": "é", "newfield": 3}), (299, {"a": "abc"})):
        t.set_row(r, f)          # the row's fields are replaced, not merged
        rows[r] = f
    check("set_row")
    assert t.evaluate(W.parse_where("newfield = 3")).tolist() == [i == 7 for i in range(n)]
    keep = np.ones(n, bool)
    keep[[0, 5, 6, 100, 298]] = False
    t.keep(keep)
    rows = [r for i, r in enumerate(rows) if keep[i]]
    assert t.n == len(rows) == n - 5
    check("keep")
    t.append([{"a": 1}], 1)
    rows.append({"a": 1})
    check("append after keep")
    # the device layout of a column with arrays: an array row's payload indexes arr_ptr, the elements are its scalars in order
    tags, pay, ptr, et, ep = t.device_column("t", t.n)
    arr_rows = np.nonzero(tags == W.TAG_ARRAY)[0]
    assert pay[arr_rows].tolist() == list(range(arr_rows.size)) and ptr.size == arr_rows.size + 1 and int(ptr[-1]) == et.size == ep.size
    for j, r in enumerate(arr_rows.tolist()):
        scalars = [e for e in rows[r]["t"] if not isinstance(e, (list, dict))]
        assert int(ptr[j + 1] - ptr[j]) == len(scalars), (r, rows[r]["t"])
