"""A per-row model of the `where=` dialect (lynsedb_amd/fields.py THE CONTRACT) for the field-filter tests.

Independent of the library: no parser (an expression is built from the helpers below, which give the `where` string AND the structure the
model reads), no columns, no normalised bits and no numpy in the decision — a dict in, a bool out.  A literal is typed from its text, a
value from its Python type, and the key and order rules are applied directly.
"""
import math
import re

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


# ---- expressions: (where string, model structure) ------------------------------------------------------------------------------
def eq(field, lit):
    return f"{field} = {lit}", ("eq", field, lit)


def rng(field, op, lit):
    assert op in ("<", "<=", ">", ">=")
    return f"{field} {op} {lit}", ("range", field, op, lit)


def contains(field, lit):
    return f"{field} CONTAINS {lit}", ("contains", field, lit)


def in_(field, lits):
    return f"{field} IN ({', '.join(lits)})", ("in", field, [key_of_literal(l) for l in lits])


def all_of(*conds):
    return " AND ".join(c[0] for c in conds), ("and", [c[1] for c in conds])


def any_of(*conds):
    return " OR ".join(c[0] for c in conds), ("or", [c[1] for c in conds])


# ---- typing ---------------------------------------------------------------------------------------------------------------------
def _float_key(f):
    return ("float", f, math.copysign(1.0, f))   # -0.0 and +0.0 are different keys; no NaN among the values or literals of the tests


def key_of_literal(lit):
    """IndexKey::from_token: quoted = Str; true / false / null; an integer that fits i64 = Int; any other number = Float."""
    if len(lit) >= 2 and lit[0] == lit[-1] and lit[0] in "'\"":
        return ("str", lit[1:-1])
    low = lit.lower()
    if low in ("true", "false"):
        return ("bool", low == "true")
    if low == "null":
        return ("null",)
    if re.fullmatch(r"[+-]?[0-9]+", lit) and I64_MIN <= int(lit) <= I64_MAX:
        return ("int", int(lit))
    return _float_key(float(lit))


def key_of_value(v):
    """IndexKey::from_json for a scalar; None for an array or an object."""
    if v is None:
        return ("null",)
    if isinstance(v, bool):
        return ("bool", v)
    if isinstance(v, int):
        return ("int", v) if I64_MIN <= v <= I64_MAX else _float_key(float(v))
    if isinstance(v, float):
        return _float_key(v)
    if isinstance(v, str):
        return ("str", v)
    return None


def _num_before(a, b):
    """a sorts strictly before b as f64 by the normalised bits: numeric order, -0.0 before +0.0"""
    return a < b or (a == b and math.copysign(1.0, a) < math.copysign(1.0, b))


def _range(value, op, lit):
    """get_range's BTreeMap path over RangeKey: Number(f64) < Text(bytes); Null, Bool, arrays, objects and missing never pass."""
    if isinstance(value, bool) or value is None or isinstance(value, (list, tuple, dict)):
        return False
    unq = lit[1:-1] if len(lit) >= 2 and lit[0] == lit[-1] and lit[0] in "'\"" else lit
    lit_key = ("text", unq.encode("utf-8"))   # RangeKey::from_token: a Number only when the unquoted token is a FINITE f64
    if re.fullmatch(r"[+-]?([0-9]+\.?[0-9]*|\.[0-9]+)([eE][+-]?[0-9]+)?", unq) and math.isfinite(float(unq)):
        lit_key = ("num", float(unq))
    val_key = ("text", value.encode("utf-8")) if isinstance(value, str) else ("num", float(value))
    if val_key[0] != lit_key[0]:
        before = val_key[0] == "num"          # every Number before every Text
        after = not before
    elif val_key[0] == "num":
        before, after = _num_before(val_key[1], lit_key[1]), _num_before(lit_key[1], val_key[1])
    else:
        before, after = val_key[1] < lit_key[1], val_key[1] > lit_key[1]
    same = not before and not after
    return {"<": before, "<=": before or same, ">": after, ">=": after or same}[op]


def model_match(cond, row) -> bool:
    """Does the row (a dict of fields, or None for a row added without fields) pass the condition?"""
    row = row or {}
    kind = cond[0]
    if kind == "and":
        return all(model_match(c, row) for c in cond[1])
    if kind == "or":
        return any(model_match(c, row) for c in cond[1])
    field = cond[1]
    if field not in row:
        return False
    v = row[field]
    if kind == "eq":
        k = key_of_value(v)
        return k is not None and k == key_of_literal(cond[2])
    if kind == "in":
        k = key_of_value(v)
        return k is not None and k in cond[2]
    if kind == "range":
        return _range(v, cond[2], cond[3])
    if kind == "contains":
        if not isinstance(v, (list, tuple)):
            return False
        want = key_of_literal(cond[2])
        return any(key_of_value(e) == want for e in v if not isinstance(e, (list, tuple, dict)))
    raise ValueError(kind)


# ---- the tables of the tests ---------------------------------------------------------------------------------------------------
P53 = 1 << 53

# hand-made rows: every value class of the contract, on the fields the expressions below name
POOL = [
    None,                                                       # a row added without fields
    {},
    {"a": 0, "s": "abc", "t": [], "m": 1, "z": 0.0},
    {"a": 1, "s": "abd", "t": ["x"], "m": 1.0, "z": -0.0},
    {"a": -1, "s": "ab", "t": ["x", "x", "y"], "m": "1", "z": 0},
    {"a": 1.0, "s": "", "t": [["x"], "y"], "m": True, "z": 1e-300},
    {"a": 1.5, "s": "é", "t": [1, 1.0, "1", True, None], "m": None, "z": -1e-300},
    {"a": I64_MAX, "s": "日本", "t": [{"x": 1}, [1]], "m": {"k": 1}, "z": 5e-324},
    {"a": I64_MIN, "s": "z", "t": "x", "m": [1], "z": -5e-324},
    {"a": P53, "s": "Z", "t": [P53, P53 + 1], "m": "true", "z": 1},
    {"a": P53 + 1, "s": "abc ", "t": [0.0], "m": "null", "z": -1},
    {"a": P53 + 2, "s": "ABC", "t": [-0.0], "m": 0, "z": 2.5},
    {"a": -P53 - 1, "s": "12", "t": ["", "x y"], "m": False, "z": -2.5},
    {"a": float(P53), "s": 12, "t": [None], "m": "x", "z": "0"},
    {"a": 9007199254740993.0, "s": 12.5, "t": [True, False], "m": 2, "z": None},
    {"a": None, "s": None, "t": None, "m": -1, "z": True},
    {"a": True, "s": True, "t": [[], {}], "m": 1e3, "z": [0]},
    {"a": False, "s": ["abc"], "t": ["y"], "m": 1000, "z": {"z": 0}},
    {"a": "1", "s": {"s": "abc"}, "t": ["X"], "m": 1000.0},
    {"a": "abc", "s": "€uro", "m": 3},
    {"a": 1 << 64, "s": "😀", "m": 4},                          # beyond i64: the number is its f64
    {"a": -(1 << 70), "s": "abé", "m": 5},
    {"s": "abc"},
    {"a": 7},
    {"u0": 1, "u1": "x"},
]
for _i in range(40):                                            # filler: small integers, a few strings, short arrays
    POOL.append({"a": _i - 20, "s": "s%02d" % (_i % 7), "t": ["x", "y", _i % 3][: _i % 4], "m": _i % 5, "z": (_i - 20) / 4.0, "k": _i * 1637 % 65536})


def expressions():
    """(name, where string, model structure): the cases of the GPU filter test."""
    c = []

    def add(name, pair):
        c.append((name, pair[0], pair[1]))

    for lit in ("1", "1.0", "'1'", "true", "false", "null", "0", "0.0", "-0.0", "'abc'", "''", "1e3", "1000", str(I64_MAX), str(I64_MIN), str(P53),
                str(P53 + 1), "9007199254740992.0", "18446744073709551616"):
        add(f"a = {lit}", eq("a", lit))
        add(f"m = {lit}", eq("m", lit))
        add(f"z = {lit}", eq("z", lit))
    for op in ("<", "<=", ">", ">="):
        for lit in ("0", "0.0", "-0.0", "1", str(P53), str(P53 + 1), str(P53 + 2), str(I64_MAX), str(I64_MIN), "-1e-300", "5e-324", "1e400"):
            add(f"a {op} {lit}", rng("a", op, lit))
            add(f"z {op} {lit}", rng("z", op, lit))
        for lit in ("'abc'", "'é'", "'日本'", "''", "'Z'", "'€'", "12", "'12'", "12.5", "'zzz'"):
            add(f"s {op} {lit}", rng("s", op, lit))
    for lit in ("'x'", "'y'", "1", "1.0", "'1'", "true", "null", "0.0", "-0.0", "''", "'x y'", str(P53 + 1), "'nope'"):
        add(f"t CONTAINS {lit}", contains("t", lit))
    add("in 1", in_("a", ["1"]))
    add("in 2", in_("a", ["1", "'abc'"]))
    add("in mixed", in_("m", ["1", "1.0", "'1'", "true", "null", "'x'", "'never seen'", "1000.0"]))
    add("in 65536", in_("k", [str(i) for i in range(65536)]))
    add("in 65536 sparse", in_("k", [str(i * 3) for i in range(65536)]))
    add("and 1", all_of(rng("a", ">=", "0")))
    add("and 4", all_of(rng("a", ">=", "-5"), rng("a", "<", "12"), eq("m", "1"), contains("t", "'x'")))
    add("and 32", all_of(*[rng("a", ">=", str(-20 + i // 2)) if i % 2 == 0 else rng("z", "<=", str(10 - i // 4)) for i in range(32)]))
    add("or two fields", any_of(eq("a", "1"), eq("s", "'abc'")))
    add("or 32 fields", any_of(*[eq(("a", "m", "z", "s", "u1")[i % 5], ("1", "null", "0.0", "'é'", "'x'", str(i))[i % 6]) for i in range(32)]))
    add("or one field", any_of(eq("a", "1"), eq("a", "1.0"), eq("a", "'1'")))
    add("nobody eq", eq("nobody", "1"))
    add("nobody range", rng("nobody", ">", "0"))
    add("nobody contains", contains("nobody", "'x'"))
    add("nobody in", in_("nobody", ["1", "2"]))
    add("nobody and", all_of(eq("a", "1"), eq("nobody", "1")))
    add("nobody or", any_of(eq("a", "1"), eq("nobody", "1")))
    return c
