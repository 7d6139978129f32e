"""Field filters (`where=`): the reference's closed filter dialect, typed field columns, and the device filter.

The reference answers a `where` string from an in-memory index when the string is one of the four forms of
`FieldStore::query_from_index` (src/storage/field_store.rs:1527-1590) and hands everything else to third-party SQL (ApexBase).  This
module is that dialect and nothing more:

    parse_where         the parsers of field_store.rs:2016-2335, function for function, including what they ignore
    FieldTable          the host copy of the fields: per field a one-byte tag and an 8-byte payload per row, row-aligned with the shard
                        (pending rows included); it is authoritative, and evaluates a predicate itself for the pending rows
    FieldFilter         `lynse_hip_fields`: the device copy of the columns a filter names, uploaded whole and lazily, and k_field_filter

THE CONTRACT (include/lynse_hip.h FIELD FILTERS has the device half)
  Forms, tried in this order:  1. `field IN (v1, v2, ...)`   2. `field = v1 OR field = v2 ...` on one field   3. `f1 = v1 OR f2 = v2 ...`
  4. `c1 AND c2 AND ...`, each c one of `field = v`, `field >= | <= | > | < v`, `field CONTAINS v`.  Anything else — `!=`, LIKE, NOT,
  parentheses, function calls, an IN inside a conjunction — is NotImplementedError (it would need ApexBase SQL).
  Values (IndexKey::from_json / insert_value): missing | Null | Bool | Int (an integer that fits i64) | Float (any other number; the key is
  normalize_f64_bits, so -0.0 and +0.0 differ) | Str | an array (indexed by CONTAINS only: scalars element-wise, nested arrays and
  objects skipped) | an object (never matched).  Equality is equality of keys of ONE variant: `x = 1` does not match a stored 1.0,
  `x = null` matches a stored null and not a missing field.
  Range (get_range's BTreeMap path): Int and Float compare as f64 through the normalised bits (an integer beyond 2^53 rounds as `as f64`
  rounds it), text compares bytewise (UTF-8), every Number sorts before every Text (`x > 5` returns the rows whose x is a string too);
  Null, Bool, missing, arrays and objects never pass a range.
  This build's own rules (the reference answers these through SQL):
    - a field no row carries matches nothing;
    - the reference's index limits (cardinality blacklist, "unstructured text" fields, a cold index) do not exist: every field is
      answered by the rules above;
    - at most 32 leaves per expression and 65,536 keys per IN / OR list, NotImplementedError beyond;
    - a non-finite float (JSON has none) is stored as Null; a value of any other Python type is stored as an object.
"""
from __future__ import annotations

import ctypes as C
import re
import struct
from typing import Optional

import numpy as np

TAG_MISSING, TAG_NULL, TAG_BOOL, TAG_INT, TAG_FLOAT, TAG_STR, TAG_ARRAY, TAG_OBJECT = range(8)
LEAF_EQ, LEAF_NUM_RANGE, LEAF_KEYSET, LEAF_STRTABLE, LEAF_CONTAINS = range(5)
OP_LT, OP_LE, OP_GT, OP_GE = range(4)
MAX_LEAVES = 32
MAX_KEYS = 65536
NO_COLUMN = 0xFFFFFFFF

_SQL_NEEDED = "this `where` expression is outside the indexed dialect (field_store.rs query_from_index) and would need ApexBase SQL: "

# char::is_whitespace (Unicode White_Space)
_WS = frozenset(map(chr, [*range(0x09, 0x0E), 0x20, 0x85, 0xA0, 0x1680, *range(0x2000, 0x200B), 0x2028, 0x2029, 0x202F, 0x205F, 0x3000]))
_I64_RE = re.compile(r"[+-]?[0-9]+\Z")
_F64_RE = re.compile(r"[+-]?(?:inf|infinity|nan|(?:[0-9]+\.?[0-9]*|\.[0-9]+)(?:[eE][+-]?[0-9]+)?)\Z", re.IGNORECASE)


def _trim_start(s: str) -> str:
    i = 0
    while i < len(s) and s[i] in _WS:
        i += 1
    return s[i:]


def _trim(s: str) -> str:
    s = _trim_start(s)
    j = len(s)
    while j > 0 and s[j - 1] in _WS:
        j -= 1
    return s[:j]


def normalize_f64_bits(f: float) -> int:
    """field_store.rs:223-230: the unsigned order of the result is the numeric order, -0.0 before +0.0."""
    bits = struct.unpack("<Q", struct.pack("<d", f))[0]
    return bits | (1 << 63) if bits >> 63 == 0 else bits ^ 0xFFFFFFFFFFFFFFFF


def _parse_i64(s: str) -> Optional[int]:
    if _I64_RE.match(s):
        v = int(s)
        if -(1 << 63) <= v < (1 << 63):
            return v
    return None


def _parse_f64(s: str) -> Optional[float]:
    return float(s) if _F64_RE.match(s) else None   # (str::parse::<f64>: no underscores, no surrounding blanks; overflow gives inf)


# ---- the parsers of field_store.rs:2016-2335 ------------------------------------------------------------------------------------
def parse_field_ref(expr: str):
    expr = _trim_start(expr)
    if expr[:1] in ('"', "`"):
        close = expr.find(expr[0], 1)
        if close < 0:
            return None
        return expr[1:close], _trim_start(expr[close + 1:])
    if not expr or not (expr[0] == "_" or (expr[0].isascii() and expr[0].isalpha())):
        return None
    end = 1
    while end < len(expr) and (expr[end] == "_" or (expr[end].isascii() and expr[end].isalnum())):
        end += 1
    return expr[:end], _trim_start(expr[end:])


def starts_with_keyword(value: str, keyword: str) -> bool:
    value = _trim_start(value)
    head = value[:len(keyword)]
    if len(head) < len(keyword) or not head.isascii() or head.upper() != keyword.upper():
        return False
    return len(value) == len(keyword) or value[len(keyword)] in _WS


def extract_value_literal(value: str) -> Optional[str]:
    """A quoted literal ends at its closing quote, an unquoted one at the first whitespace; what follows is dropped."""
    value = _trim(value)
    if not value:
        return None
    if value[0] in ('"', "'"):
        end = value.find(value[0], 1)
        return None if end < 0 else value[:end + 1]
    for i, ch in enumerate(value):
        if ch in _WS:
            return value[:i]
    return value


def unquote_token(value: str) -> str:
    value = _trim(value)
    if len(value) >= 2 and ((value[0] == '"' and value[-1] == '"') or (value[0] == "'" and value[-1] == "'")):
        return value[1:-1]
    return value


def _split_outside_quotes(expr: str, word: Optional[str]) -> list:
    """split_on_and / split_on_or (word = "AND" / "OR": ` word ` with single spaces, any letter case) and split_csv_tokens
    (word = None: commas, empty tokens dropped) — outside double quotes, single quotes and backticks."""
    parts, start, i = [], 0, 0
    dq = sq = bt = False
    n, w = len(expr), 0 if word is None else len(word)
    while i < n:
        ch = expr[i]
        if ch == '"' and not sq and not bt:
            dq = not dq
        elif ch == "'" and not dq and not bt:
            sq = not sq
        elif ch == "`" and not dq and not sq:
            bt = not bt
        elif not dq and not sq and not bt:
            if word is None:
                if ch == ",":
                    tok = _trim(expr[start:i])
                    if tok:
                        parts.append(tok)
                    start = i + 1
            elif ch == " " and i + w + 2 <= n and expr[i + w + 1] == " " and expr[i + 1:i + 1 + w].isascii() and expr[i + 1:i + 1 + w].upper() == word:
                parts.append(_trim(expr[start:i]))
                i += w + 2
                start = i
                continue
        i += 1
    tail = _trim(expr[start:])
    if word is not None or tail:
        parts.append(tail)
    return parts


def split_on_and(expr: str) -> list:
    return _split_outside_quotes(expr, "AND")


def split_on_or(expr: str) -> list:
    return _split_outside_quotes(expr, "OR")


def split_csv_tokens(values: str) -> list:
    return _split_outside_quotes(values, None)


def index_key_from_token(s: str):
    """IndexKey::from_token -> (tag, value) or None: quoted = Str, true / false / null in any case, an i64, else an f64."""
    if len(s) >= 2 and ((s[0] == '"' and s[-1] == '"') or (s[0] == "'" and s[-1] == "'")):
        return (TAG_STR, s[1:-1])
    low = s.lower()
    if low == "true":
        return (TAG_BOOL, 1)
    if low == "false":
        return (TAG_BOOL, 0)
    if low == "null":
        return (TAG_NULL, 0)
    i = _parse_i64(s)
    if i is not None:
        return (TAG_INT, i)
    f = _parse_f64(s)
    if f is not None:
        return (TAG_FLOAT, normalize_f64_bits(f))
    return None


def range_key_from_token(s: str):
    """RangeKey::from_token -> ("num", bits) | ("text", str): the unquoted token is a Number when it parses as a finite f64."""
    token = unquote_token(s)
    f = _parse_f64(token)
    if f is not None and f == f and f not in (float("inf"), float("-inf")):
        return ("num", normalize_f64_bits(f))
    return ("text", token)


def parse_equality_condition(expr: str):
    ref = parse_field_ref(_trim(expr))
    if ref is None:
        return None
    field, rest = ref
    if not rest.startswith("="):
        return None
    lit = extract_value_literal(_trim(rest[1:]))
    key = None if lit is None else index_key_from_token(lit)
    return None if key is None else (field, key)


def parse_indexed_in(expr: str):
    ref = parse_field_ref(_trim(expr))
    if ref is None:
        return None
    field, rest = ref
    if not starts_with_keyword(rest, "IN"):
        return None
    values = _trim(rest[2:])
    if not values.startswith("(") or not values.endswith(")"):
        return None
    inner = _trim(values[1:-1])
    if not inner:
        return None
    keys = []
    for token in split_csv_tokens(inner):
        key = index_key_from_token(_trim(token))
        if key is None:
            return None
        keys.append(key)
    return field, keys


def parse_indexed_or_equalities(expr: str):
    parts = split_on_or(expr)
    if len(parts) < 2:
        return None
    name, keys = None, []
    for part in parts:
        cond = parse_equality_condition(part)
        if cond is None or (name is not None and cond[0] != name):
            return None
        name = cond[0]
        keys.append(cond[1])
    return name, keys


def parse_indexed_or_leaves(expr: str):
    parts = split_on_or(expr)
    if len(parts) < 2:
        return None
    leaves = []
    for part in parts:
        cond = parse_equality_condition(part)
        if cond is None:
            return None
        leaves.append(cond)
    return leaves


def parse_single_indexed_condition(expr: str):
    ref = parse_field_ref(_trim(expr))
    if ref is None:
        return None
    field, rest = ref
    if starts_with_keyword(rest, "CONTAINS"):
        lit = extract_value_literal(_trim(rest[len("CONTAINS"):]))
        key = None if lit is None else index_key_from_token(lit)
        return None if key is None else Leaf(LEAF_CONTAINS, field, key=key)
    for token, op in ((">=", OP_GE), ("<=", OP_LE), (">", OP_GT), ("<", OP_LT)):
        if rest.startswith(token):
            lit = extract_value_literal(_trim(rest[len(token):]))
            return None if lit is None else Leaf(LEAF_NUM_RANGE, field, op=op, rkey=range_key_from_token(lit))
    if rest.startswith("="):   # plain `=` only (`!=` does not start with it, `>=` / `<=` were taken above)
        lit = extract_value_literal(_trim(rest[1:]))
        key = None if lit is None else index_key_from_token(lit)
        return None if key is None else Leaf(LEAF_EQ, field, key=key)
    return None


def parse_indexed_where(expr: str):
    conds = []
    for part in split_on_and(expr):
        c = parse_single_indexed_condition(part)
        if c is None:
            return None
        conds.append(c)
    return conds or None


class Leaf:
    """One condition.  kind LEAF_EQ / LEAF_CONTAINS: key = (tag, value); LEAF_KEYSET: keys = [(tag, value), ...];
    LEAF_NUM_RANGE: op and rkey = ("num", bits) | ("text", str) (a text literal becomes a string table when compiled for a column)."""
    __slots__ = ("kind", "field", "key", "keys", "op", "rkey")

    def __init__(self, kind: int, field: str, key=None, keys=None, op: int = 0, rkey=None):
        self.kind, self.field, self.key, self.keys, self.op, self.rkey = kind, field, key, keys, op, rkey

    def __repr__(self) -> str:
        return f"Leaf(kind={self.kind}, field={self.field!r}, key={self.key!r}, keys={self.keys!r}, op={self.op}, rkey={self.rkey!r})"


class Predicate:
    """A compiled `where`: `any` = False for the AND of the leaves, True for their OR."""
    __slots__ = ("expr", "any", "leaves")

    def __init__(self, expr: str, any_: bool, leaves: list):
        self.expr, self.any, self.leaves = expr, any_, leaves

    def fields(self) -> list:
        return sorted({l.field for l in self.leaves})


def parse_where(expr) -> Predicate:
    """The forms in the order of query_from_index; NotImplementedError for everything the reference would hand to ApexBase SQL."""
    if isinstance(expr, Predicate):
        return expr
    if not isinstance(expr, str):
        raise TypeError("where must be a string")
    got = parse_indexed_in(expr) or parse_indexed_or_equalities(expr)
    if got is not None:
        field, keys = got
        if len(keys) > MAX_KEYS:
            raise NotImplementedError(f"a `where` list of {len(keys)} keys is beyond this build's limit of {MAX_KEYS} (it would need ApexBase SQL)")
        return Predicate(expr, False, [Leaf(LEAF_KEYSET, field, keys=keys)])
    leaves = parse_indexed_or_leaves(expr)
    any_ = leaves is not None
    if any_:
        leaves = [Leaf(LEAF_EQ, f, key=k) for f, k in leaves]
    else:
        leaves = parse_indexed_where(expr)
    if leaves is None:
        raise NotImplementedError(_SQL_NEEDED + repr(expr))
    if len(leaves) > MAX_LEAVES:
        raise NotImplementedError(f"a `where` expression of {len(leaves)} leaves is beyond this build's limit of {MAX_LEAVES} (it would need ApexBase SQL)")
    return Predicate(expr, any_, leaves)


# ---- the host copy of the fields ---------------------------------------------------------------------------------------------------
_U64 = 0xFFFFFFFFFFFFFFFF


def _norm_bits_array(f: np.ndarray) -> np.ndarray:
    b = np.ascontiguousarray(f, dtype=np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63) == 0, b | np.uint64(1 << 63), ~b)


class _Column:
    __slots__ = ("tags", "payloads", "strings", "codes", "arrays", "version")

    def __init__(self, cap: int):
        self.tags = np.zeros(cap, np.uint8)
        self.payloads = np.zeros(cap, np.uint64)
        self.strings: list = []      # code -> string
        self.codes: dict = {}        # string -> code
        self.arrays: dict = {}       # row -> (element tags u8[], element payloads u64[])
        self.version = 0

    def code(self, s: str) -> int:
        c = self.codes.get(s)
        if c is None:
            c = self.codes[s] = len(self.strings)
            self.strings.append(s)
        return c

    def scalar(self, v):
        """(tag, payload) of a scalar by IndexKey::from_json, None for an array or an object."""
        if v is None:
            return TAG_NULL, 0
        if isinstance(v, (bool, np.bool_)):
            return TAG_BOOL, int(bool(v))
        if isinstance(v, (int, np.integer)):
            v = int(v)
            if -(1 << 63) <= v < (1 << 63):
                return TAG_INT, v & _U64
            try:
                return TAG_FLOAT, normalize_f64_bits(float(v))   # as_i64 fails: the number is its f64
            except OverflowError:
                return TAG_NULL, 0
        if isinstance(v, (float, np.floating)):
            v = float(v)
            if v != v or v in (float("inf"), float("-inf")):
                return TAG_NULL, 0
            return TAG_FLOAT, normalize_f64_bits(v)
        if isinstance(v, str):
            return TAG_STR, self.code(v)
        return None

    def put(self, row: int, v) -> None:
        self.arrays.pop(row, None)
        s = self.scalar(v)
        if s is not None:
            self.tags[row], self.payloads[row] = s[0], s[1]
        elif isinstance(v, (list, tuple, np.ndarray)):
            elems = [e for e in (self.scalar(x) for x in (v.tolist() if isinstance(v, np.ndarray) else v)) if e is not None]
            self.tags[row], self.payloads[row] = TAG_ARRAY, 0
            self.arrays[row] = (np.array([e[0] for e in elems], np.uint8), np.array([e[1] for e in elems], np.uint64))
        else:
            self.tags[row], self.payloads[row] = TAG_OBJECT, 0

    def clear(self, row: int) -> None:
        self.arrays.pop(row, None)
        self.tags[row], self.payloads[row] = TAG_MISSING, 0


class FieldTable:
    """Per field a tag and a payload per row (`Str`: a code into the field's dictionary; arrays: their elements on the side), row-aligned
    with the shard, pending rows included.  Every change of a column bumps its version: the device copy follows lazily."""

    def __init__(self):
        self.n = 0
        self._cap = 0
        self.cols: dict = {}      # name -> _Column
        self.ids: dict = {}       # name -> column id on the device, in order of first sight

    def _grow(self, need: int) -> None:
        if need <= self._cap:
            return
        cap = max(need, 2 * self._cap, 1024)
        for c in self.cols.values():
            c.tags = np.concatenate([c.tags, np.zeros(cap - c.tags.size, np.uint8)])
            c.payloads = np.concatenate([c.payloads, np.zeros(cap - c.payloads.size, np.uint64)])
        self._cap = cap

    def _col(self, name: str) -> _Column:
        c = self.cols.get(name)
        if c is None:
            c = self.cols[name] = _Column(self._cap)
            self.ids[name] = len(self.ids)
        return c

    def append(self, fields, count: int) -> None:
        """`count` rows; fields = None (every field missing) or one dict per row."""
        first = self.n
        self._grow(first + count)
        self.n = first + count
        if fields is None:
            return
        for j, f in enumerate(fields):
            for name, v in f.items():
                c = self._col(str(name))
                c.put(first + j, v)
                c.version += 1

    def append_columns(self, count: int, columns: dict) -> None:
        """`count` rows given column-wise: name -> an integer array (Int) or a floating array of finite values (Float), one entry per row.
        Fields not named are missing in these rows.  The bulk form of `append` for numeric fields."""
        arrays = {}
        for name, a in columns.items():
            a = np.asarray(a).reshape(-1)
            if a.size != count or a.dtype.kind not in "iuf" or (a.dtype.kind == "f" and not np.isfinite(a).all()):
                raise ValueError("append_columns takes one integer or finite floating entry per row")
            if a.dtype.kind == "u" and a.size and int(a.max()) >= (1 << 63):
                raise ValueError("append_columns: an integer beyond i64 is a Float; pass it as one")
            arrays[str(name)] = a
        first = self.n
        self._grow(first + count)
        self.n = first + count
        for name, a in arrays.items():
            c = self._col(name)
            if a.dtype.kind == "f":
                c.tags[first:self.n], c.payloads[first:self.n] = TAG_FLOAT, _norm_bits_array(a)
            else:
                c.tags[first:self.n], c.payloads[first:self.n] = TAG_INT, a.astype(np.int64).view(np.uint64)
            c.version += 1

    def set_row(self, row: int, fields: dict) -> None:
        """The row's fields are replaced: every field it carried is dropped first."""
        for c in self.cols.values():
            if c.tags[row] != TAG_MISSING:
                c.clear(row)
                c.version += 1
        for name, v in fields.items():
            c = self._col(str(name))
            c.put(row, v)
            c.version += 1

    def keep(self, keep: np.ndarray) -> None:
        """Compaction: new row j is the j-th kept old row."""
        keep = np.asarray(keep, dtype=bool)
        assert keep.size == self.n
        new_of = np.cumsum(keep) - 1
        m = int(np.count_nonzero(keep))
        for c in self.cols.values():
            c.tags = np.concatenate([c.tags[:self.n][keep], np.zeros(self._cap - m, np.uint8)])
            c.payloads = np.concatenate([c.payloads[:self.n][keep], np.zeros(self._cap - m, np.uint64)])
            c.arrays = {int(new_of[r]): a for r, a in c.arrays.items() if keep[r]}
            c.version += 1
        self.n = m

    def take(self, rows) -> "FieldTable":
        """A new table whose row j is row rows[j] of this one (a row may be taken any number of times); the dictionaries are shared."""
        rows = np.asarray(rows, dtype=np.int64).reshape(-1)
        t = FieldTable()
        t.n = t._cap = int(rows.size)
        t.ids = dict(self.ids)
        for name, c in self.cols.items():
            d = t.cols[name] = _Column(0)
            d.tags, d.payloads = c.tags[rows], c.payloads[rows]
            d.strings, d.codes = c.strings, c.codes
            if c.arrays:
                for j in np.nonzero(d.tags == TAG_ARRAY)[0].tolist():
                    d.arrays[j] = c.arrays[int(rows[j])]
        return t

    # -- the host evaluator (the pending rows; the device evaluates the same leaves for the flushed ones) ----------------------------
    def _strtable(self, c: _Column, op: int, text: str) -> np.ndarray:
        lit = text.encode("utf-8", "surrogatepass")
        out = np.zeros(len(c.strings), bool)
        for code, s in enumerate(c.strings):
            b = s.encode("utf-8", "surrogatepass")
            out[code] = b < lit if op == OP_LT else b <= lit if op == OP_LE else b > lit if op == OP_GT else b >= lit
        return out

    def _key(self, c: _Column, key):
        """(tag, payload) of a literal key against the column's dictionary; None for a string the column has never seen."""
        tag, v = key
        if tag == TAG_STR:
            code = c.codes.get(v)
            return None if code is None else (TAG_STR, code)
        return tag, v & _U64

    def _leaf_rows(self, leaf: Leaf, lo: int, hi: int) -> np.ndarray:
        c = self.cols.get(leaf.field)
        if c is None:
            return np.zeros(hi - lo, bool)
        tags, pay = c.tags[lo:hi], c.payloads[lo:hi]
        if leaf.kind == LEAF_EQ:
            k = self._key(c, leaf.key)
            return np.zeros(hi - lo, bool) if k is None else (tags == k[0]) & (pay == np.uint64(k[1]))
        if leaf.kind == LEAF_KEYSET:
            out = np.zeros(hi - lo, bool)
            by_tag: dict = {}
            for key in leaf.keys:
                k = self._key(c, key)
                if k is not None:
                    by_tag.setdefault(k[0], []).append(k[1])
            for tag, vals in by_tag.items():
                out |= (tags == tag) & np.isin(pay, np.array(vals, np.uint64))
            return out
        if leaf.kind == LEAF_NUM_RANGE:
            kind, v = leaf.rkey
            is_num, is_str = (tags == TAG_INT) | (tags == TAG_FLOAT), tags == TAG_STR
            if kind == "num":
                bits = np.where(tags == TAG_FLOAT, pay, _norm_bits_array(pay.view(np.int64).astype(np.float64)))
                lit = np.uint64(v)
                cmp_ = bits < lit if leaf.op == OP_LT else bits <= lit if leaf.op == OP_LE else bits > lit if leaf.op == OP_GT else bits >= lit
                return (is_num & cmp_) | (is_str & (leaf.op >= OP_GT))
            table = self._strtable(c, leaf.op, v)
            out = is_num & (leaf.op <= OP_LE)
            if table.size:
                out = out | (is_str & table[np.where(is_str, pay, 0).astype(np.int64)])
            return out
        if leaf.kind == LEAF_CONTAINS:
            out = np.zeros(hi - lo, bool)
            k = self._key(c, leaf.key)
            if k is not None:
                for r, (et, ep) in c.arrays.items():
                    if lo <= r < hi and bool(np.any((et == k[0]) & (ep == np.uint64(k[1])))):
                        out[r - lo] = True
            return out
        raise ValueError("unknown leaf kind")

    def evaluate(self, pred: Predicate, lo: int = 0, hi: Optional[int] = None) -> np.ndarray:
        """bool[hi - lo]: which of the rows lo .. hi - 1 the predicate selects."""
        hi = self.n if hi is None else hi
        out = np.zeros(hi - lo, bool) if pred.any else np.ones(hi - lo, bool)
        for leaf in pred.leaves:
            m = self._leaf_rows(leaf, lo, hi)
            out = (out | m) if pred.any else (out & m)
        return out

    # -- what the device needs ---------------------------------------------------------------------------------------------------
    def device_column(self, name: str, n: int):
        """The first n rows of a column in the layout of lynse_hip_fields_set_column: tags, payloads (an array row's payload is its
        index into arr_ptr), arr_ptr, element tags, element payloads."""
        c = self.cols[name]
        tags, pay = np.ascontiguousarray(c.tags[:n]), c.payloads[:n].copy()
        rows = sorted(r for r in c.arrays if r < n)
        ptr = np.zeros(len(rows) + 1, np.uint64)
        if rows:
            np.cumsum([c.arrays[r][0].size for r in rows], out=ptr[1:])
            pay[np.array(rows, np.int64)] = np.arange(len(rows), dtype=np.uint64)
        et = np.concatenate([c.arrays[r][0] for r in rows]) if rows else np.zeros(0, np.uint8)
        ep = np.concatenate([c.arrays[r][1] for r in rows]) if rows else np.zeros(0, np.uint64)
        return tags, pay, ptr, np.ascontiguousarray(et, dtype=np.uint8), np.ascontiguousarray(ep, dtype=np.uint64)

    def device_program(self, pred: Predicate):
        """-> (leaves as _lib.FieldLeaf array, aux u64[]): the leaves against the columns' dictionaries and ids."""
        from ._lib import FieldLeaf

        out = (FieldLeaf * len(pred.leaves))()
        aux: list = []
        off = 0
        never = (LEAF_EQ, NO_COLUMN, 0, 0, TAG_OBJECT, 0, 0, 0)   # matches nothing
        for i, leaf in enumerate(pred.leaves):
            c = self.cols.get(leaf.field)
            col = self.ids.get(leaf.field, NO_COLUMN)
            kind, op, flags, key_tag, key, a_off, a_len = leaf.kind, 0, 0, 0, 0, 0, 0
            if c is None:
                kind, col, op, flags, key_tag, key, a_off, a_len = never
            elif leaf.kind in (LEAF_EQ, LEAF_CONTAINS):
                k = self._key(c, leaf.key)
                if k is None:
                    kind, col, op, flags, key_tag, key, a_off, a_len = never
                else:
                    key_tag, key = k
            elif leaf.kind == LEAF_KEYSET:
                by_tag: dict = {}
                for lk in leaf.keys:
                    k = self._key(c, lk)
                    if k is not None:
                        by_tag.setdefault(k[0], set()).add(k[1])
                starts, vals = [0], []
                for tag in range(8):
                    vals.extend(sorted(by_tag.get(tag, ())))
                    starts.append(len(vals))
                block = np.array(starts + vals, dtype=np.uint64)
                a_off, a_len = off, len(vals)
                aux.append(block)
                off += block.size
            elif leaf.rkey[0] == "num":
                op, key = leaf.op, leaf.rkey[1]
            else:
                table = self._strtable(c, leaf.op, leaf.rkey[1])
                bits = np.zeros((table.size + 63) // 64 * 64, np.uint8)
                bits[:table.size] = table
                block = np.packbits(bits, bitorder="little").view(np.uint64) if bits.size else np.zeros(0, np.uint64)
                kind, flags, a_off, a_len = LEAF_STRTABLE, int(leaf.op <= OP_LE), off, table.size
                aux.append(block)
                off += block.size
            out[i] = FieldLeaf(kind, col, op, flags, key_tag, 0, key, a_off, a_len)
        return out, (np.ascontiguousarray(np.concatenate(aux), dtype=np.uint64) if aux else np.zeros(0, np.uint64))


# ---- the device filter -----------------------------------------------------------------------------------------------------------
class FieldFilter:
    """`lynse_hip_fields`: the device copy of the columns, uploaded whole by the first filter that names a column after it changed (or
    after the number of flushed rows changed), and k_field_filter over them."""

    def __init__(self, device: Optional[int] = None):
        from ._lib import check, lib
        from .core import default_device

        self._h = C.c_void_p()
        self._uploaded: dict = {}   # column id -> (version, rows)
        self.last_kernel_us = 0.0
        check(lib.lynse_hip_fields_create(default_device() if device is None else int(device), C.byref(self._h)))

    def __del__(self):
        from ._lib import lib

        if getattr(self, "_h", None) is not None and self._h:
            lib.lynse_hip_fields_destroy(self._h)
            self._h = None

    @property
    def handle(self):
        return self._h

    def hbm_bytes(self) -> int:
        from ._lib import lib

        return int(lib.lynse_hip_fields_hbm_bytes(self._h))

    def set_column(self, column: int, tags, payloads, arr_ptr=None, elem_tags=None, elem_payloads=None) -> None:
        """One column in the layout of lynse_hip_fields_set_column (the low-level entry: Collection goes through `filter`)."""
        from ._lib import check, lib

        tags = np.ascontiguousarray(tags, dtype=np.uint8)
        payloads = np.ascontiguousarray(payloads, dtype=np.uint64)
        if tags.size != payloads.size:
            raise ValueError("tags and payloads must have one entry per row")
        ptr = np.zeros(1, np.uint64) if arr_ptr is None else np.ascontiguousarray(arr_ptr, dtype=np.uint64)
        et = np.zeros(0, np.uint8) if elem_tags is None else np.ascontiguousarray(elem_tags, dtype=np.uint8)
        ep = np.zeros(0, np.uint64) if elem_payloads is None else np.ascontiguousarray(elem_payloads, dtype=np.uint64)
        if et.size != ep.size or (ptr.size and int(ptr[-1]) != et.size):
            raise ValueError("arr_ptr must end at the number of elements")
        vp = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None   # noqa: E731
        check(lib.lynse_hip_fields_set_column(self._h, int(column), vp(tags), vp(payloads), tags.size, vp(ptr) if ptr.size > 1 else None,
                                              ptr.size - 1 if ptr.size > 1 else 0, vp(et), vp(ep)))
        self._uploaded.pop(int(column), None)

    def run(self, n: int, any_: bool, leaves, aux: np.ndarray) -> int:
        """lynse_hip_fields_filter over rows 0 .. n - 1 -> the match count; the words stay on the device."""
        from ._lib import check, lib

        count, us = C.c_uint64(0), C.c_float(0.0)
        aux = np.ascontiguousarray(aux, dtype=np.uint64)
        check(lib.lynse_hip_fields_filter(self._h, int(n), 1 if any_ else 0, C.cast(leaves, C.c_void_p), len(leaves),
                                          aux.ctypes.data_as(C.c_void_p) if aux.size else None, aux.size, C.byref(count), C.byref(us)))
        self.last_kernel_us = float(us.value)
        return int(count.value)

    def upload(self, table: FieldTable, names, n: int) -> None:
        """The first n rows of the named columns of `table`, each uploaded whole if it changed since its last upload."""
        for name in names:
            c = table.cols.get(name)
            if c is None:
                continue
            col = table.ids[name]
            if self._uploaded.get(col) != (id(table), c.version, n):
                self.set_column(col, *table.device_column(name, n))
                self._uploaded[col] = (id(table), c.version, n)

    def filter(self, table: FieldTable, pred: Predicate, n: int) -> int:
        """The predicate over the first n rows of `table`: uploads the columns that changed, runs the kernel -> the match count."""
        self.upload(table, pred.fields(), n)
        leaves, aux = table.device_program(pred)
        return self.run(n, pred.any, leaves, aux)

    def words(self) -> np.ndarray:
        """The BitSet words of the last filter, read back."""
        from ._lib import check, lib

        ptr, nw = C.c_void_p(), C.c_uint64(0)
        check(lib.lynse_hip_fields_words_device(self._h, C.byref(ptr), C.byref(nw)))
        out = np.zeros(int(nw.value), np.uint64)
        check(lib.lynse_hip_fields_words(self._h, out.ctypes.data_as(C.c_void_p) if out.size else None, out.size))
        return out

    def words_device(self):
        """-> (device pointer, n_words) of the last filter's words, for FlatIndex.search_filtered_bitset_device_batch_arrays."""
        from ._lib import check, lib

        ptr, nw = C.c_void_p(), C.c_uint64(0)
        check(lib.lynse_hip_fields_words_device(self._h, C.byref(ptr), C.byref(nw)))
        return ptr, int(nw.value)
