"""Models for the named-vector-field tests.  No numpy in a decision.

    remap_model         the device mask remap as a per-bit loop over Python lists of ints: words in, words out, count
    field_search_model  a filtered field search over plain dicts: keep the allowed field rows (id -> allowed? from the per-row model of
                        tests/fields_common.py, minus the tombstones), order them by (distance, field row) with distances the caller
                        took from the oracle, cut to k, map the rows to user ids
"""
NONE = 0xFFFFFFFF


def bit(words, j):
    return (words[j >> 6] >> (j & 63)) & 1


def remap_model(row_of, src_words, n_src, tail_words=(), n_tail=0):
    """out bit r = source bit row_of[r]: from src below n_src, from tail at row_of[r] - n_src above it; NONE gives 0.
    -> (ceil(len(row_of) / 64) words as ints, the number of set bits)"""
    n_out = len(row_of)
    out = [0] * ((n_out + 63) // 64)
    count = 0
    for r, j in enumerate(row_of):
        if j == NONE:
            continue
        assert 0 <= j < n_src + n_tail, "the model is asked about a row the host checks refuse"
        b = bit(src_words, j) if j < n_src else bit(tail_words, j - n_src)
        if b:
            out[r >> 6] |= 1 << (r & 63)
            count += 1
    return out, count


def field_search_model(field_ids, dists, allowed, tombstones, k, ascending):
    """field_ids: field row -> user id (a list); dists: field row -> distance (floats, the oracle's); allowed: None = every id, or a
    dict / set of the user ids the filter lets through; tombstones: a set of user ids.  -> (ids, rows) of the best k allowed rows by
    (distance, field row); inner product (ascending = False) ranks the larger score first."""
    rows = [r for r, i in enumerate(field_ids) if i not in tombstones and (allowed is None or i in allowed)]
    rows.sort(key=lambda r: ((dists[r] if ascending else -dists[r]), r))
    rows = rows[:k]
    return [field_ids[r] for r in rows], rows
