"""The planted one-column datasets of tests/selection_common.py against a model of the radix selection (ScoreCut::cut, k_pq_hist /
k_pq_find: six digits of 11, 11, 11, 11, 11 and 9 bits over the key image << 32 | row).  For every dataset, direction, query scale and
named (threshold, cap) the model must need at least as many passes as the digit the case is about, and the keys still matching at that
digit must lie in more than one of its buckets.  If PQ_DIGIT or the key layout changes, this reports the lost coverage instead of
tests/test_gpu_selection_planted.py going quietly soft.  No GPU; the model describes the inputs, it is no expectation of a search."""
import re
from pathlib import Path

import numpy as np
import pytest

import selection_common as S

f32, u32, u64 = S.f32, S.u32, S.u64
CSRC = Path(__file__).resolve().parent.parent / "lynsedb_amd" / "csrc"


def test_constants_follow_the_sources():
    pq, rng = (CSRC / "pq.h").read_text(), (CSRC / "range.h").read_text()
    assert int(re.search(r"constexpr uint32_t PQ_DIGIT = (\d+);", pq).group(1)) == S.PQ_DIGIT
    assert int(re.search(r"constexpr uint32_t PQ_EMIT_TILE = (\d+);", pq).group(1)) == S.EMIT_TILE
    assert int(re.search(r"constexpr uint32_t RANGE_FAIL = 0x([0-9a-f]+)u;", rng).group(1), 16) == S.RANGE_FAIL
    assert int(re.search(r"constexpr uint32_t RANGE_MAX_ROWS = (\d+);", rng).group(1)) == S.RANGE_TILE
    host = (CSRC / "rerank_host.inc").read_text()
    assert int(re.search(r"const uint32_t rpb = (\d+);", host).group(1)) == S.HIST_BLOCK
    assert "rb += 256 * 8" in pq and S.HIST_TRIP == 256 * 8
    # the digits tile the 64 key bits from the top, PQ_DIGIT at a time
    hi = 64
    for d in sorted(S.DIGITS):
        top, low = S.DIGITS[d]
        assert top == hi - 1 and low == max(hi - S.PQ_DIGIT, 0)
        hi = low
    assert hi == 0


def test_key_restatement():
    x = np.array([-np.inf, -3.0e38, -1.0, -1e-45, 0.0, 1e-45, 1.1754944e-38, 1.0, 3.4028235e38, np.inf], f32)
    o = S.f32_to_ord(x)
    assert (np.diff(o.astype(np.int64)) > 0).all()                     # the ord image is monotone
    assert (np.diff(S.score_ord(x, True).astype(np.int64)) > 0).all() and (np.diff(S.score_ord(x, False).astype(np.int64)) < 0).all()
    assert S.f32_to_ord(np.array([1.0], f32))[0] == 0xBF800000 and S.f32_to_ord(np.array([-1.0], f32))[0] == 0x407FFFFF
    assert S.score_ord([-0.0], True)[0] == S.score_ord([0.0], True)[0] and S.score_ord([-0.0], False)[0] == S.score_ord([0.0], False)[0]
    # a NaN sorts last, and still below the image reserved for the rows that fail
    assert S.score_ord([np.nan], True)[0] == S.score_ord([np.inf], True)[0] == 0xFF800000 < S.RANGE_FAIL
    assert S.score_ord([np.nan], False)[0] == S.score_ord([-np.inf], False)[0] == 0xFF800000
    k = S.make_keys(np.array([5, 5, 4], u32))
    assert k.tolist() == [(5 << 32) | 0, (5 << 32) | 1, (4 << 32) | 2]


def test_pass_model_on_small_cases():
    # 4 distinct images: the first digit decides
    img = np.array([0x00200000, 0x00400000, 0x00600000, 0x00800000], u32)
    assert len(S.selection_passes(S.make_keys(img), 2)) == 1
    # equal images on rows 0..9: only the last digit tells the rows apart
    p = S.selection_passes(S.make_keys(np.full(10, 7, u32)), 3)
    assert len(p) == 6 and [x["occupied"] for x in p] == [1, 1, 1, 1, 1, 10] and p[-1]["bucket"] == 2
    # ... unless the bucket holds exactly what is needed
    assert len(S.selection_passes(S.make_keys(np.full(10, 7, u32)), 10)) == 1
    # rows 0..1023 with equal images, 512 needed: digit 5 ends it
    assert len(S.selection_passes(S.make_keys(np.full(1024, 7, u32)), 512)) == 5


CASES = [(name, asc) for name in S.DATASETS for asc in (True, False)]


@pytest.fixture(scope="module")
def report():
    lines = []
    yield lines
    print("\n" + "\n".join(lines))


@pytest.mark.parametrize("name,asc", CASES, ids=[f"{n}-{'asc' if a else 'desc'}" for n, a in CASES])
def test_every_cut_reaches_its_digit(name, asc, report):
    ds = S.DATASETS[name](asc)
    assert ds.n % 128 and ds.n % 2048 and ds.n % 8192
    for scale in ((1.0,) if asc else S.IP_SCALES):     # L1 has the one query [0]; IP the queries [1], [2], [0.5]
        scores = ds.values * f32(scale)
        assert np.isfinite(scores).all() and (scores >= f32(1.1754944e-38)).all()      # scaled values stay normal
        for cut in ds.cuts:
            images = S.range_images(scores, cut.thr * f32(scale), asc)
            n_pass = int((images != S.RANGE_FAIL).sum())
            assert n_pass > cut.cap, (cut, n_pass)                                    # the query has to select
            passes = S.selection_passes(S.make_keys(images), cut.cap)
            assert len(passes) >= cut.digit, (name, asc, scale, cut, passes)
            assert passes[cut.digit - 1]["occupied"] > 1, (name, asc, scale, cut, passes)
            report.append(f"{name:10s} {'asc ' if asc else 'desc'} x{scale:<4} {cut.name:26s} cap {cut.cap:5d} of {n_pass:7d}: "
                          f"done in pass {len(passes)}, buckets per pass {[p['occupied'] for p in passes]}")


def test_the_datasets_cover_digits_2_to_6():
    about, finish = set(), set()
    for name, asc in CASES:
        ds = S.DATASETS[name](asc)
        for cut in ds.cuts:
            passes = S.selection_passes(S.make_keys(S.range_images(ds.values, cut.thr, asc)), cut.cap)
            about.add(cut.digit)
            finish.add(len(passes))
            # every digit up to the last pass with more than one occupied bucket is one the cut really decides in
            about.update(d + 1 for d, p in enumerate(passes) if p["occupied"] > 1)
    assert {2, 3, 4, 5, 6} <= about and {2, 3, 4, 5, 6} <= finish, (about, finish)


def test_clusters_straddle_the_row_tilings():
    for name in ("digit2", "digit3", "rows_2p20"):
        ds = S.DATASETS[name](True)
        rows = next(iter(ds.groups.values()))
        for t in (S.HIST_BLOCK, S.HIST_TRIP, S.EMIT_TILE, S.RANGE_TILE):
            assert rows[0] // t != rows[-1] // t, (name, t)
    ds = S.rows_512(True)
    run, inside = ds.groups["run"], ds.groups["inside"]
    assert np.unique(run // 512).size >= 4 and np.unique(inside // 512).size == 1
    g = S.rows_2p20(True).groups["group"]
    assert g[0] == (1 << 20) - 300 and g[-1] == (1 << 20) + 299 and S.rows_2p20(True).n > 1 << 20
