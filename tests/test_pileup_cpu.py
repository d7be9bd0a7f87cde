"""CPU tests of the pileup restatement (pileup_util.py) on hand-made cases: the trim rule at its edges, the profile format, margins, the
flags and the prune; and the two deliberate deviations from src/PruneChimeras.cpp next to the reference's literal behaviour."""
import numpy as np
import pytest

import pileup_util as pu
from elba_amd.capi import OVERLAP_DTYPE


def _pairs(spec):
    """spec: [(q, t, begQ, endQ, begT, endT, passed, score)] -> rows, cols, vals"""
    vals = np.zeros(len(spec), dtype=OVERLAP_DTYPE)
    rows = np.array([s[0] for s in spec], dtype=np.int64); cols = np.array([s[1] for s in spec], dtype=np.int64)
    for a, (_, _, bq, eq, bt, et, ps, sc) in enumerate(spec):
        vals[a]["begQ"], vals[a]["endQ"], vals[a]["begT"], vals[a]["endT"], vals[a]["passed"], vals[a]["score"] = bq, eq, bt, et, ps, sc
    return rows, cols, vals


def test_trim_run_of_exactly_trim_len_does_not_qualify():
    p = [1] * 100
    assert pu.trimmed_interval_literal(p, 1, maxlen=100) == (-1, -1)
    assert pu.trimmed_interval(p, 1, maxlen=100) == (-1, -1)
    p = [1] * 101
    assert pu.trimmed_interval_literal(p, 1, maxlen=100) == (0, 101)
    assert pu.trimmed_interval(p, 1, maxlen=100) == (0, 101)


def test_later_longer_run_with_lower_average_does_not_replace_the_best():
    # a constant run becomes the best at its first base with span > maxlen and stays there (curavg never rises again)
    p = [0] + [5] * 30 + [0] + [2] * 60 + [0]
    assert pu.trimmed_interval_literal(p, 2, maxlen=20) == (1, 22)
    assert pu.trimmed_interval(p, 2, maxlen=20) == (1, 22)
    # ... and a later run with a higher average does replace it, once its span passes the new maxlen (21)
    p = [2] * 30 + [0] + [5] * 40
    assert pu.trimmed_interval_literal(p, 2, maxlen=20) == (31, 53)
    assert pu.trimmed_interval(p, 2, maxlen=20) == (31, 53)
    # a rising run keeps extending the best
    p = list(range(1, 41))
    assert pu.trimmed_interval_literal(p, 1, maxlen=20) == (0, 40)
    assert pu.trimmed_interval(p, 1, maxlen=20) == (0, 40)


def test_best_end_is_where_the_average_last_rose():
    p = [3] * 25 + [1] * 10
    # span > 20 from base 20 on; curavg stays 3 (not > 3) through base 24, then falls: the best is [0, 21)
    assert pu.trimmed_interval_literal(p, 1, maxlen=20) == (0, 21)
    assert pu.trimmed_interval(p, 1, maxlen=20) == (0, 21)


def test_depth_exactly_at_min_depth_counts():
    p = [3] * 50
    assert pu.trimmed_interval_literal(p, 3, maxlen=10) == (0, 11)
    assert pu.trimmed_interval_literal(p, 4, maxlen=10) == (-1, -1)
    assert pu.long_runs(p, 3, 50) == 1 and pu.long_runs(p, 3, 51) == 0 and pu.long_runs(p, 4, 1) == 0


@pytest.mark.parametrize("seed", range(30))
def test_vectorised_trim_equals_the_literal_loop(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 400))
    p = np.repeat(rng.integers(0, 6, 40), rng.integers(1, 30, 40))[:n]
    for thr in (1, 2, 3):
        for ml in (0, 5, 30, 100):
            assert pu.trimmed_interval(p, thr, ml) == pu.trimmed_interval_literal(p.tolist(), thr, ml), (thr, ml)


def test_the_reference_returns_the_open_run_not_the_best():
    p = [4] * 40 + [0] + [1] * 5
    assert pu.trimmed_interval_literal(p, 1, maxlen=10, fixed=False) == (41, 45)      # the run still open at the last base
    assert pu.trimmed_interval_literal(p, 1, maxlen=10) == (0, 11)                    # the best run (half-open)


def test_profile_format_margins_and_edges():
    lens = [100, 50, 0, 30]
    rows, cols, vals = _pairs([
        (0, 1, 0, 100, 0, 50, 1, 10),       # touches 0 and len of both
        (0, 3, 10, 10, 5, 5, 1, 10),        # zero-length intervals: dropped
        (0, 3, 40, 60, 0, 30, 1, 10),
        (1, 3, 20, 22, 10, 12, 1, 10),      # emptied by margin 1
        (0, 1, 50, 60, 10, 20, 0, 10),      # not passed (mode 1 only)
    ])
    got, st, depth, off = pu.pileup(lens, rows, cols, vals, mode=0, margin=1)
    assert list(got["seg_off"]) == [0, 5, 8, 8, 11]
    assert list(zip(got["seg_start"][:5], got["seg_depth"][:5])) == [(0, 0), (1, 1), (41, 2), (59, 1), (99, 0)]
    assert list(zip(got["seg_start"][5:8], got["seg_depth"][5:8])) == [(0, 0), (1, 1), (49, 0)]
    assert list(zip(got["seg_start"][8:], got["seg_depth"][8:])) == [(0, 0), (1, 1), (29, 0)]
    assert st["pairs"] == 4 and st["intervals"] == 4 and st["max_depth"] == 2
    got1, st1, _, _ = pu.pileup(lens, rows, cols, vals, mode=1, margin=0)
    assert st1["pairs"] == 5 and st1["intervals"] == 10 - 2
    a, b = int(got1["seg_off"][1]), int(got1["seg_off"][2])
    assert list(zip(got1["seg_start"][a:b], got1["seg_depth"][a:b])) == [(0, 1), (10, 2), (22, 1)]      # equal neighbours merged at 20


def test_read_without_intervals_and_empty_read():
    lens = [10, 0, 7]
    rows, cols, vals = _pairs([])
    got, st, _, _ = pu.pileup(lens, rows, cols, vals)
    assert list(got["seg_off"]) == [0, 1, 1, 2]
    assert list(got["seg_start"]) == [0, 0] and list(got["seg_depth"]) == [0, 0]
    assert list(got["flags"]) == [1, 1, 1] and list(got["trim_beg"]) == [-1, -1, -1]


def test_segments_rebuild_the_per_base_depth():
    rng = np.random.default_rng(5)
    lens = rng.integers(0, 300, 60)
    n = 400
    rows = rng.integers(0, 60, n); cols = rng.integers(0, 60, n)
    keep = rows < cols
    rows, cols = rows[keep], cols[keep]
    vals = np.zeros(len(rows), dtype=OVERLAP_DTYPE)
    for a in range(len(rows)):
        for (fb, fe, r) in (("begQ", "endQ", rows[a]), ("begT", "endT", cols[a])):
            x = sorted(rng.integers(0, lens[r] + 1, 2))
            vals[a][fb], vals[a][fe] = x
        vals[a]["passed"] = rng.integers(0, 2); vals[a]["score"] = rng.integers(-1, 5)
    for mode in (0, 1):
        for margin in (0, 3):
            got, st, depth, off = pu.pileup(lens, rows, cols, vals, mode=mode, margin=margin, min_depth=2, min_run=10, trim_len=20)
            so, ss, sd = got["seg_off"], got["seg_start"], got["seg_depth"]
            for v in range(len(lens)):
                a, b = int(so[v]), int(so[v + 1])
                if lens[v] == 0:
                    assert a == b
                    continue
                assert ss[a] == 0 and (np.diff(ss[a:b]) > 0).all() and (np.diff(sd[a:b]) != 0).all()
                assert (pu.profile_of(so, ss, sd, lens, v) == depth[off[v]:off[v + 1]]).all()
                assert b - a <= 2 * (int((rows == v).sum()) + int((cols == v).sum())) + 1
            assert st["segments"] == len(ss)


def test_out_of_range_interval_is_rejected():
    rows, cols, vals = _pairs([(0, 1, 0, 11, 0, 5, 1, 1)])
    with pytest.raises(pu.BadInterval):
        pu.pileup([10, 10], rows, cols, vals)
    rows, cols, vals = _pairs([(0, 1, 6, 5, 0, 5, 1, 1)])
    with pytest.raises(pu.BadInterval):
        pu.pileup([10, 10], rows, cols, vals)


def test_flags_and_prune():
    lens = [100, 100, 100, 100]
    rows, cols, vals = _pairs([
        (0, 1, 0, 40, 0, 40, 1, 1),
        (0, 2, 60, 100, 0, 40, 1, 1),          # read 0: two covered stretches with a hole: split
        (1, 2, 0, 100, 0, 100, 1, 1),
        (2, 3, 0, 100, 0, 100, 1, 1),
    ])
    got, st, _, _ = pu.pileup(lens, rows, cols, vals, min_depth=1, min_run=30, trim_len=10)
    assert list(got["flags"]) == [2, 0, 0, 0]
    r, c, v = pu.prune(rows, cols, vals, got["flags"], 2)
    assert list(zip(r, c)) == [(1, 2), (2, 3)]
    got, st, _, _ = pu.pileup(lens, rows, cols, vals, min_depth=2, min_run=30, trim_len=10)
    assert got["flags"][3] == 1 and got["flags"][0] == 1


def test_upper_triangle_only_pileup_of_the_reference_misses_the_row_read():
    """The reference's GetReadPileup on the upper-triangular R credits the column read only: read 0 (the smallest id) never gets coverage,
    read 2 gets it from both partners.  The symmetrised pileup credits every read of every pair."""
    lens = [50, 50, 50]
    rows, cols, vals = _pairs([(0, 1, 10, 50, 0, 40, 1, 1), (0, 2, 0, 30, 20, 50, 1, 1), (1, 2, 5, 45, 0, 40, 1, 1)])
    ref = pu.reference_upper_pileup(lens, rows, cols, vals)
    assert sum(ref[0]) == 0 and sum(ref[1]) == 40 and sum(ref[2]) == 30 + 40
    got, st, depth, off = pu.pileup(lens, rows, cols, vals)
    assert depth[off[0]:off[1]].sum() == 40 + 30 and depth[off[1]:off[2]].sum() == 40 + 40 and depth[off[2]:off[3]].sum() == 30 + 40
    # the column read's share is exactly the reference's
    only_t = np.zeros(150, np.int64)
    for c, o in zip(cols, vals):
        only_t[50 * c + o["begT"]:50 * c + o["endT"]] += 1
    assert (np.concatenate([np.array(x) for x in ref]) == only_t).all()
