"""Cutting weak overlaps (elba_cut_weak_overlaps, elba_amd/csrc/weak.hip) restated in plain Python, twice, and the hand-made graphs the
test files use.

cut_weak             the rule of include/elba_amd.h statement by statement, with loops over columns and Python integers.  Input: (M, rows,
                     cols, vals) of S in export order (columns ascending, rows ascending within a column).  Returns the cut S and every
                     field of the stats except the times.  No read flag changes, so none is returned.
cut_weak_sorted      a second implementation for the larger cases that shares nothing with the first: a lexsort by (column, side), segmented
                     maxima and counts by reduceat, the mirror image by a search in the keys column * M + row.
S_of                 what tr.hip leaves of an upper-triangular edge list none of whose entries is transitive: both images, without those
                     whose direction is not 0 .. 3 (directionT = -1 on the loaded edge gives a pair with one image).
WeakGraph            tip_util.Graph whose links carry a score and the end of each read they lie on; overlaps() writes score, direction and
                     directionT from them, explicitly.
hand_cases           graphs named after the clause of the rule they show, with what each claims (cnt, best, the weak entries, the removed
                     pairs, the emptied sides), so that a case that does not show what its name says fails in test_weak_cpu.py.
simplify             clip_tips(.., 64), pop_bubbles(.., 64), cut_weak of the restatements until a pass of the three removes nothing: what
                     Engine.simplify_graph(.., min_overlap_ratio=..) is held against."""
import numpy as np

import bubble_util as bu
import contig_util as cu
import tip_util as tu

STATS = ("nreads", "nnz_before", "nnz_after", "branch_sides", "weak_entries", "entries_removed", "sides_emptied")
Q07 = 45875                                                     # int(round(0.7 * 65536))
assert Q07 == int(round(0.7 * 65536))


def q16_of(ratio):
    return int(round(ratio * 65536))


def cut_weak(M, rows, cols, vals, q16, trace=None):
    """Returns (rows, cols, vals, stats).  trace, a dict, receives cnt and best {(read, side): .}, weak (a set of (row, col)) and removed
    (a set of (row, col))."""
    assert 1 <= q16 <= 65536
    rows = [int(r) for r in rows]; cols = [int(c) for c in cols]
    score = [int(s) for s in np.asarray(vals)["score"]]
    side = [int(d) & 1 for d in np.asarray(vals)["direction"]]     # the end of read c the overlap lies on
    n = len(rows)
    column = {}                                                 # c -> its entries, rows ascending
    for z in range(n):
        column.setdefault(cols[z], []).append(z)
    # 1. cnt and best per read and side
    cnt, best = {}, {}
    for c in range(M):
        for e in (0, 1):
            mine = [z for z in column.get(c, ()) if side[z] == e]
            cnt[(c, e)] = len(mine)
            if mine:
                best[(c, e)] = max(score[z] for z in mine)
    # 2. weak at its column
    weak = set()
    for c in range(M):
        for z in column.get(c, ()):
            k = (c, side[z])
            if cnt[k] >= 2 and best[k] > 0 and score[z] * 65536 < q16 * best[k]:
                weak.add(z)
    # 3. removed: weak at its column, or its mirror image weak at its own
    entry = {(rows[z], cols[z]): z for z in range(n)}
    assert len(entry) == n
    removed = set()
    for z in range(n):
        mirror = entry.get((cols[z], rows[z]))                  # the entry of column r whose row is c, if S holds one
        if z in weak or (mirror is not None and mirror in weak):
            removed.add(z)
    # 4. survivors in their order
    live = [z for z in range(n) if z not in removed]
    after = {}
    for z in live:
        after[(cols[z], side[z])] = after.get((cols[z], side[z]), 0) + 1
    st = dict(nreads=M, nnz_before=n, nnz_after=len(live), branch_sides=sum(1 for k in cnt if cnt[k] >= 2), weak_entries=len(weak),
              entries_removed=len(removed), sides_emptied=sum(1 for k in cnt if cnt[k] >= 1 and after.get(k, 0) == 0))
    if trace is not None:
        trace.update(cnt=cnt, best=best, weak={(rows[z], cols[z]) for z in weak}, removed={(rows[z], cols[z]) for z in removed})
    idx = np.array(live, dtype=np.int64)
    return np.asarray(rows, dtype=np.int64)[idx], np.asarray(cols, dtype=np.int64)[idx], np.asarray(vals)[idx], st


def cut_weak_sorted(M, rows, cols, vals, q16):
    """The same result from sorted segments.  Returns (rows, cols, vals, stats)."""
    rows = np.asarray(rows, dtype=np.int64); cols = np.asarray(cols, dtype=np.int64); vals = np.asarray(vals)
    n = len(rows)
    st = dict(nreads=M, nnz_before=n, nnz_after=n, branch_sides=0, weak_entries=0, entries_removed=0, sides_emptied=0)
    if n == 0:
        return rows, cols, vals, st
    score = vals["score"].astype(np.int64)
    seg = cols * 2 + (vals["direction"].astype(np.int64) & 1)   # the (column, side) of every entry
    order = np.lexsort((score, seg))                            # by segment, the best last
    s_sorted = seg[order]
    first = np.flatnonzero(np.r_[True, s_sorted[1:] != s_sorted[:-1]])
    last = np.r_[first[1:], n] - 1
    seg_cnt = last - first + 1
    seg_best = score[order][last]
    assert (seg_best == np.maximum.reduceat(score[order], first)).all()
    which = np.cumsum(np.r_[False, s_sorted[1:] != s_sorted[:-1]])      # segment of every sorted entry
    cnt = np.empty(n, dtype=np.int64); best = np.empty(n, dtype=np.int64)
    cnt[order] = seg_cnt[which]; best[order] = seg_best[which]
    weak = (cnt >= 2) & (best > 0) & (score * 65536 < q16 * best)
    key = cols * M + rows                                       # ascending: the export order
    assert (np.diff(key) > 0).all()
    at = np.searchsorted(key, rows * M + cols)
    has = (at < n) & (key[np.minimum(at, n - 1)] == rows * M + cols)
    mirror_weak = np.zeros(n, dtype=bool)
    mirror_weak[has] = weak[at[has]]
    keep = ~(weak | mirror_weak)
    seg_after = np.bincount(seg[keep], minlength=2 * M)
    seg_before = np.bincount(seg, minlength=2 * M)
    st.update(nnz_after=int(keep.sum()), branch_sides=int((seg_before >= 2).sum()), weak_entries=int(weak.sum()), entries_removed=int((~keep).sum()),
              sides_emptied=int(((seg_before >= 1) & (seg_after == 0)).sum()))
    return rows[keep], cols[keep], vals[keep], st


def same(a, b):
    """Two results (rows, cols, vals, stats) are equal entry for entry, field for field."""
    return bool(len(a[0]) == len(b[0]) and (a[0] == b[0]).all() and (a[1] == b[1]).all() and a[2].tobytes() == b[2].tobytes() and a[3] == b[3])


def S_of(rows, cols, vals):
    """S of an upper-triangular edge list none of whose entries is transitive, contained or of a bad read: both triangles in export order,
    an image whose direction is not 0 .. 3 left out (tr.hip drops it)."""
    r, c, v = tu.symmetric_of(rows, cols, vals)
    ok = (v["direction"] >= 0) & (v["direction"] <= 3)
    return r[ok], c[ok], v[ok]


def simplify(M, rows, cols, vals, max_tip_reads, max_arm_reads, q16, passes=16):
    """The restatements in the order Engine.simplify_graph(.., min_overlap_ratio) runs the calls.  Returns (rows, cols, vals, flags,
    [(tip stats, bubble stats, weak stats)])."""
    flags = np.zeros(M, dtype=np.uint8)
    out = []
    for _ in range(passes):
        rows, cols, vals, f1, s1 = tu.clip_tips(M, rows, cols, vals, max_tip_reads, 64)
        rows, cols, vals, f2, s2 = bu.pop_bubbles(M, rows, cols, vals, max_arm_reads, 64)
        rows, cols, vals, s3 = cut_weak(M, rows, cols, vals, q16)
        flags |= f1 | f2
        out.append((s1, s2, s3))
        if s1["reads_removed"] == 0 and s2["reads_removed"] == 0 and s3["entries_removed"] == 0:
            break
    return rows, cols, vals, flags, out


class WeakGraph(tu.Graph):
    """link(u, v, score, su, sv): the overlap lies on end su of read u and end sv of read v.  A chain goes from end 1 of a read to end 0
    of the next with score 100, so that a read inside a chain has one entry on each side.  one_image: directionT = -1 on the loaded edge,
    which leaves the entry in the larger read's column alone."""

    def __init__(self):
        super().__init__()
        self.attr = {}

    def link(self, u, v, score=100, su=1, sv=0, one_image=False):
        super().link(u, v)
        self.attr[(u, v)] = (int(score), su, sv, one_image)

    def overlaps(self, rng, perm=None, M=None):
        M, rows, cols, vals = super().overlaps(rng, perm=perm, M=M)
        at = {(int(r), int(c)): z for z, (r, c) in enumerate(zip(rows, cols))}
        for (u, v), (score, su, sv, one) in self.attr.items():
            if perm is not None:
                u, v = int(perm[u]), int(perm[v])
            if u > v:
                u, v, su, sv = v, u, sv, su
            o = vals[at[(u, v)]]                                 # S(u, v), in column v: direction & 1 is the end of v; its transpose, in column u, gets directionT
            o["score"] = score; o["direction"] = sv; o["directionT"] = -1 if one else su
        return M, rows, cols, vals


def _pairs(*uv):
    return {frozenset(p) for p in uv}


def _y(g, arms, scores, sides, tail=4, left=True):
    """Anchor a (with a chain of `tail` reads entering its end 0 if left) and one chain of `tail` reads per arm, hung on end sides[i] of a
    with score scores[i]; an arm's first read takes the overlap on its end 0.  Returns (a, first reads)."""
    a = g.new()[0]
    if left:
        ids = g.new(tail)
        g.chain(ids)
        g.link(ids[-1], a)
    firsts = []
    for _ in range(arms):
        ids = g.new(tail)
        g.chain(ids)
        firsts.append(ids[0])
    for x, s, e in zip(firsts, scores, sides):
        g.link(a, x, s, su=e, sv=0)
    return a, firsts


def hand_cases():
    """name -> dict(graph, q16, perm, and the claims: cnt {(read, side): n}, best {(read, side): score}, weak (entries (row, col) weak at
    their own column, all of them), removed (pairs, all of them), branch_sides, sides_emptied)."""
    cases = {}
    for s2, cut in ((69, True), (70, False)):
        g = WeakGraph()
        a, (x, y) = _y(g, 2, (100, s2), (1, 1))
        assert (s2 * 65536 < Q07 * 100) == cut
        cases["y_same_side_100_%d_%s" % (s2, "cut" if cut else "kept")] = dict(
            graph=g, q16=Q07, cnt={(a, 0): 1, (a, 1): 2, (y, 0): 1, (y, 1): 1}, best={(a, 1): 100, (a, 0): 100, (y, 0): s2},
            weak={(y, a)} if cut else set(), removed=_pairs((a, y)) if cut else set(), branch_sides=1, sides_emptied=1 if cut else 0)
    g = WeakGraph()
    a, (x, y) = _y(g, 2, (100, 69), (1, 0), left=False)
    cases["the_two_edges_on_opposite_sides"] = dict(graph=g, q16=Q07, cnt={(a, 0): 1, (a, 1): 1}, best={(a, 0): 69, (a, 1): 100}, weak=set(), removed=set(),
                                                    branch_sides=0, sides_emptied=0)
    for s2, cut in ((50, False), (49, True)):
        g = WeakGraph()
        a, (x, y) = _y(g, 2, (100, s2), (1, 1))
        assert (s2 * 65536 == 32768 * 100) == (not cut) and (s2 * 65536 < 32768 * 100) == cut
        cases["threshold_half_of_100_score_%d" % s2] = dict(graph=g, q16=32768, cnt={(a, 1): 2}, best={(a, 1): 100}, weak={(y, a)} if cut else set(),
                                                            removed=_pairs((a, y)) if cut else set(), branch_sides=1, sides_emptied=1 if cut else 0)
    g = WeakGraph()
    a, (x, y, w) = _y(g, 3, (100, 100, 99), (1, 1, 1))
    cases["ties_at_the_best_stay_at_ratio_1"] = dict(graph=g, q16=65536, cnt={(a, 1): 3}, best={(a, 1): 100}, weak={(w, a)}, removed=_pairs((a, w)), branch_sides=1,
                                                     sides_emptied=1)
    g = WeakGraph()
    a, (x, y, w) = _y(g, 3, (10, 0, -5), (1, 1, 1))
    cases["zero_and_negative_scores_under_a_positive_best"] = dict(graph=g, q16=1, cnt={(a, 1): 3}, best={(a, 1): 10, (y, 0): 0, (w, 0): -5}, weak={(y, a), (w, a)},
                                                                   removed=_pairs((a, y), (a, w)), branch_sides=1, sides_emptied=2)
    for name, scores in (("best_zero", (0, -7)), ("best_negative", (-3, -7))):
        g = WeakGraph()
        a, (x, y) = _y(g, 2, scores, (1, 1))
        cases["a_side_whose_%s_has_nothing_weak" % name] = dict(graph=g, q16=65536, cnt={(a, 1): 2}, best={(a, 1): scores[0]}, weak=set(), removed=set(), branch_sides=1,
                                                                sides_emptied=0)
    g = WeakGraph()
    a, (x, y) = _y(g, 2, (2 ** 31 - 1, -2 ** 31), (1, 1))
    cases["scores_int32_max_and_min"] = dict(graph=g, q16=65536, cnt={(a, 1): 2}, best={(a, 1): 2 ** 31 - 1}, weak={(y, a)}, removed=_pairs((a, y)), branch_sides=1,
                                             sides_emptied=1)
    for q, cut in ((65535, False), (65536, True)):               # the products need 48 bits: (2^31 - 2) * 65536 against q * (2^31 - 1)
        g = WeakGraph()
        a, (x, y) = _y(g, 2, (2 ** 31 - 1, 2 ** 31 - 2), (1, 1))
        assert ((2 ** 31 - 2) * 65536 < q * (2 ** 31 - 1)) == cut
        cases["scores_int32_max_and_one_less_q%d" % q] = dict(graph=g, q16=q, cnt={(a, 1): 2}, best={(a, 1): 2 ** 31 - 1}, weak={(y, a)} if cut else set(),
                                                              removed=_pairs((a, y)) if cut else set(), branch_sides=1, sides_emptied=1 if cut else 0)
    # a - b is the best of a's end 1 (50 against 10) and weak at b's end 0 (50 against 100): it goes, a - c goes for itself, and a's end 1 is empty
    g = WeakGraph()
    a, (b, c) = _y(g, 2, (50, 10), (1, 1))
    d = g.new(4)
    g.chain(d)
    g.link(d[-1], b, 100, su=1, sv=0)
    cases["best_at_its_column_weak_at_its_row"] = dict(graph=g, q16=Q07, cnt={(a, 1): 2, (b, 0): 2, (c, 0): 1}, best={(a, 1): 50, (b, 0): 100}, weak={(a, b), (c, a)},
                                                       removed=_pairs((a, b), (a, c)), branch_sides=2, sides_emptied=2)
    # one image only, weak at the column that holds it: u < v, the entry is S(u, v) in column v
    g = WeakGraph()
    v_chain = g.new(4)                                          # ids below: the one-image pair's smaller read comes first
    g.chain(v_chain)
    u = v_chain[0]
    a, (x,) = _y(g, 1, (100,), (1,))
    g.link(u, a, 30, su=0, sv=1, one_image=True)
    assert u < a
    cases["one_image_weak_at_its_own_column"] = dict(graph=g, q16=Q07, cnt={(a, 1): 2, (u, 0): 0, (u, 1): 1}, best={(a, 1): 100}, weak={(u, a)}, removed=_pairs((u, a)),
                                                     branch_sides=1, sides_emptied=0)
    # one image only, and the missing image is the one that would be weak: the pair stays
    g = WeakGraph()
    a, (x,) = _y(g, 1, (100,), (1,))
    w = g.new(4)
    g.chain(w)
    assert a < w[0]
    g.link(a, w[0], 30, su=1, sv=0, one_image=True)             # in column w[0] alone on its side; column a holds no entry for it
    cases["one_image_whose_missing_image_would_be_weak"] = dict(graph=g, q16=Q07, cnt={(a, 1): 1, (w[0], 0): 1}, best={(a, 1): 100, (w[0], 0): 30}, weak=set(),
                                                                removed=set(), branch_sides=0, sides_emptied=0)
    # a read of degree 2 with both entries on one side
    g = WeakGraph()
    m = g.new()[0]
    p, q = g.new(4), g.new(4)
    g.chain(p); g.chain(q)
    g.link(m, p[0], 100, su=0, sv=0)
    g.link(m, q[0], 10, su=0, sv=0)
    cases["degree_2_read_with_both_entries_on_one_side"] = dict(graph=g, q16=Q07, cnt={(m, 0): 2, (m, 1): 0}, best={(m, 0): 100}, weak={(q[0], m)}, removed=_pairs((m, q[0])),
                                                                branch_sides=1, sides_emptied=1)
    return cases


def case_S(case, rng, extra_reads=0):
    """(M, rows, cols, vals) of a hand case for elba_set_overlaps, and the S the reduction at fuzz 0 leaves of it."""
    g = case["graph"]
    M, rows, cols, vals = g.overlaps(rng, perm=case.get("perm"), M=g.n + extra_reads)
    return (M, rows, cols, vals), S_of(rows, cols, vals)


def plant_weak_edges(M, rows, cols, vals, pairs, score, directions):
    """Adds the pairs (u < v, not yet in the list) with the given score and (direction, directionT) to an upper-triangular edge list.
    Returns (rows, cols, vals) in (row, col) order."""
    xr = np.array([p[0] for p in pairs], dtype=np.int64); xc = np.array([p[1] for p in pairs], dtype=np.int64)
    assert (xr < xc).all() and xc.max() < M
    xv = np.zeros(len(pairs), dtype=np.asarray(vals).dtype)
    xv["passed"] = 1; xv["score"] = score
    xv["direction"] = [d[0] for d in directions]; xv["directionT"] = [d[1] for d in directions]
    xv["suffix"] = 7; xv["suffixT"] = 7
    r = np.concatenate([np.asarray(rows, dtype=np.int64), xr]); c = np.concatenate([np.asarray(cols, dtype=np.int64), xc])
    v = np.concatenate([np.asarray(vals), xv])
    key = r * M + c
    assert len(np.unique(key)) == len(key)
    order = np.lexsort((c, r))
    return r[order], c[order], v[order]


def random_S(rng, M, p_one_image=0.05, lo=-3, hi=12):
    """S of a random triangle-free graph with random sides and small random scores (so that ties, zeros and negative bests occur);
    p_one_image of the pairs keep one image."""
    lens = np.full(M, 20)
    rows, cols, vals = cu.random_string_graph(rng, M, lens)
    vals["score"] = rng.integers(lo, hi, len(vals))
    vals["directionT"][rng.random(len(vals)) < p_one_image] = -1
    return (rows, cols, vals), S_of(rows, cols, vals)


def relabel_upper(perm, rows, cols, vals):
    """The same overlaps with read v renamed perm[v]: an upper-triangular edge list again (a pair whose order turns round is transposed)."""
    edges = {}
    for r, c, v in zip(rows, cols, vals):
        i, j = int(perm[r]), int(perm[c])
        edges[(min(i, j), max(i, j))] = v if i < j else cu.transpose(v)
    return cu.upper(edges)
