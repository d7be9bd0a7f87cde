"""Tip clipping (elba_clip_tips, elba_amd/csrc/tips.hip) restated in plain Python, twice, and the hand-made graphs both test files use.

clip_tips            the rule of include/elba_amd.h statement by statement: sets and dictionaries, one round at a time, from the dead ends
                     inwards.  Input: (M, rows, cols, vals) of S in export order (columns ascending, rows ascending within a column).
                     Returns the clipped S, the flags (bit 2 of every removed read) and every field of the stats except the times.
clip_tips_peel       a second implementation that shares nothing with the first and runs on the CPU only: per round it freezes a degree
                     table, looks from every anchor OUTWARDS along each of its edges for a chain that ends in a dead end, and deletes the
                     tips one at a time from a working set of entries, anchors taken in the order the caller's permutation gives.  It needs
                     a symmetric S.  That both agree whatever the order pins the claim that order does not matter.
Graph, hand_cases    graphs named after the clause of the rule they show, with what each claims (degrees, tip lengths, spared anchors,
                     reads removed, rounds run), so that a case that does not show what its name says fails in test_tips_cpu.py."""
import numpy as np

import contig_util as cu

STATS = ("nreads", "nnz_before", "nnz_after", "dead_ends", "tips", "reads_removed", "entries_removed", "spared_anchors", "rounds_run")


def clip_tips(M, rows, cols, vals, max_tip_reads, rounds=1, trace=None):
    """Returns (rows, cols, vals, flags, stats).  trace, a list, receives per round (tips = [(dead end, reads, anchor)], spared anchors)."""
    rows = [int(r) for r in rows]; cols = [int(c) for c in cols]
    live = list(range(len(rows)))                               # entries of S still there, in export order
    flags = np.zeros(M, dtype=np.uint8)
    st = dict(nreads=M, nnz_before=len(rows), nnz_after=len(rows), dead_ends=0, tips=0, reads_removed=0, entries_removed=0, spared_anchors=0, rounds_run=0)
    for rnd in range(rounds):
        # the degrees as the round finds them: a read's degree is the length of its column
        column = {}
        for a in live:
            column.setdefault(cols[a], []).append(rows[a])
        deg = {v: len(column.get(v, ())) for v in range(M)}
        # 1. dead ends
        dead_ends = [v for v in range(M) if deg[v] == 1]
        if rnd == 0:
            st["dead_ends"] = len(dead_ends)
        # 2. tips
        tips = []
        for v1 in dead_ends:
            chain = [v1]
            prev, cur = v1, column[v1][0]
            while True:
                if deg[cur] >= 3:                               # the anchor
                    tips.append((v1, tuple(chain), cur))
                    break
                if deg[cur] != 2:                               # a read of degree 1: a plain path
                    break
                if len(chain) == max_tip_reads:                 # cur would be read max_tip_reads + 1 of the chain
                    break
                a, b = column[cur]
                nxt = a if a != prev else b
                chain.append(cur)
                prev, cur = cur, nxt
        st["tips"] += len(tips)
        # 3. sparing
        T = {}
        for _, _, b in tips:
            T[b] = T.get(b, 0) + 1
        spared = {b for b in T if not deg[b] - T[b] >= 1}
        st["spared_anchors"] += len(spared)
        removed = set()
        for _, chain, b in tips:
            if b not in spared:
                removed |= set(chain)
        if trace is not None:
            trace.append((tips, spared))
        st["rounds_run"] = rnd + 1
        if not removed:
            break
        # 4. removal
        st["reads_removed"] += len(removed)
        for v in removed:
            flags[v] |= 4
        live = [a for a in live if rows[a] not in removed and cols[a] not in removed]
    st["nnz_after"] = len(live)
    st["entries_removed"] = st["nnz_before"] - len(live)
    idx = np.array(live, dtype=np.int64)
    return np.asarray(rows, dtype=np.int64)[idx], np.asarray(cols, dtype=np.int64)[idx], np.asarray(vals)[idx], flags, st


def clip_tips_peel(M, rows, cols, vals, max_tip_reads, rounds=1, order=None):
    """The same result by peeling: from the anchors outwards, one tip deleted at a time.  order: a permutation of the reads, the order in
    which anchors are visited (default: descending)."""
    rows = np.asarray(rows, dtype=np.int64); cols = np.asarray(cols, dtype=np.int64)
    assert set(zip(rows.tolist(), cols.tolist())) == set(zip(cols.tolist(), rows.tolist())), "clip_tips_peel needs both triangles"
    order = list(range(M - 1, -1, -1)) if order is None else [int(v) for v in order]
    present = np.ones(len(rows), dtype=bool)
    flags = np.zeros(M, dtype=np.uint8)
    st = dict(nreads=M, nnz_before=len(rows), nnz_after=len(rows), dead_ends=0, tips=0, reads_removed=0, entries_removed=0, spared_anchors=0, rounds_run=0)
    for rnd in range(rounds):
        frozen = np.bincount(cols[present], minlength=M)        # the frozen degree table of the round
        nbrs = [[] for _ in range(M)]
        for r, c in zip(rows[present].tolist(), cols[present].tolist()):
            nbrs[c].append(r)
        if rnd == 0:
            st["dead_ends"] = int((frozen == 1).sum())
        deleted = 0
        for b in order:
            if frozen[b] < 3:
                continue
            found = []
            for u in nbrs[b]:                                   # outwards along every edge of b
                chain, prev, cur = [u], b, u
                while frozen[cur] == 2 and len(chain) <= max_tip_reads:
                    nxt = nbrs[cur][0] if nbrs[cur][0] != prev else nbrs[cur][1]
                    prev, cur = cur, nxt
                    chain.append(cur)
                if frozen[cur] == 1 and len(chain) <= max_tip_reads:
                    found.append(chain)
            st["tips"] += len(found)
            if not found:
                continue
            if len(found) == frozen[b]:
                st["spared_anchors"] += 1
                continue
            for chain in found:                                 # one tip at a time
                gone = np.isin(rows, chain) | np.isin(cols, chain)
                present &= ~gone
                flags[chain] |= 4
                deleted += len(chain)
        st["rounds_run"] = rnd + 1
        st["reads_removed"] += deleted
        if not deleted:
            break
    st["nnz_after"] = int(present.sum())
    st["entries_removed"] = st["nnz_before"] - st["nnz_after"]
    return rows[present], cols[present], np.asarray(vals)[present], flags, st


def same(a, b):
    """Two results (rows, cols, vals, flags, stats) are equal entry for entry, field for field."""
    ok = len(a[0]) == len(b[0]) and (a[0] == b[0]).all() and (a[1] == b[1]).all() and a[2].tobytes() == b[2].tobytes()
    return bool(ok and (a[3] == b[3]).all() and a[4] == b[4])


class Graph:
    """Reads and pairs by construction: arm(b, n) hangs a chain of n new reads off b and returns them, b's neighbour first."""

    def __init__(self):
        self.n = 0
        self.pairs = []

    def new(self, k=1):
        ids = list(range(self.n, self.n + k))
        self.n += k
        return ids

    def link(self, u, v):
        self.pairs.append((u, v))

    def chain(self, ids, closed=False):
        for u, v in zip(ids[:-1], ids[1:]):
            self.link(u, v)
        if closed:
            self.link(ids[-1], ids[0])
        return ids

    def arm(self, b, n):
        ids = self.new(n)
        self.link(b, ids[0])
        return self.chain(ids)

    def overlaps(self, rng, perm=None, M=None):
        """(M, rows, cols, vals) for elba_set_overlaps: reads of 20 .. 40 bases are assumed, suffix and suffixT in [5, 9] so that at fuzz 0
        no entry is transitive (a two-edge walk is at least 10) and every suffix is a valid prefix.  perm renames read v to perm[v]."""
        M = self.n if M is None else M
        edges = {}
        for u, v in self.pairs:
            if perm is not None:
                u, v = int(perm[u]), int(perm[v])
            i, j = min(u, v), max(u, v)
            assert i != j and (i, j) not in edges
            o = cu.edge(rng, 20, 20)
            o["suffix"] = int(rng.integers(5, 10)); o["suffixT"] = int(rng.integers(5, 10))
            edges[(i, j)] = o
        return (M,) + cu.upper(edges)


def symmetric_of(rows, cols, vals):
    """S of an upper-triangular edge list none of whose entries is removed: both triangles in export order."""
    return cu.symmetric({(int(r), int(c)): v for r, c, v in zip(rows, cols, vals)})


def _y(arms):
    g = Graph()
    b = g.new()[0]
    return g, b, [g.arm(b, n) for n in arms]


def hand_cases():
    """name -> dict(graph, max, rounds, perm, and the claims: deg {read: degree}, tip_lengths (first round, sorted), spared (first
    round), removed (all rounds, a set), rounds_run, deg_after {read: degree})."""
    cases = {}
    for mx in (1, 2, 7):
        g, b, arms = _y([1, mx, mx + 1])
        cases["y_arms_1_max_maxplus1_max%d" % mx] = dict(graph=g, max=mx, rounds=1, deg={b: 3, arms[2][-1]: 1}, tip_lengths=[1, mx], spared=set(),
                                                         removed=set(arms[0]) | set(arms[1]), rounds_run=1, deg_after={b: 1})
    g, b, arms = _y([1, 2, 10])
    cases["two_tips_one_long_arm"] = dict(graph=g, max=3, rounds=1, deg={b: 3}, tip_lengths=[1, 2], spared=set(), removed=set(arms[0]) | set(arms[1]),
                                          rounds_run=1, deg_after={b: 1})
    g, b, arms = _y([1, 2, 2])
    cases["star_of_three_short_arms"] = dict(graph=g, max=3, rounds=2, deg={b: 3}, tip_lengths=[1, 2, 2], spared={b}, removed=set(), rounds_run=1, deg_after={b: 3})
    g, b, arms = _y([1, 1, 2, 3])
    cases["star_of_four_short_arms"] = dict(graph=g, max=3, rounds=2, deg={b: 4}, tip_lengths=[1, 1, 2, 3], spared={b}, removed=set(), rounds_run=1, deg_after={b: 4})
    g = Graph()
    p = g.chain(g.new(6))
    cases["plain_path"] = dict(graph=g, max=7, rounds=3, deg={p[0]: 1, p[2]: 2, p[5]: 1}, tip_lengths=[], spared=set(), removed=set(), rounds_run=1, deg_after={p[0]: 1})
    g = Graph()
    cyc = g.chain(g.new(5), closed=True)
    tip = g.arm(cyc[2], 2)
    cases["cycle_with_one_tip"] = dict(graph=g, max=2, rounds=2, deg={cyc[2]: 3, cyc[0]: 2, tip[1]: 1}, tip_lengths=[2], spared=set(), removed=set(tip), rounds_run=2,
                                       deg_after={v: 2 for v in cyc})
    g, b, arms = _y([5, 6, 7, 2])
    cases["anchor_of_degree_4_with_one_tip"] = dict(graph=g, max=3, rounds=1, deg={b: 4}, tip_lengths=[2], spared=set(), removed=set(arms[3]), rounds_run=1, deg_after={b: 3})
    for rounds, removed_n, run in ((1, 2, 1), (2, 4, 2), (64, 4, 3)):
        g, a, arms = _y([6, 7, 1])
        c1 = arms[2][0]
        bb = g.arm(c1, 1)[0]
        x, y = g.arm(bb, 1)[0], g.arm(bb, 1)[0]
        rm = {x, y} if rounds == 1 else {x, y, bb, c1}
        assert len(rm) == removed_n
        cases["tip_on_a_tip_rounds%d" % rounds] = dict(graph=g, max=2, rounds=rounds, deg={a: 3, bb: 3, c1: 2, x: 1, y: 1}, tip_lengths=[1, 1], spared=set(), removed=rm,
                                                       rounds_run=run, deg_after={a: 3 if rounds == 1 else 2, bb: 1 if rounds == 1 else 0})
    g, a, arms = _y([5, 6, 1])
    c = arms[2][0]
    b2 = g.arm(c, 1)[0]
    g.arm(b2, 5); g.arm(b2, 6)
    cases["two_anchors_joined_by_a_short_chain"] = dict(graph=g, max=3, rounds=2, deg={a: 3, c: 2, b2: 3}, tip_lengths=[], spared=set(), removed=set(), rounds_run=1,
                                                        deg_after={a: 3, b2: 3})
    for name, first in (("dead_end_0_anchor_last", "dead"), ("anchor_0_dead_end_last", "anchor")):
        g, b, arms = _y([1, 5, 6])
        d, M = arms[0][0], g.n
        rest = [v for v in range(M) if v not in (b, d)]
        perm = np.zeros(M, dtype=np.int64)
        perm[d], perm[b] = (0, M - 1) if first == "dead" else (M - 1, 0)
        perm[rest] = np.arange(1, M - 1)
        cases[name] = dict(graph=g, max=1, rounds=1, perm=perm, deg={int(perm[b]): 3, int(perm[d]): 1}, tip_lengths=[1], spared=set(), removed={int(perm[d])},
                           rounds_run=1, deg_after={int(perm[b]): 2, int(perm[d]): 0})
        assert {int(perm[b]), int(perm[d])} == {0, M - 1}
    return cases


def case_overlaps(case, rng, extra_reads=0):
    """(M, rows, cols, vals) of a hand case for elba_set_overlaps; extra_reads isolated reads follow the graph's."""
    g = case["graph"]
    return g.overlaps(rng, perm=case.get("perm"), M=g.n + extra_reads)


def plant_tips(rng, M, rows, cols, vals, anchors, lengths):
    """Adds a chain of lengths[i] NEW reads (ids from M on) to anchors[i].  Returns (M', rows, cols, vals, planted reads), (row, col) order."""
    xr, xc, planted, nxt = [], [], [], int(M)
    for b, n in zip(anchors, lengths):
        prev = int(b)
        for _ in range(int(n)):
            xr.append(prev); xc.append(nxt)                     # prev < nxt: new ids are the largest
            planted.append(nxt)
            prev, nxt = nxt, nxt + 1
    xv = np.zeros(len(xr), dtype=np.asarray(vals).dtype)
    xv["passed"] = 1
    xv["direction"] = rng.integers(0, 4, len(xr)); xv["directionT"] = rng.integers(0, 4, len(xr))
    xv["suffix"] = rng.integers(5, 10, len(xr)); xv["suffixT"] = rng.integers(5, 10, len(xr))
    r = np.concatenate([np.asarray(rows, dtype=np.int64), np.array(xr, dtype=np.int64)])
    c = np.concatenate([np.asarray(cols, dtype=np.int64), np.array(xc, dtype=np.int64)])
    v = np.concatenate([np.asarray(vals), xv])
    order = np.lexsort((c, r))
    return nxt, r[order], c[order], v[order], np.array(planted, dtype=np.int64)
