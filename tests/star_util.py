"""Resolving three-armed stars (elba_resolve_stars, elba_amd/csrc/stars.hip) restated in plain Python, twice, and the hand-made graphs the
test files use.

r_pairs              the pairs of R from the loaded overlaps: `passed`, and both reads without flag bits 0 and 1 — the flags of the ORACLE's
                     reduction (oracle/pyoracle.py), not what the device keeps.
resolve_stars        the rule of include/elba_amd.h statement by statement: lists and dictionaries, every round on tables frozen at its
                     start.  Input: (M, rows, cols, vals) of S in export order (columns ascending, rows ascending within a column) and the
                     set of R pairs.  Returns the resolved S, the flags (bit 5 of every removed read) and every field of the stats but the times.
resolve_stars_peel   a second form that shares nothing with the first and runs on the CPU only: neighbour SETS that change as it goes, R as
                     neighbour sets too, centres visited in the order the caller's permutation gives within a round, the odd arm found by
                     counting for every neighbour how many of the other two it overlaps, the round's removals collected and then applied.
                     It needs a symmetric S.
simplify             clip_tips, pop_bubbles, [cut_weak], [cut_bridges], resolve_stars of the restatements until a pass removes nothing: what
                     Engine.simplify_graph(.., stars=..) is held against.
StarGraph            tip_util.Graph with two more kinds of pair: rpair(u, v), a pair of R that never reaches S (passed, direction and
                     directionT -1), and one_image(u, v), a pair of which the reduction keeps one image (directionT -1: S(min, max) only).
hand_cases           graphs named after the clause of the rule they show, each with its claims (removed set, centres, pairs0 .. 3, degrees
                     before and after, the rounds that remove something), so that a case that does not show what its name says fails in
                     test_stars_cpu.py.
star_chain           a chain of stars of which round k can resolve the k-th only: exactly K rounds remove something.
lookup_case          a star whose pair {s, k} is looked up in a row of R of a given length with the key at a given place.
long_paths, plant_stars, layout_stars, random_stars
                     generators: stars planted into paths of consecutive reads (the pair of the two path neighbours as an R-only entry);
                     into a layout of string_graph_util.layout_overlaps, where the GPU's own reduction removes the pair as transitive;
                     and rounds_util.random_graph with R-only pairs among the neighbours of its degree-3 reads."""
import numpy as np

import bridge_util as br
import bubble_util as bu
import contig_util as cu
import rounds_util as ru
import string_graph_util as sgu
import tip_util as tu
import weak_util as wu
from oracle import pyoracle as po

STATS = ("nreads", "nnz_before", "nnz_after", "centres", "pairs0", "pairs1", "pairs2", "pairs3", "reads_removed", "entries_removed", "rounds_run")
long_paths = br.long_paths


def r_pairs(M, rows, cols, vals, cutoff=0.0, fuzz=0):
    """The set of (i, j), i < j, that the symmetrised R of a reduction of these overlaps holds."""
    rows = np.asarray(rows, dtype=np.int64); cols = np.asarray(cols, dtype=np.int64); vals = np.asarray(vals)
    _, flags, _ = po.string_graph(M, rows, cols, vals, cutoff, fuzz)
    keep = (vals["passed"] != 0) & ((flags[rows] & 3) == 0) & ((flags[cols] & 3) == 0) if len(rows) else np.zeros(0, dtype=bool)
    return frozenset(zip(rows[keep].tolist(), cols[keep].tolist()))


def resolve_stars(M, rows, cols, vals, R, rounds=1, trace=None):
    """Returns (rows, cols, vals, flags, stats).  trace, a list, receives per round dict(centres=[(u, e, odd arm or None)], odd=set)."""
    assert 1 <= int(rounds) <= 64
    rows = [int(r) for r in rows]; cols = [int(c) for c in cols]
    n = len(rows)
    live = list(range(n))
    flags = np.zeros(M, dtype=np.uint8)
    centres, by_e, reads_removed, rounds_run = 0, [0, 0, 0, 0], 0, 0
    for _ in range(int(rounds)):
        rounds_run += 1
        # the tables of the round, frozen
        column = {}                                             # c -> the rows of its entries, in their order
        for z in live:
            column.setdefault(cols[z], []).append(rows[z])
        deg = {v: len(column.get(v, ())) for v in range(M)}
        odd, seen = set(), []
        for u in range(M):
            # centre
            if deg[u] != 3:
                continue
            x1, x2, x3 = column[u]
            assert x1 < x2 < x3
            if not (deg[x1] == 2 and deg[x2] == 2 and deg[x3] == 2):
                continue
            centres += 1
            # pairs in R
            present = [p for p in ((x1, x2), (x1, x3), (x2, x3)) if p in R]
            e = len(present)
            by_e[e] += 1
            # odd arm
            w = None
            if e == 1:
                (w,) = {x1, x2, x3} - set(present[0])
                odd.add(w)
            seen.append((u, e, w))
        if trace is not None:
            trace.append(dict(centres=seen, odd=set(odd)))
        if not odd:                                             # a round that removed nothing: the call stops, and the round counts
            break
        # removal
        for w in odd:
            flags[w] |= 32
        reads_removed += len(odd)
        live = [z for z in live if rows[z] not in odd and cols[z] not in odd]
    st = dict(nreads=M, nnz_before=n, nnz_after=len(live), centres=centres, pairs0=by_e[0], pairs1=by_e[1], pairs2=by_e[2], pairs3=by_e[3],
              reads_removed=reads_removed, entries_removed=n - len(live), rounds_run=rounds_run)
    idx = np.array(live, dtype=np.int64)
    return np.asarray(rows, dtype=np.int64)[idx], np.asarray(cols, dtype=np.int64)[idx], np.asarray(vals)[idx], flags, st


def resolve_stars_peel(M, rows, cols, vals, R, rounds=1, order=None):
    """The same result from neighbour sets: within a round the reads are visited in the order `order` gives (a permutation of the reads;
    default: descending), the odd arms are collected, and only then taken out.  Returns (rows, cols, vals, flags, stats)."""
    rows = np.asarray(rows, dtype=np.int64); cols = np.asarray(cols, dtype=np.int64)
    assert set(zip(rows.tolist(), cols.tolist())) == set(zip(cols.tolist(), rows.tolist())), "resolve_stars_peel needs both triangles"
    order = list(range(M - 1, -1, -1)) if order is None else [int(v) for v in order]
    nb = [set() for _ in range(M)]
    for r, c in zip(rows.tolist(), cols.tolist()):
        nb[c].add(r)
    overlaps = [set() for _ in range(M)]                        # R as neighbour sets
    for a, b in R:
        overlaps[a].add(b); overlaps[b].add(a)
    dead = np.zeros(M, dtype=bool)
    tally = {0: 0, 1: 0, 2: 0, 3: 0}
    runs = ncentres = 0
    for _ in range(int(rounds)):
        runs += 1
        batch = []
        for u in order:
            if len(nb[u]) != 3 or any(len(nb[x]) != 2 for x in nb[u]):
                continue
            ncentres += 1
            links = {x: len(overlaps[x] & (nb[u] - {x})) for x in nb[u]}       # how many of the other two each neighbour overlaps
            tally[sum(links.values()) // 2] += 1
            if sorted(links.values()) == [0, 1, 1]:
                batch.append(min(links, key=links.get))
        batch = set(batch)
        if not batch:
            break
        for w in batch:
            for y in nb[w]:
                nb[y].discard(w)
            nb[w] = set()
            dead[w] = True
    present = ~(dead[rows] | dead[cols]) if len(rows) else np.zeros(0, dtype=bool)
    flags = np.where(dead, 32, 0).astype(np.uint8)
    st = dict(nreads=M, nnz_before=len(rows), nnz_after=int(present.sum()), centres=ncentres, pairs0=tally[0], pairs1=tally[1], pairs2=tally[2], pairs3=tally[3],
              reads_removed=int(dead.sum()), entries_removed=int((~present).sum()), rounds_run=runs)
    return rows[present], cols[present], np.asarray(vals)[present], flags, st


def same(a, b, keys=STATS):
    """Two results (rows, cols, vals, flags, stats) are equal entry for entry, and field for field in `keys`."""
    ok = len(a[0]) == len(b[0]) and (a[0] == b[0]).all() and (a[1] == b[1]).all() and a[2].tobytes() == b[2].tobytes()
    return bool(ok and (a[3] == b[3]).all() and all(a[4][k] == b[4][k] for k in keys))


def simplify(M, rows, cols, vals, R, max_tip_reads, max_arm_reads, stars=64, q16=None, bridges=None, passes=16):
    """The restatements in the order Engine.simplify_graph(.., min_overlap_ratio, bridges, stars) runs the calls.  Returns (rows, cols, vals,
    flags, [(tip stats, bubble stats, [weak stats,] [bridge stats,] star stats)])."""
    flags = np.zeros(M, dtype=np.uint8)
    out = []
    for _ in range(passes):
        rows, cols, vals, f1, s1 = tu.clip_tips(M, rows, cols, vals, max_tip_reads, 64)
        rows, cols, vals, f2, s2 = bu.pop_bubbles(M, rows, cols, vals, max_arm_reads, 64)
        p = (s1, s2)
        flags |= f1 | f2
        idle = s1["reads_removed"] == 0 and s2["reads_removed"] == 0
        if q16 is not None:
            rows, cols, vals, s3 = wu.cut_weak(M, rows, cols, vals, q16)
            p += (s3,)
            idle = idle and s3["entries_removed"] == 0
        if bridges is not None:
            rows, cols, vals, f4, s4 = br.cut_bridges(M, rows, cols, vals, *bridges)
            p += (s4,)
            flags |= f4
            idle = idle and s4["reads_removed"] == 0
        rows, cols, vals, f5, s5 = resolve_stars(M, rows, cols, vals, R, stars)
        p += (s5,)
        flags |= f5
        idle = idle and s5["reads_removed"] == 0
        out.append(p)
        if idle:
            break
    return rows, cols, vals, flags, out


class StarGraph(tu.Graph):
    """tip_util.Graph, plus pairs that are in R only and pairs of which S keeps one image."""

    def __init__(self):
        super().__init__()
        self.ronly = []
        self.single = set()

    def rpair(self, u, v):
        self.ronly.append((u, v))

    def one_image(self, u, v):
        """Links u and v by a pair whose directionT is -1: the reduction keeps S(row min, col max) and not its mirror image."""
        self.link(u, v)
        self.single.add((u, v))

    def overlaps(self, rng, perm=None, M=None):
        """As tip_util.Graph.overlaps; an R-only pair is passed and has direction = directionT = -1 (tr.hip's k_tr_emit keeps it in R,
        k_tr_mark forms no product with it, k_tr_select drops it)."""
        M = self.n if M is None else M
        edges = {}
        for kind, plist in (("S", self.pairs), ("R", self.ronly)):
            for u0, v0 in plist:
                u, v = (int(perm[u0]), int(perm[v0])) if perm is not None else (u0, v0)
                i, j = min(u, v), max(u, v)
                assert i != j and (i, j) not in edges, (i, j)
                o = cu.edge(rng, 20, 20)
                o["suffix"] = int(rng.integers(5, 10)); o["suffixT"] = int(rng.integers(5, 10))
                if kind == "R":
                    o["direction"] = -1; o["directionT"] = -1
                elif (u0, v0) in self.single:
                    o["directionT"] = -1
                edges[(i, j)] = o
        return (M,) + cu.upper(edges)

    def without_ronly(self):
        g = StarGraph()
        g.n, g.pairs, g.single = self.n, list(self.pairs), set(self.single)
        return g


def _star(g, tails=(2, 2, 2), pairs=()):
    """A read u with one arm per element of tails (arm i: tails[i] new reads in a chain, u's neighbour first; 2 or more make the neighbour
    a read of degree 2), and the pairs (i, j) of arms' first reads planted as R-only pairs.  u < arm 0 < arm 1 < ...  Returns (u, arms)."""
    u = g.new()[0]
    arms = [g.arm(u, t) for t in tails]
    for i, j in pairs:
        g.rpair(arms[i][0], arms[j][0])
    return u, arms


def _case(g, removed, centres, by_e, deg, deg_after, moves, perm=None, **more):
    if perm is not None:
        removed = {int(perm[v]) for v in removed}
        deg = {int(perm[v]): d for v, d in deg.items()}; deg_after = {int(perm[v]): d for v, d in deg_after.items()}
    return dict(graph=g, perm=perm, removed=set(removed), centres=centres, by_e=tuple(by_e), deg=deg, deg_after=deg_after, moves=moves, **more)


def _place(n, first, last):
    """A permutation of n reads that sends `first` to 0 and `last` to n - 1 and keeps the others in order."""
    rest = [v for v in range(n) if v not in (first, last)]
    perm = np.zeros(n, dtype=np.int64)
    perm[first], perm[last] = 0, n - 1
    perm[rest] = np.arange(1, n - 1)
    return perm


def star_chain(g, K):
    """K stars in a row of which round k resolves the k-th and no other: centre c_k has the neighbours y_(k-1) (a_1 for the first), b_k and
    w_k; {y_(k-1), b_k} is a pair in R, so w_k is c_k's odd arm.  w_k's other neighbour y_k has degree 3 (w_k, c_(k+1), a dead end q_k)
    until w_k goes: only then has c_(k+1) three neighbours of degree 2.  The last w's other neighbour is a dead end.  Returns
    (centres, odd arms)."""
    cs, ws = [], []
    prev = g.new()[0]                                           # a_1, with a dead end behind it
    g.arm(prev, 1)
    for k in range(K):
        c = g.new()[0]
        g.link(prev, c)
        b = g.arm(c, 2)[0]
        w = g.arm(c, 1)[0]
        g.rpair(prev, b)
        y = g.new()[0]
        g.link(w, y)
        if k < K - 1:
            g.arm(y, 1)                                         # q_k: y has degree 3 once c_(k+1) is linked to it
        cs.append(c); ws.append(w)
        prev = y
    return cs, ws


def hand_cases():
    """name -> dict(graph, perm, and the claims: removed (a set of reads), centres and by_e = (pairs0 .. pairs3) summed over the rounds of a
    call with rounds = 64, deg {read: degree} before, deg_after, moves = the rounds that remove something)."""
    cases = {}
    P = {"01": (0, 1), "02": (0, 2), "12": (1, 2)}
    # e = 0 .. 3 on a plain star: arms of two reads.  e = 1 once per pair, the odd arm in each slot
    g = StarGraph(); u, arms = _star(g)
    cases["e0_no_pair_in_R_left_alone"] = _case(g, (), 1, (1, 0, 0, 0), {u: 3, arms[0][0]: 2, arms[1][0]: 2, arms[2][0]: 2}, {u: 3, arms[2][0]: 2}, 0)
    for name, odd in (("12", 0), ("02", 1), ("01", 2)):
        g = StarGraph(); u, arms = _star(g, pairs=[P[name]])
        w = arms[odd][0]
        cases["e1_pair_%s_odd_arm_in_slot_%d" % (name, odd)] = _case(g, {w}, 1, (0, 1, 0, 0), {u: 3, w: 2, arms[odd][1]: 1},
                                                                    {u: 2, w: 0, arms[odd][1]: 0, arms[(odd + 1) % 3][0]: 2}, 1)
    for name in ("01_02", "01_12", "02_12"):
        g = StarGraph(); u, arms = _star(g, pairs=[P[x] for x in name.split("_")])
        cases["e2_pairs_%s_left_alone" % name] = _case(g, (), 1, (0, 0, 1, 0), {u: 3}, {u: 3, arms[0][0]: 2}, 0)
    g = StarGraph(); u, arms = _star(g, pairs=list(P.values()))
    cases["e3_all_three_pairs_left_alone"] = _case(g, (), 1, (0, 0, 0, 1), {u: 3}, {u: 3, arms[1][0]: 2}, 0)
    # a neighbour of degree 1 or 3: no centre, whatever R says
    for slot in range(3):
        g = StarGraph(); u, arms = _star(g, tails=tuple(1 if i == slot else 2 for i in range(3)), pairs=[P["12" if slot == 0 else "02" if slot == 1 else "01"]])
        cases["neighbour_%d_of_degree_1_no_centre" % slot] = _case(g, (), 0, (0, 0, 0, 0), {u: 3, arms[slot][0]: 1}, {u: 3}, 0)
        g = StarGraph(); u, arms = _star(g, pairs=[P["12" if slot == 0 else "02" if slot == 1 else "01"]])
        g.arm(arms[slot][0], 1)
        cases["neighbour_%d_of_degree_3_no_centre" % slot] = _case(g, (), 0, (0, 0, 0, 0), {u: 3, arms[slot][0]: 3}, {u: 3}, 0)
    # a read of degree 4 (and of 2) with the pair in R: no centre
    g = StarGraph(); u, arms = _star(g, tails=(2, 2, 2, 2), pairs=[(0, 1)])
    cases["centre_of_degree_4_no_centre"] = _case(g, (), 0, (0, 0, 0, 0), {u: 4}, {u: 4}, 0)
    g = StarGraph(); u, arms = _star(g, tails=(2, 2), pairs=[(0, 1)])
    cases["read_of_degree_2_no_centre"] = _case(g, (), 0, (0, 0, 0, 0), {u: 2}, {u: 2}, 0)
    # the pair of R joins a neighbour and a read that is no neighbour, or the centre and a neighbour: neither counts
    g = StarGraph(); u, arms = _star(g)
    g.rpair(arms[0][0], arms[1][1]); g.rpair(arms[2][0], arms[0][1])
    cases["pairs_of_R_that_join_no_two_neighbours_do_not_count"] = _case(g, (), 1, (1, 0, 0, 0), {u: 3}, {u: 3}, 0)
    # two centres that share a neighbour w: the odd arm of u1, a paired arm of u2 — u2 loses w and its own odd arm d
    g = StarGraph()
    u1 = g.new()[0]; a = g.arm(u1, 2)[0]; b = g.arm(u1, 2)[0]; w = g.arm(u1, 1)[0]
    u2 = g.new()[0]; g.link(w, u2); c = g.arm(u2, 2)[0]; d = g.arm(u2, 2)[0]
    g.rpair(a, b); g.rpair(w, c)
    cases["two_centres_share_the_odd_arm_of_one_which_is_a_paired_arm_of_the_other"] = _case(
        g, {w, d}, 2, (0, 2, 0, 0), {u1: 3, u2: 3, w: 2, d: 2}, {u1: 2, u2: 1, w: 0, d: 0, c: 2}, 1)
    # two centres with the same three neighbours: both name w, which goes once
    g = StarGraph()
    u1, u2 = g.new(2)
    a, b, w = g.new(3)
    for x in (a, b, w):
        g.link(u1, x); g.link(u2, x)
    g.rpair(a, b)
    cases["two_centres_with_the_same_three_neighbours_one_removal"] = _case(g, {w}, 2, (0, 2, 0, 0), {u1: 3, u2: 3, a: 2, b: 2, w: 2}, {u1: 2, u2: 2, w: 0, a: 2}, 1)
    # ... and they disagree: u1 and u2 see the same R, so they cannot; but two centres can name two different arms of a shared pair of neighbours
    g = StarGraph()
    u1, u2 = g.new(2)
    a, b = g.new(2)
    for x in (a, b):
        g.link(u1, x); g.link(u2, x)
    w1 = g.arm(u1, 2)[0]; w2 = g.arm(u2, 2)[0]
    g.rpair(a, b)
    cases["two_centres_share_the_paired_arms_each_loses_its_own"] = _case(g, {w1, w2}, 2, (0, 2, 0, 0), {u1: 3, u2: 3, a: 2, b: 2}, {u1: 2, u2: 2, a: 2, b: 2, w1: 0}, 1)
    # a removal makes a new centre: exactly K rounds remove something (K across SG_BATCH = 4)
    for K in (2, 4, 5, 9):
        g = StarGraph(); cs, ws = star_chain(g, K)
        cases["chain_of_%d_stars_needs_%d_rounds" % (K, K)] = _case(g, set(ws), K, (0, K, 0, 0), {cs[0]: 3, cs[-1]: 3, ws[0]: 2}, {c: 2 for c in cs}, K, chain=(cs, ws))
    # a centre, or an arm, at read 0 and at read M - 1
    for name in ("centre_0_odd_arm_last", "centre_last_odd_arm_0", "paired_arm_0_centre_last", "odd_arm_0_paired_arm_last", "random_relabelling"):
        g = StarGraph(); u, arms = _star(g, pairs=[(0, 1)])
        w = arms[2][0]
        if name == "random_relabelling":
            perm = np.random.default_rng(5).permutation(g.n)
        else:
            first, last = {"centre_0_odd_arm_last": (u, w), "centre_last_odd_arm_0": (w, u), "paired_arm_0_centre_last": (arms[0][0], u),
                           "odd_arm_0_paired_arm_last": (w, arms[1][0])}[name]
            perm = _place(g.n, first, last)
        cases["star_%s" % name] = _case(g, {w}, 1, (0, 1, 0, 0), {u: 3, w: 2, arms[0][0]: 2, arms[1][0]: 2}, {u: 2, w: 0}, 1, perm=perm)
    # one-image pairs: the statements on the columns as they are
    # column u holds x3, column x3 does not hold u (u is the larger read): x3 has two other entries, so it has degree 2, and it is the odd arm
    g = StarGraph()
    x1, x2, x3 = g.new(3)
    for x in (x1, x2):
        g.arm(x, 1)
    g.arm(x3, 1); g.arm(x3, 1)
    u = g.new()[0]
    g.link(x1, u); g.link(x2, u); g.one_image(x3, u)
    g.rpair(x1, x2)
    cases["one_image_column_of_the_centre_holds_the_arm_whose_column_does_not_hold_it"] = _case(g, {x3}, 1, (0, 1, 0, 0), {u: 3, x3: 2}, {u: 2, x3: 0}, 1, one_image=True)
    # u has four partners, but column u does not hold the fourth (u is the smaller read): degree 3, a centre
    g = StarGraph(); u, arms = _star(g, pairs=[(0, 1)])
    x4 = g.new()[0]
    g.one_image(u, x4)
    cases["one_image_fourth_partner_not_in_the_centres_column"] = _case(g, {arms[2][0]}, 1, (0, 1, 0, 0), {u: 3, x4: 1}, {u: 2, x4: 1}, 1, one_image=True)
    # the arm's own column lacks its tail (one image): degree 1, no centre
    g = StarGraph(); u = g.new()[0]
    arms = [g.arm(u, 2), g.arm(u, 2)]
    x3, t3 = g.new(2)
    g.link(u, x3); g.one_image(x3, t3)
    arms.append([x3, t3])
    g.rpair(arms[0][0], arms[1][0])
    cases["one_image_arm_whose_column_lacks_its_tail_has_degree_1_no_centre"] = _case(g, (), 0, (0, 0, 0, 0), {u: 3, x3: 1, t3: 1}, {u: 3}, 0, one_image=True)
    return cases


def case_overlaps(case, rng, extra_reads=0):
    """(M, rows, cols, vals) of a hand case for elba_set_overlaps; extra_reads isolated reads follow the graph's."""
    g = case["graph"]
    return g.overlaps(rng, perm=case.get("perm"), M=g.n + extra_reads)


LOOKUP_LENGTHS = (2, 3, 4, 64, 65, 2048, 2049)
LOOKUP_PLACES = ("first", "last", "below", "above", "between")


def lookup_case(length, place, short):
    """A star u with neighbours x0, x1, x2 whose pair {x0, x1} is the one R is asked about.  s = x_short is the read with the shorter row
    of R, of exactly `length` entries: u, its tail t_s, fillers (isolated reads, R-only pairs), and the key k = x_(1 - short) when `place`
    says it is present ("first": every other column of the row is above k; "last": every other one below).  When k is absent ("below":
    every column above k; "above": every column below; "between": some on each side) e is 0.  The other read's row has length + 7 entries:
    long too, and never the one searched.  Returns (M, rows, cols, vals, dict(u, s, k, odd, present)); the reads are renamed so that the
    order of ids is what `place` asks for.
    A row of R of length 1 cannot be searched: a neighbour of a centre has degree 2, so its row of R holds its two partners in S at least;
    for the same reason a row of length 2 cannot hold the key."""
    present = place in ("first", "last")
    assert length >= (3 if present else 2)
    g = StarGraph()
    u, arms = _star(g)
    s, k = arms[short][0], arms[1 - short][0]
    nfill = length - 2 - (1 if present else 0)
    fill_s = g.new(nfill)
    fill_k = g.new(length + 7 - 2 - (1 if present else 0))
    for f in fill_s:
        g.rpair(s, f)
    for f in fill_k:
        g.rpair(k, f)
    if present:
        g.rpair(s, k)
    # sort keys: k at 0; the columns of row s (u, s's tail, its fillers) below or above it; everything else further out, in order
    others = [u, arms[short][1]] + fill_s
    if place in ("first", "below"):
        side = [1] * len(others)
    elif place in ("last", "above"):
        side = [-1] * len(others)
    else:
        side = [(-1) ** i for i in range(len(others))]          # u below k, the tail above, fillers alternating
    key = {v: 10.0 * (v + 1) * (1 if v % 2 else -1) for v in range(g.n)}       # any distinct keys far from 0 on both sides
    for i, (v, sd) in enumerate(zip(others, side)):
        key[v] = sd * (1 + i) * 0.001
    key[k] = 0.0
    key[s] = 5.0 if short == 0 else -5.0                        # s above k, or below it: the look-up is asked as (k, s) or as (s, k)
    ranked = sorted(range(g.n), key=key.get)
    perm = np.zeros(g.n, dtype=np.int64)
    perm[ranked] = np.arange(g.n)
    M, rows, cols, vals = g.overlaps(np.random.default_rng(length * 10 + short), perm=perm)
    info = dict(u=int(perm[u]), s=int(perm[s]), k=int(perm[k]), odd=int(perm[arms[2][0]]), present=present, row=sorted(int(perm[v]) for v in others))
    return M, rows, cols, vals, info


def plant_stars(rng, M, rows, cols, vals, n, gap=4, pairs_in_R=1):
    """Plants n stars into a graph of long paths of consecutive reads (br.long_paths): at n inner reads u, a multiple of gap + 1 reads from
    the start of their path, a stray read w (new, ids from M on) with one more new read behind it, so that w has degree 2, and the pair
    {u - 1, u + 1} as an R-only entry (pairs_in_R = 1; 0: none).  Returns (M', rows, cols, vals, centres, odd arms), (row, col) order."""
    rows = np.asarray(rows, dtype=np.int64); cols = np.asarray(cols, dtype=np.int64)
    assert (cols == rows + 1).all()
    starts = np.concatenate([[0], np.flatnonzero(np.diff(rows) != 1) + 1]).astype(np.int64)
    slots = []
    for a, b in zip(starts.tolist(), starts[1:].tolist() + [len(rows)]):
        first, last = int(rows[a]), int(cols[b - 1])            # the path's two end reads
        slots += list(range(first + gap + 1, last - gap, gap + 1))
    assert len(slots) >= n, (len(slots), n)
    centres = np.sort(rng.choice(np.array(slots, dtype=np.int64), size=n, replace=False))
    w = M + 2 * np.arange(n, dtype=np.int64)
    xr = np.concatenate([centres, w, centres - 1] if pairs_in_R else [centres, w])
    xc = np.concatenate([w, w + 1, centres + 1] if pairs_in_R else [w, w + 1])
    xv = np.zeros(len(xr), dtype=np.asarray(vals).dtype)
    xv["passed"] = 1
    xv["direction"] = rng.integers(0, 4, len(xr)); xv["directionT"] = rng.integers(0, 4, len(xr))
    xv["suffix"] = rng.integers(5, 10, len(xr)); xv["suffixT"] = rng.integers(5, 10, len(xr))
    if pairs_in_R:
        xv["direction"][2 * n:] = -1; xv["directionT"][2 * n:] = -1
    r = np.concatenate([rows, xr]); c = np.concatenate([cols, xc]); v = np.concatenate([np.asarray(vals), xv])
    assert (r < c).all()
    order = np.lexsort((c, r))
    return M + 2 * n, r[order], c[order], v[order], centres, w


def layout_stars(seed, M=5, every=None):
    """Reads 0 .. M - 1 of string_graph_util.layout_overlaps at a coverage at which each overlaps the next two at least, every pair passed,
    with both directions and uncontained: the reduction at fuzz 1000 removes the pairs with a read between them as transitive, and they
    stay in R.  Behind every read u in `every` (default: the middle one) a stray read w with one more read behind it.  {u - 1, u + 1} is
    then a pair in R because the device's own reduction put it there.  Returns (M', rows, cols, vals, centres, odd arms); reduce with
    cutoff 0.65, fuzz 1000."""
    rng = np.random.default_rng(seed)
    rows, cols, vals = sgu.layout_overlaps(rng, M, 8, p_fail=0.0, p_nodir=0.0, p_contained=0.0)
    centres = np.array([M // 2] if every is None else list(every), dtype=np.int64)
    n = len(centres)
    w = M + 2 * np.arange(n, dtype=np.int64)
    xr = np.concatenate([centres, w]); xc = np.concatenate([w, w + 1])
    xv = np.zeros(2 * n, dtype=vals.dtype)
    xv["passed"] = 1
    xv["direction"] = rng.integers(0, 4, 2 * n); xv["directionT"] = rng.integers(0, 4, 2 * n)
    xv["suffix"] = rng.integers(3000, 6000, 2 * n); xv["suffixT"] = rng.integers(3000, 6000, 2 * n)
    r = np.concatenate([rows, xr]); c = np.concatenate([cols, xc]); v = np.concatenate([vals, xv])
    order = np.lexsort((c, r))
    return M + 2 * n, r[order], c[order], v[order], centres, w


def random_stars(seed, p_one_image=0.0):
    """rounds_util.random_graph(seed) — no triangle, so no two neighbours of a read are partners — with R-only pairs among the neighbours of
    its reads of degree 3 (none, one, two or all three of the pairs, mostly one), tails that make more of those neighbours reads of degree
    2, and a few R-only pairs anywhere.  p_one_image: that share of the pairs gets directionT -1.  Returns (M, rows, cols, vals)."""
    M, rows, cols, vals, _, _ = ru.random_graph(seed)
    rng = np.random.default_rng(seed + 5000)
    have = set(zip(rows.tolist(), cols.tolist()))
    nb = [[] for _ in range(M)]
    for r, c in have:
        nb[r].append(c); nb[c].append(r)
    extra = {}
    for u in range(M):
        if len(nb[u]) != 3:
            continue
        three = [(a, b) for a in nb[u] for b in nb[u] if a < b]
        k = int(rng.choice([0, 1, 1, 1, 1, 2, 3]))
        for i in rng.choice(3, size=k, replace=False):
            extra[three[int(i)]] = 1
    for _ in range(M // 10):
        a, b = sorted(int(x) for x in rng.integers(0, M, 2))
        if a != b and (a, b) not in have:
            extra[(a, b)] = 1
    xr = np.array([p[0] for p in sorted(extra)], dtype=np.int64); xc = np.array([p[1] for p in sorted(extra)], dtype=np.int64)
    xv = np.zeros(len(xr), dtype=vals.dtype)
    xv["passed"] = 1; xv["direction"] = -1; xv["directionT"] = -1
    xv["suffix"] = rng.integers(5, 10, len(xr)); xv["suffixT"] = rng.integers(5, 10, len(xr))
    vals = vals.copy()
    if p_one_image:
        vals["directionT"][rng.random(len(vals)) < p_one_image] = -1
    r = np.concatenate([rows, xr]); c = np.concatenate([cols, xc]); v = np.concatenate([vals, xv])
    order = np.lexsort((c, r))
    return M, r[order], c[order], v[order]
