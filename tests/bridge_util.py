"""Cutting bridges (elba_cut_bridges, elba_amd/csrc/bridges.hip) restated in plain Python, twice, and the hand-made graphs the test files use.

cut_bridges          the rule of include/elba_amd.h statement by statement: dictionaries and lists, one pass on frozen tables.  Input: (M, rows,
                     cols, vals) of S in export order (columns ascending, rows ascending within a column).  Returns the cut S, the flags (bit
                     4 of every removed read) and every field of the stats except the times.
cut_bridges_peel     a second implementation that shares nothing with the first and runs on the CPU only: neighbour SETS that change as it
                     goes (no column order, no frozen table), anchors visited in the order the caller's permutation gives, every candidate
                     re-decided on the graph as it is then and removed at once.  It needs a symmetric S.  By guarantees 1 and 3 of the header
                     it must give the same S, flags, bridges and removed counts whatever the order; it does not compute chains and long_flanks.
simplify             clip_tips(.., 64), pop_bubbles(.., 64), [cut_weak], cut_bridges of the restatements until a pass removes nothing: what
                     Engine.simplify_graph(.., bridges=..) is held against.
hand_cases           graphs named after the clause of the rule they show, with what each claims (removed set, degrees before and after,
                     chains, long_flanks, bridges), so that a case that does not show what its name says fails in test_bridges_cpu.py.
                     F is min_flank_reads, mx max_bridge_reads.
long_paths, plant_bridges
                     paths of consecutive reads, and H's planted into them: a chain of t new reads between two inner reads of paths, every
                     anchor at least `gap` reads from the next anchor and from its path's ends."""
import numpy as np

import bubble_util as bu
import tip_util as tu
import weak_util as wu
from oracle import pyoracle as po

STATS = ("nreads", "nnz_before", "nnz_after", "anchors", "chains", "long_flanks", "bridges", "reads_removed", "entries_removed")
PEEL_STATS = ("nreads", "nnz_before", "nnz_after", "bridges", "reads_removed", "entries_removed")
PARAMS = ((1, 2), (2, 3), (3, 7))                               # (mx, F) of the H-based hand cases


def cut_bridges(M, rows, cols, vals, max_bridge_reads, min_flank_reads, trace=None):
    """Returns (rows, cols, vals, flags, stats).  trace, a dict, receives chains = [(a, b, reads)], long = {(u, w)} and bridges = [(a, b, reads)]."""
    mx, F = int(max_bridge_reads), int(min_flank_reads)
    assert 1 <= mx <= 65534 and mx < F <= 65535
    rows = [int(r) for r in rows]; cols = [int(c) for c in cols]
    n = len(rows)
    column = {}                                                 # c -> the rows of its entries, in their order
    for z in range(n):
        column.setdefault(cols[z], []).append(rows[z])
    deg = {v: len(column.get(v, ())) for v in range(M)}

    def onward(cur, came_from):                                 # from a read of degree 2: the first row of its column that is not the read it came from
        return [x for x in column[cur] if x != came_from][0]

    # anchors
    anchors = [v for v in range(M) if deg[v] >= 3]
    # chains: exactly the arms of elba_pop_bubbles
    chains = []
    for a in anchors:
        for v1 in column[a]:
            if deg[v1] != 2:
                continue
            reads, prev, cur = [], a, v1
            while True:
                if deg[cur] >= 3:
                    if cur > a:                                 # recorded at the smaller anchor; b == a is no chain
                        chains.append((a, cur, tuple(reads)))
                    break
                if deg[cur] != 2 or len(reads) == mx:           # a read of degree 0 or 1, or read mx + 1
                    break
                reads.append(cur)
                prev, cur = cur, onward(cur, prev)
    # flanks: for a read u of degree exactly 3 and an entry of its column with row w
    long_flank = set()
    for u in range(M):
        if deg[u] != 3:
            continue
        for w in column[u]:
            count, prev, cur = 0, u, w
            while count < F and deg[cur] == 2:
                count += 1
                prev, cur = cur, onward(cur, prev)
            if count == F:
                long_flank.add((u, w))
    # bridges
    bridges = []
    for a, b, reads in chains:
        v1, vt = reads[0], reads[-1]
        if deg[a] != 3 or deg[b] != 3:
            continue
        if not all((a, w) in long_flank for w in column[a] if w != v1):
            continue
        if vt not in column[b]:                                 # (only where S holds one image of a pair)
            continue
        if not all((b, w) in long_flank for w in column[b] if w != vt):
            continue
        bridges.append((a, b, reads))
    # removal
    removed = set()
    for _, _, reads in bridges:
        removed |= set(reads)
    flags = np.zeros(M, dtype=np.uint8)
    for v in removed:
        flags[v] |= 16
    live = [z for z in range(n) if rows[z] not in removed and cols[z] not in removed]
    st = dict(nreads=M, nnz_before=n, nnz_after=len(live), anchors=len(anchors), chains=len(chains), long_flanks=len(long_flank), bridges=len(bridges),
              reads_removed=len(removed), entries_removed=n - len(live))
    if trace is not None:
        trace.update(chains=chains, long=long_flank, bridges=bridges)
    idx = np.array(live, dtype=np.int64)
    return np.asarray(rows, dtype=np.int64)[idx], np.asarray(cols, dtype=np.int64)[idx], np.asarray(vals)[idx], flags, st


def cut_bridges_peel(M, rows, cols, vals, max_bridge_reads, min_flank_reads, order=None):
    """The same S and flags by peeling: anchors in the order `order` gives (a permutation of the reads; default: descending), every bridge
    found removed at once from neighbour sets, the next one decided on what is left.  Returns (rows, cols, vals, flags, stats of PEEL_STATS)."""
    mx, F = int(max_bridge_reads), int(min_flank_reads)
    rows = np.asarray(rows, dtype=np.int64); cols = np.asarray(cols, dtype=np.int64)
    assert set(zip(rows.tolist(), cols.tolist())) == set(zip(cols.tolist(), rows.tolist())), "cut_bridges_peel needs both triangles"
    order = list(range(M - 1, -1, -1)) if order is None else [int(v) for v in order]
    nb = [set() for _ in range(M)]
    for r, c in zip(rows.tolist(), cols.tolist()):
        nb[c].add(r)

    def run(u, w):
        """The reads of degree 2 from w on, away from u, and the read that ends them; at most `F` of them are looked at."""
        reads, prev, cur = [], u, w
        while len(nb[cur]) == 2 and len(reads) < F:
            reads.append(cur)
            (nxt,) = nb[cur] - {prev}                           # symmetric: cur was reached from prev, which is one of its two neighbours
            prev, cur = cur, nxt
        return reads, cur

    def two_long_flanks(u, but):
        return all(len(run(u, w)[0]) >= F for w in nb[u] if w != but)

    gone, nbridges = [], 0
    for a in order:
        if len(nb[a]) != 3:
            continue
        for v1 in sorted(nb[a]):
            if len(nb[v1]) != 2:
                continue
            reads, b = run(a, v1)
            if len(nb[b]) == 2 or len(reads) > mx or b == a or len(nb[b]) != 3:      # ran on past F reads; too long; a loop; a dead end or a hub
                continue
            if two_long_flanks(a, v1) and two_long_flanks(b, reads[-1]):
                for v in reads:
                    for w in nb[v]:
                        nb[w].discard(v)
                    nb[v] = set()
                gone += reads
                nbridges += 1
                break                                           # a has degree 2 now
    dead = np.zeros(M, dtype=bool)
    dead[gone] = True
    assert len(gone) == int(dead.sum())
    present = ~(dead[rows] | dead[cols])
    flags = np.where(dead, 16, 0).astype(np.uint8)
    st = dict(nreads=M, nnz_before=len(rows), nnz_after=int(present.sum()), bridges=nbridges, reads_removed=len(gone), entries_removed=int((~present).sum()))
    return rows[present], cols[present], np.asarray(vals)[present], flags, st


def same(a, b, keys=STATS):
    """Two results (rows, cols, vals, flags, stats) are equal entry for entry, and field for field in `keys`."""
    ok = len(a[0]) == len(b[0]) and (a[0] == b[0]).all() and (a[1] == b[1]).all() and a[2].tobytes() == b[2].tobytes()
    return bool(ok and (a[3] == b[3]).all() and all(a[4][k] == b[4][k] for k in keys))


def simplify(M, rows, cols, vals, max_tip_reads, max_arm_reads, bridges, q16=None, passes=16):
    """The restatements in the order Engine.simplify_graph(.., min_overlap_ratio, bridges) runs the calls.  Returns (rows, cols, vals, flags,
    [(tip stats, bubble stats, [weak stats,] bridge stats)])."""
    flags = np.zeros(M, dtype=np.uint8)
    out = []
    for _ in range(passes):
        rows, cols, vals, f1, s1 = tu.clip_tips(M, rows, cols, vals, max_tip_reads, 64)
        rows, cols, vals, f2, s2 = bu.pop_bubbles(M, rows, cols, vals, max_arm_reads, 64)
        p = (s1, s2)
        idle = s1["reads_removed"] == 0 and s2["reads_removed"] == 0
        if q16 is not None:
            rows, cols, vals, s3 = wu.cut_weak(M, rows, cols, vals, q16)
            p += (s3,)
            idle = idle and s3["entries_removed"] == 0
        rows, cols, vals, f4, s4 = cut_bridges(M, rows, cols, vals, *bridges)
        p += (s4,)
        idle = idle and s4["reads_removed"] == 0
        flags |= f1 | f2 | f4
        out.append(p)
        if idle:
            break
    return rows, cols, vals, flags, out


def _tail(g, u, n2, end="dead"):
    """Hangs a flank of n2 reads of degree 2 off u.  end "dead": a read of degree 1 follows them; "anchor": a read of degree 3 with two
    dead-end chains of two reads.  Returns (the n2 reads, the read that ends them)."""
    ids = g.arm(u, n2 + 1)
    if end == "anchor":
        g.arm(ids[-1], 2); g.arm(ids[-1], 2)
    return ids[:-1], ids[-1]


def _h(g, t, flanks, ends=("dead",) * 4):
    """a with flanks[0], flanks[1] and b with flanks[2], flanks[3] (reads of degree 2 each, None: no such flank), joined by a chain of t
    reads (0: a direct entry).  a and its flanks come first, then the chain, then b: a < chain < b.  Returns (a, b, chain, flank read lists)."""
    a = g.new()[0]
    fl = [None] * 4
    for i in (0, 1):
        if flanks[i] is not None:
            fl[i] = _tail(g, a, flanks[i], ends[i])[0]
    ch = g.new(t)
    b = g.new()[0]
    g.chain([a] + ch + [b])
    for i in (2, 3):
        if flanks[i] is not None:
            fl[i] = _tail(g, b, flanks[i], ends[i])[0]
    return a, b, ch, fl


def _case(g, mx, F, removed, chains, long_flanks, bridges, deg, deg_after, perm=None, **more):
    if perm is not None:
        removed = {int(perm[v]) for v in removed}
        deg = {int(perm[v]): d for v, d in deg.items()}; deg_after = {int(perm[v]): d for v, d in deg_after.items()}
    return dict(graph=g, mx=mx, F=F, perm=perm, removed=set(removed), chains=chains, long_flanks=long_flanks, bridges=bridges, deg=deg, deg_after=deg_after, **more)


def hand_cases():
    """name -> dict(graph, mx, F, perm, and the claims: removed (a set of reads), deg {read: degree} before, deg_after, chains, long_flanks,
    bridges).  The chord case also has cycle (its reads), for the circular contig."""
    cases = {}
    for mx, F in PARAMS:
        tag = "mx%d_F%d" % (mx, F)
        # an H with four flanks of F reads of degree 2, each ending in a dead end, and a bar of t reads: cut iff t <= mx
        for t in sorted({1, mx, mx + 1}):
            g = tu.Graph()
            a, b, ch, fl = _h(g, t, (F, F, F, F))
            cut = t <= mx
            # a bar of t >= F reads (t = mx + 1 = F) is no chain, and seen from a or b it is a long flank
            cases["h_bar_of_%d_%s_%s" % (t, "cut" if cut else "too_long", tag)] = _case(
                g, mx, F, ch if cut else (), 1 if cut else 0, 4 + (2 if t >= F else 0), 1 if cut else 0, {a: 3, b: 3, ch[0]: 2, fl[0][0]: 2},
                {a: 2 if cut else 3, b: 2 if cut else 3, ch[0]: 0 if cut else 2, fl[0][0]: 2, fl[3][-1]: 2})
        # one of the four flanks, each in turn, with F - 1 reads of degree 2 and then a dead end
        for i in range(4):
            g = tu.Graph()
            a, b, ch, fl = _h(g, 1, tuple(F - 1 if j == i else F for j in range(4)))
            cases["flank_%d_of_Fminus1_reads_then_a_dead_end_%s" % (i, tag)] = _case(g, mx, F, (), 1, 3, 0, {a: 3, b: 3, ch[0]: 2}, {a: 3, b: 3, ch[0]: 2})
        # the same flank ending at another anchor c: after F - 1 reads of degree 2 nothing is cut, after F the bar is.  The reads between a (or
        # b) and c are a chain themselves when there are at most mx of them (F - 1 = mx), never a bridge: c's other flanks have one read
        for i in range(4):
            for n2 in (F - 1, F):
                g = tu.Graph()
                a, b, ch, fl = _h(g, 1, tuple(n2 if j == i else F for j in range(4)), tuple("anchor" if j == i else "dead" for j in range(4)))
                cut = n2 == F
                cases["flank_%d_of_%s_reads_then_an_anchor_%s" % (i, "F" if cut else "Fminus1", tag)] = _case(
                    g, mx, F, ch if cut else (), 1 + (1 if n2 <= mx else 0), 3 + (2 if cut else 0), 1 if cut else 0, {a: 3, b: 3, fl[i][-1]: 2},
                    {a: 2 if cut else 3, b: 2 if cut else 3, ch[0]: 0 if cut else 2})
        # deg(a) == 4 or deg(b) == 4 with everything long: only the columns of degree exactly 3 have flanks
        for which in ("a", "b"):
            g = tu.Graph()
            a, b, ch, fl = _h(g, 1, (F, F, F, F))
            _tail(g, a if which == "a" else b, F)
            cases["deg_%s_is_4_%s" % (which, tag)] = _case(g, mx, F, (), 1, 2, 0, {a: 4 if which == "a" else 3, b: 4 if which == "b" else 3}, {a: 4 if which == "a" else 3, ch[0]: 2})
        # a chain from a back to a, of max(2, mx) reads (a loop needs two reads beside a; at mx = 1 the walk gives up before it is back)
        g = tu.Graph()
        a = g.new()[0]
        fa = _tail(g, a, F)[0]
        t = max(2, mx)
        loop = bu.between(g, a, a, t)
        cases["chain_from_a_back_to_a_%s" % tag] = _case(g, mx, F, (), 0, 1 + (2 if t >= F else 0), 0, {a: 3, loop[0]: 2}, {a: 3, loop[0]: 2})
        # a direct entry a - b beside the chain: seen from a, b is a flank of no reads
        g = tu.Graph()
        a, b, ch, fl = _h(g, 1, (F, None, F, None))
        g.link(a, b)
        cases["direct_entry_beside_the_chain_%s" % tag] = _case(g, mx, F, (), 1, 2, 0, {a: 3, b: 3, ch[0]: 2}, {a: 3, b: 3, ch[0]: 2})
        # two short chains between a and b plus one outer flank each: each chain is the other's short flank
        g = tu.Graph()
        a, b, ch, fl = _h(g, 1, (F, None, F, None))
        ch2 = bu.between(g, a, b, mx)
        cases["two_short_chains_between_a_and_b_%s" % tag] = _case(g, mx, F, (), 2, 2, 0, {a: 3, b: 3, ch[0]: 2, ch2[0]: 2}, {a: 3, b: 3, ch[0]: 2, ch2[-1]: 2})
        # a short chain beside a parallel arm of F reads, with long outer flanks: the arm is a long flank of both anchors, the short chain is cut
        g = tu.Graph()
        a, b, ch, fl = _h(g, mx, (F, None, F, None))
        arm = bu.between(g, a, b, F)
        cases["short_chain_beside_a_parallel_arm_of_F_reads_%s" % tag] = _case(g, mx, F, ch, 1, 4, 1, {a: 3, b: 3, arm[0]: 2}, {a: 2, b: 2, arm[0]: 2, ch[0]: 0})
        # two H's on one path whose anchors are F reads apart (both cut) and F - 1 apart (neither: each is the other's short flank)
        for apart in (F, F - 1):
            g = tu.Graph()
            a1, b1, ch1, fl1 = _h(g, 1, (F, None, F, F))
            a2, b2, ch2, fl2 = _h(g, 1, (F, None, F, F))
            mid = bu.between(g, a1, a2, apart)
            cut = apart == F
            cases["two_Hs_on_one_path_%s_apart_%s" % ("F" if cut else "Fminus1", tag)] = _case(
                g, mx, F, ch1 + ch2 if cut else (), 2 + (1 if apart <= mx else 0), 8 if cut else 6, 2 if cut else 0, {a1: 3, a2: 3, b1: 3, b2: 3, mid[0]: 2},
                {a1: 2 if cut else 3, a2: 2 if cut else 3, b1: 2 if cut else 3, b2: 2 if cut else 3, mid[0]: 2})
        # a cycle of 2 F + 3 reads with one chord chain of mx reads: afterwards one circular contig of all the cycle's reads
        g = tu.Graph()
        a = g.new()[0]
        s1 = g.new(F)
        b = g.new()[0]
        s2 = g.new(F + 1)
        cyc = g.chain([a] + s1 + [b] + s2, closed=True)
        ch = bu.between(g, a, b, mx)
        cases["cycle_with_one_chord_chain_%s" % tag] = _case(g, mx, F, ch, 1, 4, 1, {a: 3, b: 3, s1[0]: 2}, {v: 2 for v in cyc}, cycle=cyc)
        # anchors at reads 0 and M - 1, a bridge read at 0, a random relabelling
        for name in ("a_0_b_last", "a_last_b_0", "bridge_read_0_a_last", "random_relabelling"):
            g = tu.Graph()
            a, b, ch, fl = _h(g, mx, (F, F, F, F))
            Mg = g.n
            if name == "random_relabelling":
                perm = np.random.default_rng(100 * mx + F).permutation(Mg)
            else:
                first, last = {"a_0_b_last": (a, b), "a_last_b_0": (b, a), "bridge_read_0_a_last": (ch[0], a)}[name]
                rest = [v for v in range(Mg) if v not in (first, last)]
                perm = np.zeros(Mg, dtype=np.int64)
                perm[first], perm[last] = 0, Mg - 1
                perm[rest] = np.arange(1, Mg - 1)
            cases["h_%s_%s" % (name, tag)] = _case(g, mx, F, ch, 1, 4, 1, {a: 3, b: 3, ch[0]: 2}, {a: 2, b: 2, ch[-1]: 0}, perm=perm)
        # flanks that are the two ends of one loop through u: the walk counts the loop's reads beside u, from either end.  2 F - 1 of them
        # (a loop of 2 F reads with u): both long; F - 1 (a loop of F reads with u; it needs two reads beside u, so not at F = 2): both short
        for n2 in (2 * F - 1, F - 1):
            if n2 < 2:
                continue
            g = tu.Graph()
            u, b, ch, fl = _h(g, 1, (None, None, F, F))
            loop = bu.between(g, u, u, n2)
            cut = n2 >= F
            cases["flanks_that_are_one_loop_of_%s_reads_with_u_%s" % ("2F" if cut else "F", tag)] = _case(
                g, mx, F, ch if cut else (), 1, 4 if cut else 2, 1 if cut else 0, {u: 3, b: 3, loop[0]: 2}, {u: 2 if cut else 3, b: 2 if cut else 3, loop[0]: 2})
    return cases


def case_overlaps(case, rng, extra_reads=0):
    """(M, rows, cols, vals) of a hand case for elba_set_overlaps; extra_reads isolated reads follow the graph's."""
    g = case["graph"]
    return g.overlaps(rng, perm=case.get("perm"), M=g.n + extra_reads)


def long_paths(rng, n_paths, length):
    """(M, rows, cols, vals): n_paths paths of `length` consecutive reads each, an upper-triangular edge list for elba_set_overlaps with
    suffixes the reduction keeps at fuzz 0."""
    M = n_paths * length
    r = np.arange(M - 1, dtype=np.int64)
    r = r[(r + 1) % length != 0]
    v = np.zeros(len(r), dtype=po.OVERLAP_DTYPE)
    v["passed"] = 1
    v["direction"] = rng.integers(0, 4, len(r)); v["directionT"] = rng.integers(0, 4, len(r))
    v["suffix"] = rng.integers(5, 10, len(r)); v["suffixT"] = rng.integers(5, 10, len(r))
    return M, r, r + 1, v


def plant_bridges(rng, M, rows, cols, vals, n, t, gap=8):
    """Plants n H's into a graph of long paths (every read of degree <= 2, no cycle): a chain of t NEW reads (ids from M on) between two
    inner reads of the paths, drawn at random among the reads that lie a multiple of gap + 1 steps, and at least gap + 1, from the smaller end
    of their path and more than gap from the other.  Any two anchors are then gap reads apart or more, so with min_flank_reads <= gap and
    t <= max_bridge_reads exactly the planted reads are bridges.  Returns (M', rows, cols, vals, planted reads, [(u, v)]), (row, col) order."""
    rows = np.asarray(rows, dtype=np.int64); cols = np.asarray(cols, dtype=np.int64)
    nb = [[] for _ in range(M)]
    for r, c in zip(rows.tolist(), cols.tolist()):
        nb[r].append(c); nb[c].append(r)
    assert max(len(x) for x in nb) <= 2
    slots, seen = [], np.zeros(M, dtype=bool)
    for s in range(M):
        if len(nb[s]) != 1 or seen[s]:
            continue
        path, prev, cur = [s], -1, s
        while True:
            nxt = [x for x in nb[cur] if x != prev]
            if not nxt:
                break
            prev, cur = cur, nxt[0]
            path.append(cur)
        seen[path] = True
        slots += [path[i] for i in range(gap + 1, len(path) - gap - 1, gap + 1)]
    assert len(slots) >= 2 * n, (len(slots), n)
    pick = rng.choice(np.array(slots, dtype=np.int64), size=2 * n, replace=False)
    pairs = [(int(u), int(v)) for u, v in pick.reshape(n, 2)]
    M2, r2, c2, v2, planted = bu.plant_bubbles(rng, M, rows, cols, vals, [(min(p), max(p)) for p in pairs], [t] * n)
    return M2, r2, c2, v2, planted, pairs
