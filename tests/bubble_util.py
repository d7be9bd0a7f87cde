"""Bubble popping (elba_pop_bubbles, elba_amd/csrc/bubbles.hip) restated in plain Python, twice, and the hand-made graphs both test files use.

pop_bubbles          the rule of include/elba_amd.h statement by statement: one round at a time, from every entry of an anchor's column along
                     the tips walk.  Input: (M, rows, cols, vals) of S in export order (columns ascending, rows ascending within a column).
                     Returns the popped S, the flags (bit 3 of every removed read) and every field of the stats except the times.
pop_bubbles_chains   a second implementation that shares nothing with the first and runs on the CPU only: per round it freezes the degrees,
                     finds the maximal chains of degree-2 reads as the components of the degree-2 subgraph (union-find, no walk), classifies
                     each by the two reads it ends at, groups the chains by (a, b) and deletes the losing arms one at a time from a working
                     set of entries, in the order the caller's permutation gives.  It needs a symmetric S.  That both agree whatever the
                     order pins the claim that order does not matter.
hand_cases           graphs named after the clause of the rule they show, with what each claims (degrees, arms found, bubbles, reads
                     removed, rounds run, degrees after), so that a case that does not show what its name says fails in test_bubbles_cpu.py.
simplify             clip_tips(.., 64) then pop_bubbles(.., 64) of the restatements until a pass of both removes nothing: what
                     Engine.simplify_graph is held against."""
import numpy as np

import tip_util as tu

STATS = ("nreads", "nnz_before", "nnz_after", "anchors", "arms", "bubbles", "arms_removed", "reads_removed", "entries_removed", "rounds_run")


def _stats(M, n):
    return dict(nreads=M, nnz_before=n, nnz_after=n, anchors=0, arms=0, bubbles=0, arms_removed=0, reads_removed=0, entries_removed=0, rounds_run=0)


def pop_bubbles(M, rows, cols, vals, max_arm_reads, rounds=1, trace=None):
    """Returns (rows, cols, vals, flags, stats).  trace, a list, receives per round (arms = [(a, b, reads)], removed arms = [(a, b, reads)])."""
    rows = [int(r) for r in rows]; cols = [int(c) for c in cols]
    live = list(range(len(rows)))                               # entries of S still there, in export order
    flags = np.zeros(M, dtype=np.uint8)
    st = _stats(M, len(rows))
    for rnd in range(rounds):
        # the degrees as the round finds them: a read's degree is the length of its column
        column = {}
        for z in live:
            column.setdefault(cols[z], []).append(rows[z])
        deg = {v: len(column.get(v, ())) for v in range(M)}
        # anchors
        anchors = [v for v in range(M) if deg[v] >= 3]
        if rnd == 0:
            st["anchors"] = len(anchors)
        # arms: every entry of an anchor's column whose row has degree 2 starts the tips walk, "came from" = the anchor
        arms = []
        for a in anchors:
            for v1 in column[a]:                                # ascending: the entries of column a in their order
                if deg[v1] != 2:
                    continue
                chain, prev, cur = [], a, v1
                while True:
                    if deg[cur] >= 3:                           # b
                        if cur > a:                             # recorded at the smaller anchor; b == a is no arm.  chain has >= 1 read: v1
                            arms.append((a, cur, tuple(chain)))
                        break
                    if deg[cur] != 2:                           # a read of degree 0 or 1
                        break
                    if len(chain) == max_arm_reads:             # cur would be read max_arm_reads + 1
                        break
                    x, y = column[cur]
                    nxt = x if x != prev else y                 # not the read it came from; the smaller, should neither be
                    chain.append(cur)
                    prev, cur = cur, nxt
        st["arms"] += len(arms)
        # bubbles: all arms with the same (a, b), two or more
        groups = {}
        for arm in arms:
            groups.setdefault(arm[:2], []).append(arm)
        gone = []
        for key in sorted(groups):
            g = groups[key]
            if len(g) < 2:
                continue
            st["bubbles"] += 1
            kept = max(g, key=lambda arm: (len(arm[2]), -arm[2][0]))      # the most reads; on a tie the smallest first read
            gone += [arm for arm in g if arm is not kept]
        st["arms_removed"] += len(gone)
        removed = set()
        for _, _, chain in gone:
            removed |= set(chain)
        if trace is not None:
            trace.append((arms, gone))
        st["rounds_run"] = rnd + 1
        if not removed:
            break
        # removal
        st["reads_removed"] += len(removed)
        for v in removed:
            flags[v] |= 8
        live = [z for z in live if rows[z] not in removed and cols[z] not in removed]
    st["nnz_after"] = len(live)
    st["entries_removed"] = st["nnz_before"] - len(live)
    idx = np.array(live, dtype=np.int64)
    return np.asarray(rows, dtype=np.int64)[idx], np.asarray(cols, dtype=np.int64)[idx], np.asarray(vals)[idx], flags, st


def _root(parent, x):
    while parent[x] != x:
        parent[x] = parent[parent[x]]
        x = parent[x]
    return x


def pop_bubbles_chains(M, rows, cols, vals, max_arm_reads, rounds=1, order=None):
    """The same result from the chains of the degree-2 subgraph, losing arms deleted one at a time.  order: a permutation of the reads; the
    losing arms of a round are deleted in the order it gives their first reads (default: descending)."""
    rows = np.asarray(rows, dtype=np.int64); cols = np.asarray(cols, dtype=np.int64)
    assert set(zip(rows.tolist(), cols.tolist())) == set(zip(cols.tolist(), rows.tolist())), "pop_bubbles_chains needs both triangles"
    rank = np.zeros(M, dtype=np.int64)
    rank[list(range(M - 1, -1, -1)) if order is None else [int(v) for v in order]] = np.arange(M)
    present = np.ones(len(rows), dtype=bool)
    flags = np.zeros(M, dtype=np.uint8)
    st = _stats(M, len(rows))
    for rnd in range(rounds):
        frozen = np.bincount(cols[present], minlength=M)        # the frozen degree table of the round
        if rnd == 0:
            st["anchors"] = int((frozen >= 3).sum())
        r, c = rows[present], cols[present]
        # maximal chains of degree-2 reads: components of the subgraph S induces on them
        parent = list(range(M))
        both = (frozen[r] == 2) & (frozen[c] == 2)
        for u, v in zip(r[both].tolist(), c[both].tolist()):
            ru, rv = _root(parent, u), _root(parent, v)
            if ru != rv:
                parent[ru] = rv
        members, ends = {}, {}                                  # ends: (read of the chain, the read outside the chain it touches)
        for v in np.flatnonzero(frozen == 2).tolist():
            members.setdefault(_root(parent, v), []).append(v)
        out = (frozen[c] == 2) & (frozen[r] != 2)
        for u, v in zip(r[out].tolist(), c[out].tolist()):
            ends.setdefault(_root(parent, v), []).append((v, u))
        # classify by the two ends; group the arms by (a, b)
        groups = {}
        for root, reads in members.items():
            e = ends.get(root, [])
            if len(e) != 2:                                     # a cycle of degree-2 reads
                assert len(e) == 0
                continue
            (v_a, a), (v_b, b) = sorted(e, key=lambda t: t[1])
            if frozen[a] < 3 or frozen[b] < 3 or a == b or len(reads) > max_arm_reads:
                continue                                        # a dead end, a chain back to its anchor, a chain too long
            groups.setdefault((a, b), []).append((len(reads), v_a, reads))       # v_a: the arm's read in the smaller anchor's column
            st["arms"] += 1
        losers = []
        for g in groups.values():
            if len(g) < 2:
                continue
            st["bubbles"] += 1
            best = max(n for n, _, _ in g)
            keep = min(first for n, first, _ in g if n == best)
            losers += [(first, reads) for _, first, reads in g if first != keep]
        st["arms_removed"] += len(losers)
        st["rounds_run"] = rnd + 1
        if not losers:
            break
        for first, reads in sorted(losers, key=lambda t: rank[t[0]]):    # one arm at a time
            present &= ~(np.isin(rows, reads) | np.isin(cols, reads))
            flags[reads] |= 8
            st["reads_removed"] += len(reads)
    st["nnz_after"] = int(present.sum())
    st["entries_removed"] = st["nnz_before"] - st["nnz_after"]
    return rows[present], cols[present], np.asarray(vals)[present], flags, st


def simplify(M, rows, cols, vals, max_tip_reads, max_arm_reads, passes=16):
    """The restatements alternated as Engine.simplify_graph alternates the calls.  Returns (rows, cols, vals, flags, [(tip stats, bubble stats)])."""
    flags = np.zeros(M, dtype=np.uint8)
    out = []
    for _ in range(passes):
        rows, cols, vals, f1, s1 = tu.clip_tips(M, rows, cols, vals, max_tip_reads, 64)
        rows, cols, vals, f2, s2 = pop_bubbles(M, rows, cols, vals, max_arm_reads, 64)
        flags |= f1 | f2
        out.append((s1, s2))
        if s1["reads_removed"] == 0 and s2["reads_removed"] == 0:
            break
    return rows, cols, vals, flags, out


def between(g, a, b, n):
    """A chain of n new reads from a to b (n = 0: the direct edge); returns them, a's neighbour first."""
    ids = g.new(n)
    g.chain([a] + ids + [b])
    return ids


def _bubble(g, arms, a=None, tails=(5, 5), direct=False):
    """a and b joined by one chain per element of arms (the earlier the arm, the smaller its reads; all between a and b in id), each with a
    dead-end tail of tails[.] reads (0: none).  Returns (a, b, chains)."""
    if a is None:
        a = g.new()[0]
        if tails[0]:
            g.arm(a, tails[0])
    chains = [g.new(n) for n in arms]
    b = g.new()[0]
    for ch in chains:
        g.chain([a] + ch + [b])
    if direct:
        g.link(a, b)
    if tails[1]:
        g.arm(b, tails[1])
    return a, b, chains


def _flat(chains):
    return {v for ch in chains for v in ch}


def hand_cases():
    """name -> dict(graph, max, rounds, perm, and the claims: deg {read: degree}, arm_lengths (first round, sorted), bubbles (first
    round), removed (all rounds, a set), rounds_run, deg_after {read: degree}; the two alternation cases also max_tip and removed_simplify)."""
    cases = {}
    g = tu.Graph()
    a, b, ch = _bubble(g, [1, 2])
    cases["arms_1_2"] = dict(graph=g, max=3, rounds=2, deg={a: 3, b: 3}, arm_lengths=[1, 2], bubbles=1, removed=set(ch[0]), rounds_run=2, deg_after={a: 2, b: 2})
    g = tu.Graph()
    a, b, ch = _bubble(g, [2, 2])
    assert ch[0][0] < ch[1][0]
    cases["arms_2_2_tie_smaller_first_read_kept"] = dict(graph=g, max=2, rounds=1, deg={a: 3, b: 3}, arm_lengths=[2, 2], bubbles=1, removed=set(ch[1]), rounds_run=1,
                                                         deg_after={a: 2, b: 2, ch[0][0]: 2, ch[1][0]: 0})
    for mx in (2, 7):
        g = tu.Graph()
        a, b, ch = _bubble(g, [1, mx, mx + 1])
        cases["arms_1_max_maxplus1_max%d" % mx] = dict(graph=g, max=mx, rounds=2, deg={a: 4, b: 4}, arm_lengths=[1, mx], bubbles=1, removed=set(ch[0]), rounds_run=2,
                                                       deg_after={a: 3, b: 3, ch[2][0]: 2})
    g = tu.Graph()
    a, b, ch = _bubble(g, [1, 2, 3])
    cases["three_arms_1_2_3"] = dict(graph=g, max=3, rounds=1, deg={a: 4, b: 4}, arm_lengths=[1, 2, 3], bubbles=1, removed=_flat(ch[:2]), rounds_run=1, deg_after={a: 2, b: 2})
    g = tu.Graph()
    a, b, ch = _bubble(g, [2], direct=True)
    cases["direct_edge_and_one_arm"] = dict(graph=g, max=3, rounds=2, deg={a: 3, b: 3}, arm_lengths=[2], bubbles=0, removed=set(), rounds_run=1, deg_after={a: 3, b: 3})
    g = tu.Graph()
    a, b, ch = _bubble(g, [1, 2], direct=True)
    cases["direct_edge_and_two_arms"] = dict(graph=g, max=3, rounds=2, deg={a: 4, b: 4}, arm_lengths=[1, 2], bubbles=1, removed=set(ch[0]), rounds_run=2, deg_after={a: 3, b: 3})
    g = tu.Graph()
    a = g.new()[0]
    g.arm(a, 5)
    loop = between(g, a, a, 3)
    cases["chain_from_a_back_to_a"] = dict(graph=g, max=7, rounds=2, deg={a: 3, loop[1]: 2}, arm_lengths=[], bubbles=0, removed=set(), rounds_run=1, deg_after={a: 3})
    g, a, arms = tu._y([1, 5, 6])
    cases["chain_from_a_to_a_dead_end"] = dict(graph=g, max=7, rounds=2, deg={a: 3, arms[0][0]: 1}, arm_lengths=[], bubbles=0, removed=set(), rounds_run=1, deg_after={a: 3})
    g = tu.Graph()
    a, b, ch = _bubble(g, [1, 2, 3], tails=(0, 0))
    cases["theta_ends_as_a_path"] = dict(graph=g, max=3, rounds=64, deg={a: 3, b: 3}, arm_lengths=[1, 2, 3], bubbles=1, removed=_flat(ch[:2]), rounds_run=2,
                                         deg_after={a: 1, b: 1, ch[2][0]: 2, ch[2][1]: 2, ch[2][2]: 2})
    g = tu.Graph()
    a, b1, ch1 = _bubble(g, [1, 2])
    _, b2, ch2 = _bubble(g, [2, 1], a=a)
    cases["two_bubbles_sharing_their_smaller_anchor"] = dict(graph=g, max=2, rounds=1, deg={a: 5, b1: 3, b2: 3}, arm_lengths=[1, 1, 2, 2], bubbles=2,
                                                             removed=set(ch1[0]) | set(ch2[1]), rounds_run=1, deg_after={a: 3, b1: 2, b2: 2})
    g = tu.Graph()
    a, m, ch1 = _bubble(g, [1, 2], tails=(5, 0))
    _, c, ch2 = _bubble(g, [2, 1], a=m)
    assert a < m < c
    cases["two_bubbles_in_series"] = dict(graph=g, max=2, rounds=1, deg={a: 3, m: 4, c: 3}, arm_lengths=[1, 1, 2, 2], bubbles=2, removed=set(ch1[0]) | set(ch2[1]),
                                          rounds_run=1, deg_after={a: 2, m: 2, c: 2})
    for rounds, run in ((1, 1), (2, 2), (64, 3)):
        # A - p - a =(x | y1 y2)= b - q - B beside A - r - B: the inner bubble first; one round later the outer one, arms of 6 reads and 1
        g = tu.Graph()
        A = g.new()[0]
        g.arm(A, 5)
        p, a = g.new(2)
        x = g.new(1); y = g.new(2)
        b, q, r, B = g.new(4)
        g.chain([A, p, a]); g.chain([a] + x + [b]); g.chain([a] + y + [b]); g.chain([b, q, B]); g.chain([A, r, B])
        g.arm(B, 5)
        cases["nested_bubble_rounds%d" % rounds] = dict(graph=g, max=6, rounds=rounds, deg={A: 3, B: 3, a: 3, b: 3}, arm_lengths=[1, 1, 1, 1, 2], bubbles=1,
                                                        removed=set(x) if rounds == 1 else set(x) | {r}, rounds_run=run,
                                                        deg_after={A: 3 if rounds == 1 else 2, B: 3 if rounds == 1 else 2, a: 2, b: 2})
    # the two alternation cases: what each call alone does, and what Engine.simplify_graph(max_tip, max, ..) does
    g = tu.Graph()
    a, b, ch = _bubble(g, [1, 2])
    t = g.arm(ch[0][0], 1)
    cases["tip_on_an_arm"] = dict(graph=g, max=3, max_tip=1, rounds=64, deg={a: 3, b: 3, ch[0][0]: 3, t[0]: 1}, arm_lengths=[2], bubbles=0, removed=set(), rounds_run=1,
                                  deg_after={a: 3, b: 3}, removed_simplify={t[0]: 4, ch[0][0]: 8})
    g = tu.Graph()
    main = g.chain(g.new(12))
    p = g.arm(main[6], 1)
    a, b, ch = _bubble(g, [1, 2], a=p[0], tails=(0, 4))
    cases["bubble_inside_a_dead_end_chain"] = dict(graph=g, max=3, max_tip=3, rounds=64, deg={main[6]: 3, a: 3, b: 3}, arm_lengths=[1, 2], bubbles=1, removed=set(ch[0]),
                                                   rounds_run=2, deg_after={main[6]: 3, a: 2, b: 2}, removed_simplify={ch[0][0]: 8})
    for name, a_is in (("anchors_0_and_last", 0), ("anchors_last_and_0", 1)):
        g = tu.Graph()
        a, b, ch = _bubble(g, [2, 2])
        M = g.n
        rest = [v for v in range(M) if v not in (a, b)]
        perm = np.zeros(M, dtype=np.int64)
        perm[a], perm[b] = (0, M - 1) if a_is == 0 else (M - 1, 0)
        perm[rest] = np.arange(1, M - 1)
        # the arms are recorded at read 0; their first reads are its neighbours: ch[.][0] if that is a, ch[.][-1] if it is b
        first = [int(perm[c[0] if a_is == 0 else c[-1]]) for c in ch]
        lose = ch[int(np.argmax(first))]
        cases[name] = dict(graph=g, max=2, rounds=1, perm=perm, deg={0: 3, M - 1: 3}, arm_lengths=[2, 2], bubbles=1, removed={int(perm[v]) for v in lose}, rounds_run=1,
                           deg_after={0: 2, M - 1: 2})
    return cases


def plant_bubbles(rng, M, rows, cols, vals, pairs, lengths):
    """Adds a chain of lengths[i] NEW reads (ids from M on) between the two reads of pairs[i].  Returns (M', rows, cols, vals, planted
    reads), (row, col) order."""
    xr, xc, planted, nxt = [], [], [], int(M)
    for (u, v), n in zip(pairs, lengths):
        prev = int(u)
        for _ in range(int(n)):
            xr.append(prev); xc.append(nxt)                     # prev < nxt: new ids are the largest
            planted.append(nxt)
            prev, nxt = nxt, nxt + 1
        xr.append(int(v)); xc.append(prev)
    xv = np.zeros(len(xr), dtype=np.asarray(vals).dtype)
    xv["passed"] = 1
    xv["direction"] = rng.integers(0, 4, len(xr)); xv["directionT"] = rng.integers(0, 4, len(xr))
    xv["suffix"] = rng.integers(5, 10, len(xr)); xv["suffixT"] = rng.integers(5, 10, len(xr))
    r = np.concatenate([np.asarray(rows, dtype=np.int64), np.array(xr, dtype=np.int64)])
    c = np.concatenate([np.asarray(cols, dtype=np.int64), np.array(xc, dtype=np.int64)])
    v = np.concatenate([np.asarray(vals), xv])
    assert (r < c).all()
    order = np.lexsort((c, r))
    return nxt, r[order], c[order], v[order], np.array(planted, dtype=np.int64)
