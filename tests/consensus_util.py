"""Contig polishing (elba_polish_contigs; the rule is stated in include/elba_amd.h) restated twice in Python, hand cases with their claims and
a mutator that plants errors into the ground-truth layouts of placement_util.truth_set.  The two restatements share nothing with
elba_amd/csrc/polish.hip nor with each other: polish_loops keeps every cell of the band in a dict and writes every slice, existence test and
tie out; polish_tables computes one row of the band at a time with numpy, the left dependency through the prefix-minimum identity
H[b] = b + min over e <= b of (cand[e] - e), and calls the columns with key arrays.

Both take the same `cin` dict (inputs_of): seqs (the reads, forward), contigs (strings), kinds, reads (the placement records,
placement_util.PLACEMENT), band, max_diff_q16, min_depth, and return (out, stats): out as Engine.polish_contigs(votes=True) returns it
without its times, stats without `batches` and the times."""
import itertools
import math

import numpy as np

import contig_ex_util as cx
import contig_util as cu
import placement_util as pu

POLISH_READ = np.dtype([("dist", "<i4"), ("n", "<i4"), ("end_j", "<i4"), ("status", "<i4")])
NOT_PLACED, OUTSIDE, REJECTED, VOTED = 0, 1, 2, 3
STATS = ("nreads", "voted", "rejected", "outside", "low_depth_columns", "bases_before", "bases_after", "sum_dist", "cells")
GET_STATS = ("voted", "rejected", "outside", "low_depth_columns", "bases_before", "bases_after", "sum_dist", "cells", "batches")
CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
INF = 1 << 28


def inputs_of(seqs, contigs, kinds, reads, band=64, max_diff=0.25, min_depth=3):
    return dict(seqs=list(seqs), contigs=list(contigs), kinds=[int(k) for k in kinds], reads=np.asarray(reads), band=int(band), max_diff_q16=int(round(max_diff * 65536)),
                min_depth=int(min_depth))


def _pack(cin, seqs, cols, gaps, recs, counts, st):
    nc = len(cin["contigs"])
    reads = np.zeros(len(recs), dtype=POLISH_READ)
    for r, t in enumerate(recs):
        reads[r] = t
    L = [len(s) for s in cin["contigs"]]
    st = dict(st)
    st["nreads"] = len(recs); st["bases_before"] = sum(L); st["bases_after"] = sum(len(s) for s in seqs)
    return dict(seqs=list(seqs), col_off=np.concatenate([[0], np.cumsum(L)]).astype(np.int64),
                col=np.concatenate([np.asarray(c, dtype=np.uint32).reshape(-1, 5) for c in cols] + [np.zeros((0, 5), np.uint32)]),
                gap=np.concatenate([np.asarray(g, dtype=np.uint32).reshape(-1, 4) for g in gaps] + [np.zeros((0, 4), np.uint32)]),
                reads=reads, **{k: np.array([c[k] for c in counts], dtype=np.int64).reshape(nc) for k in ("voters", "substituted", "deleted", "inserted")}), st


# ---- restatement 1: loops over dict-held cells -------------------------------------------------------------------------------------
def polish_loops(cin, read_order=None):
    W, nc = cin["band"], len(cin["contigs"])
    col = [[[0] * 5 for _ in s] for s in cin["contigs"]]
    gap = [[[0] * 4 for _ in range(len(s) + 1)] for s in cin["contigs"]]
    counts = [dict(voters=0, substituted=0, deleted=0, inserted=0) for _ in range(nc)]
    st = dict.fromkeys(STATS, 0)
    M = len(cin["seqs"])
    recs = [None] * M
    for r in (range(M) if read_order is None else read_order):
        r = int(r)
        p = cin["reads"][r]
        if int(p["kind"]) == pu.NONE:
            recs[r] = (0, 0, 0, NOT_PLACED)
            continue
        if int(p["flags"]) & pu.OUTSIDE:
            recs[r] = (0, 0, 0, OUTSIDE); st["outside"] += 1
            continue
        k, start = int(p["contig"]), int(p["start"])
        s, circ = cin["contigs"][k], cin["kinds"][k] == cx.CIRCLE
        L = len(s)
        rd = cu.revcomp(cin["seqs"][r]) if int(p["strand"]) else cin["seqs"][r]
        l = len(rd)
        if circ:
            i0, i1 = 0, min(l, L)
        else:
            i0, i1 = max(0, -start), min(l, L - start)
        n, stc, q = i1 - i0, start + i0, rd[i0:i1]
        assert n >= 1

        def exists(i, j):
            if not (0 <= i <= n and 0 <= j - i - stc + W // 2 < W):
                return False
            return circ or 0 <= j <= L

        D, choice = {}, {}
        for j in range(stc - W // 2, stc + W // 2):
            if exists(0, j):
                D[(0, j)] = 0
        for i in range(1, n + 1):
            for j in range(i + stc - W // 2, i + stc + W // 2):           # ascending j: the left neighbour is there when this cell is computed
                if not exists(i, j):
                    continue
                terms = []
                if (i - 1, j - 1) in D:
                    terms.append(D[(i - 1, j - 1)] + (0 if q[i - 1] == s[(j - 1) % L] else 1))
                else:
                    terms.append(math.inf)
                terms.append(D[(i - 1, j)] + 1 if (i - 1, j) in D else math.inf)
                terms.append(D[(i, j - 1)] + 1 if (i, j - 1) in D else math.inf)
                d = min(terms)
                if d == math.inf:
                    continue                                             # a cell nothing reaches: infinite, never on a path
                D[(i, j)] = d
                choice[(i, j)] = terms.index(d)                          # the first of diagonal, up, left
        ends = [(D[(n, j)], j) for j in range(n + stc - W // 2, n + stc + W // 2) if (n, j) in D]
        dist, end_j = min(ends)
        st["cells"] += n * W
        if dist > (cin["max_diff_q16"] * n) >> 16:
            recs[r] = (dist, n, end_j, REJECTED); st["rejected"] += 1
            continue
        recs[r] = (dist, n, end_j, VOTED); st["voted"] += 1; st["sum_dist"] += dist; counts[k]["voters"] += 1
        i, j = n, end_j
        while i > 0:
            ch = choice[(i, j)]
            if ch == 0:
                col[k][(j - 1) % L if circ else j - 1][CODE[q[i - 1]]] += 1
                i, j = i - 1, j - 1
            elif ch == 2:
                col[k][(j - 1) % L if circ else j - 1][4] += 1
                j -= 1
            else:
                while i - 1 > 0 and choice[(i - 1, j)] == 1:             # to the last step of the run, the first base in read order
                    i -= 1
                gap[k][j % L if circ else j][CODE[q[i - 1]]] += 1
                i -= 1
    seqs = []
    for k in range(nc):
        s, circ = cin["contigs"][k], cin["kinds"][k] == cx.CIRCLE
        L = len(s)
        depth = [sum(c) for c in col[k]]
        out = []

        def gap_base(g):
            if g == L:
                span = depth[L - 1]
            elif g == 0:
                span = min(depth[L - 1], depth[0]) if circ else depth[0]
            else:
                span = min(depth[g - 1], depth[g])
            if 2 * sum(gap[k][g]) > span:
                counts[k]["inserted"] += 1
                return "ACGT"[max(range(4), key=lambda b: (gap[k][g][b], -b))]
            return ""

        for c in range(L):
            out.append(gap_base(c))
            if depth[c] < cin["min_depth"]:
                st["low_depth_columns"] += 1
                out.append(s[c])
                continue
            own = CODE[s[c]]
            order = [own] + [b for b in range(4) if b != own] + [4]     # the contig's own base, then A, C, G, T, then the deletion
            best = order[0]
            for b in order[1:]:
                if col[k][c][b] > col[k][c][best]:
                    best = b
            if best == 4:
                counts[k]["deleted"] += 1
            else:
                out.append("ACGT"[best])
                counts[k]["substituted"] += best != own
        if L and not circ:
            out.append(gap_base(L))
        seqs.append("".join(out))
    return _pack(cin, seqs, col, gap, recs, counts, st)


# ---- restatement 2: numpy, one row of the band at a time ---------------------------------------------------------------------------
def _codes(s):
    return np.frombuffer(s.encode("ascii"), dtype=np.uint8).copy() if False else np.array([CODE[x] for x in s], dtype=np.int64)


def polish_tables(cin, walks=None):
    """walks: a dict that takes every voter's walked steps, {read: [(choice, row, column, band cell)]} from the end cell back to row 1
    (choice 0 diagonal, 1 up, 2 left; the step enters cell (row, column) from its predecessor)."""
    W, nc = cin["band"], len(cin["contigs"])
    sc = [_codes(s) for s in cin["contigs"]]
    col = [np.zeros((len(s), 5), dtype=np.int64) for s in cin["contigs"]]
    gap = [np.zeros((len(s) + 1, 4), dtype=np.int64) for s in cin["contigs"]]
    voters = np.zeros(nc, dtype=np.int64)
    st = dict.fromkeys(STATS, 0)
    M = len(cin["seqs"])
    recs = [(0, 0, 0, NOT_PLACED)] * M
    band = np.arange(W, dtype=np.int64)
    for r in range(M):
        p = cin["reads"][r]
        if int(p["kind"]) == pu.NONE:
            continue
        if int(p["flags"]) & pu.OUTSIDE:
            recs[r] = (0, 0, 0, OUTSIDE); st["outside"] += 1
            continue
        k, start = int(p["contig"]), int(p["start"])
        circ, L = cin["kinds"][k] == cx.CIRCLE, len(cin["contigs"][k])
        rd = _codes(cin["seqs"][r])
        if int(p["strand"]):
            rd = 3 - rd[::-1]
        l = len(rd)
        i0, i1 = (0, min(l, L)) if circ else (max(0, -start), min(l, L - start))
        n, q = i1 - i0, rd[i0:i1]
        base0 = start + i0 - W // 2                                      # column of band cell b in row i: base0 + i + b
        j0 = base0 + band
        prev = np.where(np.ones(W, bool) if circ else (j0 >= 0) & (j0 <= L), 0, INF)
        choices = np.zeros((n + 1, W), dtype=np.int8)
        for i in range(1, n + 1):
            j = base0 + i + band
            pos = j - 1
            sb = sc[k][np.mod(pos, L)] if circ else np.where((pos >= 0) & (pos < L), sc[k][np.clip(pos, 0, L - 1)], 4)
            dg = prev + (sb != q[i - 1])
            up = np.concatenate([prev[1:], [INF]]) + 1
            cand = np.minimum(dg, up)
            h = band + np.minimum.accumulate(cand - band)
            ok = np.ones(W, bool) if circ else (j >= 0) & (j <= L)
            h = np.where(ok & (h < INF // 2), h, INF)
            choices[i] = np.where(dg == h, 0, np.where(up == h, 1, 2))
            prev = h
        bend = int(np.argmin(prev))                                      # the first of the smallest: the smallest j
        dist, end_j = int(prev[bend]), base0 + n + bend
        st["cells"] += n * W
        if dist > (cin["max_diff_q16"] * n) >> 16:
            recs[r] = (dist, n, end_j, REJECTED); st["rejected"] += 1
            continue
        recs[r] = (dist, n, end_j, VOTED); st["voted"] += 1; st["sum_dist"] += dist; voters[k] += 1
        steps = []                                                       # (choice, i, j) from the end back to row 0
        i, j = n, end_j
        while i > 0:
            ch = int(choices[i][j - i - base0])
            steps.append((ch, i, j))
            i, j = (i - 1, j - 1) if ch == 0 else ((i - 1, j) if ch == 1 else (i, j - 1))
        if walks is not None:
            walks[r] = [(ch, i, j, j - i - base0) for ch, i, j in steps]
        wrap = (lambda x: x % L) if circ else (lambda x: x)
        for (ch, j), run in itertools.groupby(steps, key=lambda t: (t[0], t[2] if t[0] == 1 else None)):
            run = list(run)
            if ch == 1:
                gap[k][wrap(j), q[run[-1][1] - 1]] += 1
            else:
                for _, i, jj in run:
                    col[k][wrap(jj - 1), q[i - 1] if ch == 0 else 4] += 1
    seqs, counts = [], []
    for k in range(nc):
        s, circ, L = sc[k], cin["kinds"][k] == cx.CIRCLE, len(sc[k])
        if L == 0:
            seqs.append(""); counts.append(dict(voters=int(voters[k]), substituted=0, deleted=0, inserted=0))
            continue
        depth = col[k].sum(axis=1)
        low = depth < cin["min_depth"]
        pri = np.tile(np.array([5, 4, 3, 2, 1]), (L, 1))
        pri[np.arange(L), s] = 6
        win = np.argmax(col[k] * 8 + pri, axis=1)
        win = np.where(low, s, win)
        left = np.concatenate([[depth[-1] if circ else depth[0]], depth[:-1]])
        span = np.concatenate([np.minimum(left, depth), [depth[-1]]])
        gs = gap[k].sum(axis=1)
        ins = 2 * gs > span
        if circ:
            ins[L] = False
        gb = np.argmax(gap[k], axis=1)
        out = np.full((L + 1, 2), -1, dtype=np.int64)
        out[ins, 0] = gb[ins]
        out[:L, 1] = np.where(win == 4, -1, win)
        flat = out.reshape(-1)
        seqs.append("".join("ACGT"[x] for x in flat[flat >= 0]))
        counts.append(dict(voters=int(voters[k]), substituted=int(((win != s) & (win != 4)).sum()), deleted=int((win == 4).sum()), inserted=int(ins.sum())))
        st["low_depth_columns"] += int(low.sum())
    return _pack(cin, seqs, col, gap, recs, counts, st)


KEYS = ("seqs", "voters", "substituted", "deleted", "inserted", "col_off", "col", "gap", "reads")


def walked_steps(cin):
    """{read: [(choice, row, column, band cell)]} of every voter, from its end cell back to row 1, by polish_tables."""
    walks = {}
    polish_tables(cin, walks)
    return walks


def runs_of(steps, choice):
    """The maximal runs of consecutive steps of one choice in a walk, in read order: [(first row, last row, first column, last column,
    first band cell, last band cell)]."""
    out = []
    for ch, run in itertools.groupby(reversed(steps), key=lambda t: t[0]):
        run = list(run)
        if ch == choice:
            out.append((run[0][1], run[-1][1], run[0][2], run[-1][2], run[0][3], run[-1][3]))
    return out


def first_difference(a, b):
    """For assertion messages: the first field and index at which two polish outputs differ; None when they are the same."""
    for k in KEYS:
        if k == "seqs":
            if list(a[k]) != list(b[k]):
                i = next((i for i, (x, y) in enumerate(zip(a[k], b[k])) if x != y), min(len(a[k]), len(b[k])))
                return "seqs[%d]: %r against %r" % (i, a[k][i:i + 1], b[k][i:i + 1])
            continue
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.shape != y.shape:
            return "%s: shape %r against %r" % (k, x.shape, y.shape)
        ne = np.argwhere(x != y)
        if len(ne):
            i = tuple(ne[0])
            return "%s%r: %r against %r" % (k, i, x[i], y[i])
    return None


# ---- hand cases --------------------------------------------------------------------------------------------------------------------
def _genome(seed, n):
    """n bases without two equal neighbours: an alignment against it has no run to slide a gap along."""
    rng = np.random.default_rng(seed)
    out = [int(rng.integers(0, 4))]
    while len(out) < n:
        out.append(int((out[-1] + rng.integers(1, 4)) % 4))
    return "".join("ACGT"[x] for x in out)


def _other(ch, skip=""):
    return next(x for x in "ACGT" if x != ch and x not in skip)


def _case(name, kind, chain, others, band=64, max_diff=0.25, min_depth=1, reads=None, seq=None, col=None, gap=None, stats=None, counts=None):
    """chain: [(sequence as stored, prefix, strand)] — the contig is the concatenation of the oriented prefixes; others: [(sequence as
    stored, start, strand)], placed through the chain read that holds their first credited base.  Reads are numbered chain first.  Claims:
    reads {read: (dist, n, end_j, status)}, seq (the polished contig), col {(column, code): count}, gap {(gap, code): count}, stats,
    counts {name: value} of the one contig."""
    contig = "".join(pu.oriented(s, st)[:p] for s, p, st in chain)
    seqs = [s for s, _, _ in chain] + [s for s, _, _ in others]
    recs = np.zeros(len(seqs), dtype=pu.PLACEMENT)
    at, L = 0, len(contig)
    for r, (s, p, st) in enumerate(chain):
        fl = pu.CLIPPED if (kind != cx.CIRCLE and at + len(s) > L) or (kind == cx.CIRCLE and len(s) > L) else 0
        if kind == cx.CIRCLE and at % L + min(len(s), L) > L:
            fl |= pu.WRAPPED
        recs[r] = (at, 0, r, 0, st, pu.CHAIN, fl, 0)
        at += p
    for x, (s, start, st) in enumerate(others):
        l = len(s)
        if kind == cx.CIRCLE:
            fl = (pu.CLIPPED if l > L else 0) | (pu.WRAPPED if start % L + min(l, L) > L else 0)
        else:
            lo, hi = max(start, 0), min(start + l, L)
            fl = (pu.CLIPPED if (lo, hi) != (start, start + l) else 0) | (pu.OUTSIDE if hi <= lo else 0)
        recs[len(chain) + x] = (start, 0, 0, l, st, pu.ANCHORED, fl, 0)
    return dict(name=name, kind=kind, chain=chain, others=others, cin=inputs_of(seqs, [contig], [kind], recs, band, max_diff, min_depth), reads=reads or {}, seq=seq,
                col=col or {}, gap=gap or {}, stats=stats or {}, counts=counts or {})


def hand_cases():
    out = []
    S, P, C = cx.SINGLE, cx.PATH, cx.CIRCLE
    G = _genome(1, 200)
    g = lambda a, b: G[a:b]
    sub = lambda s, i: s[:i] + _other(s[i]) + s[i + 1:]
    # the three step kinds at the first and the last row, on a contig of one read (120 bases)
    ctg = g(0, 120)
    out.append(_case("diagonal-first-and-last-row", S, [(ctg, 120, 0)], [(g(10, 50), 10, 0), (cu.revcomp(g(60, 100)), 60, 1)],
                     reads={0: (0, 120, 120, VOTED), 1: (0, 40, 50, VOTED), 2: (0, 40, 100, VOTED)}, seq=ctg,
                     col={(10, CODE[G[10]]): 2, (49, CODE[G[49]]): 2, (9, CODE[G[9]]): 1, (50, CODE[G[50]]): 1}, stats=dict(voted=3, sum_dist=0, cells=200 * 64)))
    # a substitution in the first and in the last base of a read: a diagonal step with a mismatch (the diagonal is preferred to the up step
    # of the same cost), outvoted by the two reads that agree with the contig
    r1 = sub(sub(g(10, 50), 0), 39)
    # — in the first row.  In the last row the mismatch ties with an end one column earlier (the last base inserted behind column 48 or
    # set against it): the smaller j wins, end_j = 49
    out.append(_case("mismatch-first-and-last-row", S, [(ctg, 120, 0)], [(r1, 10, 0), (g(5, 60), 5, 0)], reads={1: (2, 40, 49, VOTED)}, seq=ctg,
                     col={(10, CODE[r1[0]]): 1, (10, CODE[G[10]]): 2}, stats=dict(sum_dist=2)))
    # an up step in row 1 at column 0, where nothing else leads: the read's extra first base goes to gap 0; two reads agree, so gap 0 emits
    x0 = _other(G[0])
    out.append(_case("up-first-row-gap-0", S, [(ctg, 120, 0)], [(x0 + g(0, 39), 0, 0), (x0 + g(0, 29), 0, 0)], reads={1: (1, 40, 39, VOTED), 2: (1, 30, 29, VOTED)},
                     seq=x0 + ctg, gap={(0, CODE[x0]): 2}, counts=dict(inserted=1, voters=3)))
    # an up step in the last row: the read's last base x is no contig base (x differs from the base before and is not the next one), the
    # end cell with the smaller j wins the tie against the mismatch one column further
    xl = _other(G[49], skip=G[50])
    out.append(_case("up-last-row", S, [(ctg, 120, 0)], [(g(10, 50) + xl, 10, 0)], reads={1: (1, 41, 50, VOTED)}, seq=ctg[:50] + xl + ctg[50:], gap={(50, CODE[xl]): 1},
                     counts=dict(inserted=1)))                              # (span(50) = min(2, 1): one vote is more than half of it)
    # a left step: the read lacks contig base 30; three such reads delete the column
    d30 = g(10, 30) + g(31, 60)
    out.append(_case("left-deletes-a-column", S, [(ctg, 120, 0)], [(d30, 10, 0)] * 3, min_depth=3, reads={1: (1, 49, 60, VOTED)}, seq=ctg[:30] + ctg[31:],
                     col={(30, 4): 3, (30, CODE[G[30]]): 1}, counts=dict(deleted=1)))
    # an insertion run of two bases: only the first base in read order is restored
    ins2 = g(10, 30) + "".join([_other(G[29], skip=G[30])] * 1) + _other(G[30], skip=G[29]) + g(30, 60)
    i0b = ins2[20]
    out.append(_case("insertion-run-of-two", S, [(ctg, 120, 0)], [(ins2, 10, 0)] * 3, reads={1: (2, 52, 60, VOTED)}, seq=ctg[:30] + i0b + ctg[30:], gap={(30, CODE[i0b]): 3},
                     counts=dict(inserted=1)))
    # gap L: three reads carry one more base behind the contig's end — the slice cuts it off (i1 = L - start): nothing to vote with
    out.append(_case("slice-cut-at-the-end", S, [(ctg, 120, 0)], [(g(90, 125), 90, 0)], reads={1: (0, 30, 120, VOTED)}, seq=ctg, stats=dict(cells=150 * 64)))
    # a read clipped at the start: start -7, i0 = 7, st = 0
    out.append(_case("slice-cut-at-the-start", S, [(ctg, 120, 0)], [(_genome(9, 7) + g(0, 30), -7, 0)], reads={1: (0, 30, 30, VOTED)}, seq=ctg))
    # gap L on a path: the last base of the contig's last read is missing in the chain read but two reads that end there... the contig ends
    # with the chain read, so a gap L vote needs a read that inserts behind column L - 1 inside its slice: read = g(90, 119) + x + G[119]
    xe = _other(G[118], skip=G[119])
    rl = g(90, 119) + xe + G[119]
    out.append(_case("gap-before-the-last-column", S, [(ctg, 120, 0)], [(rl, 89, 0)] * 2, reads={1: (1, 31, 120, VOTED)}, gap={(119, CODE[xe]): 2}, seq=ctg[:119] + xe + ctg[119:]))
    # gap L: two reads placed one column early end in a base behind the contig's last one, inside their slice (start + l = L): an up step
    # in the last row at column L; 2 * 2 > span(L) = depth[L - 1] = 3, so the polished contig is one base longer
    xL = _other(G[119])
    out.append(_case("gap-L", S, [(ctg, 120, 0)], [(g(90, 120) + xL, 89, 0)] * 2, reads={1: (1, 31, 120, VOTED)}, gap={(120, CODE[xL]): 2}, seq=ctg + xL,
                     counts=dict(inserted=1)))
    # the distance at the cap and one over it: 40 rows, max_diff 0.1 -> cap 4 (6553 * 40 >> 16 = 3: so 0.1 is 3; 0.125 is 5)
    r4 = g(10, 50)
    for i in (5, 15, 25, 35):
        r4 = sub(r4, i)
    r5 = sub(r4, 30)
    out.append(_case("distance-at-and-over-the-cap", S, [(ctg, 120, 0)], [(r4, 10, 0), (r5, 10, 0)], max_diff=0.1 + 1e-9 if False else 4 / 40,
                     reads={1: (4, 40, 50, VOTED), 2: (5, 40, 50, REJECTED)}, stats=dict(voted=2, rejected=1, sum_dist=4)))
    # min_depth - 1, on and + 1: columns 0 .. 19 have depth 1 (the chain read), 20 .. 39 depth 2, 40 .. 59 depth 3, all other reads with a
    # substitution that two of them share at 25 and at 45 (depth 2 of 3 wins at 45; at 25 it is 2 against 1 too but below min_depth = 3)
    a = sub(g(20, 60), 5); a = sub(a, 25)
    b = sub(g(40, 60), 5)
    for md, want in ((1, sub(sub(ctg, 25), 45)), (2, sub(sub(ctg, 25), 45)), (3, sub(ctg, 45)), (4, ctg)):
        cas = _case("min-depth-%d" % md, S, [(ctg, 120, 0)], [(a, 20, 0), (b, 40, 0)], min_depth=md, seq=None, stats=dict(low_depth_columns={1: 0, 2: 80, 3: 100, 4: 120}[md]))
        out.append(cas)
    # drift: a read whose first d bases are missing in the contig placement — placed d columns too far left or right of where it reads
    for W in (64, 128, 256):
        big = _genome(W, 3 * W + 40)
        for d, ok in ((W // 2 - 1, True), (W // 2, False)):
            # placed at column W, reading like the contig from column W + d: the main diagonal is off by d; cell b = W/2 + d exists iff d < W/2
            rd = big[W + d:W + d + 40]
            out.append(_case("drift-%d-band-%d" % (d, W), S, [(big, len(big), 0)], [(rd, W, 0)], band=W, max_diff=1.0,
                             reads={1: ((0, 40, W + d + 40, VOTED) if ok else None)}, seq=big))
            rd = big[W - d:W - d + 40]
            out.append(_case("drift-minus-%d-band-%d" % (d, W), S, [(big, len(big), 0)], [(rd, W, 0)], band=W, max_diff=1.0,
                             reads={1: (0, 40, W - d + 40, VOTED)}, seq=big))
    # the band clipped by j < 0 and by j > L: a contig of 50 bases, shorter than the band on both sides of a read over all of it
    small = g(100, 150)
    out.append(_case("band-clipped-at-both-ends", S, [(small, 50, 0)], [(small, 0, 0), (sub(small, 20), 0, 0)], reads={1: (0, 50, 50, VOTED), 2: (1, 50, 50, VOTED)}, seq=small))
    # a circle of four reads of 40 bases, prefixes 25 (L = 100): the fourth wraps; one read at a negative start, one longer than the circle
    ring = _genome(5, 100)
    rr = ring * 3
    chain = [(rr[0:40], 25, 0), (cu.revcomp(rr[25:65]), 25, 1), (rr[50:90], 25, 0), (cu.revcomp(rr[75:115]), 25, 1)]
    neg = rr[90:130]                                                     # start -10: columns 90 .. 129 unrolled from -10
    longr = sub(rr[30:160], 64)                                          # 130 bases: n = 100, from column 30
    out.append(_case("circle-wrap-negative-start-long-read", C, chain, [(neg, -10, 0), (longr, 30, 0)],
                     reads={3: (0, 40, 115, VOTED), 4: (0, 40, 30, VOTED), 5: (1, 100, 130, VOTED)}, seq=ring, col={(94, CODE[longr[64]]): 1}))
    # a contig no read votes on: max_diff 0 rejects the only other read, the chain read alone leaves depth 1 < min_depth
    out.append(_case("no-voter-but-the-chain", S, [(ctg, 120, 0)], [(sub(g(10, 50), 3), 10, 0)], max_diff=0.0, min_depth=2, reads={1: (1, 40, 50, REJECTED)}, seq=ctg,
                     stats=dict(voted=1, rejected=1, low_depth_columns=120), counts=dict(voters=1)))
    # ties of the column call: two reads, two different substitutions at column 30 against the chain read's base: 1 : 1 : 1, the contig's own
    # base stays; without the chain's vote (two reads A and C against own G..): see the votes
    o = G[30]
    two = [x for x in "ACGT" if x != o][:2]
    ra, rb = g(10, 30) + two[0] + g(31, 60), g(10, 30) + two[1] + g(31, 60)
    out.append(_case("tie-own-base-first", S, [(ctg, 120, 0)], [(ra, 10, 0), (rb, 10, 0)], seq=ctg))
    out.append(_case("tie-smaller-code-next", S, [(ctg, 120, 0)], [(ra, 10, 0), (ra, 10, 0), (rb, 10, 0), (rb, 10, 0)], seq=ctg[:30] + min(two, key=CODE.get) + ctg[31:],
                     counts=dict(substituted=1)))
    # a base against the deletion, 2 : 2 with the own base at 1: the base wins the tie against the deletion
    out.append(_case("tie-base-before-deletion", S, [(ctg, 120, 0)], [(ra, 10, 0), (ra, 10, 0), (d30, 10, 0), (d30, 10, 0)], seq=ctg[:30] + two[0] + ctg[31:]))
    # a gap's tie: two insertions of different bases at gap 30 from two reads each, span 5: 2 * 4 > 5, the smaller code is emitted
    ia, ib = sorted((_other(G[29], skip=G[30]), _other(G[29], skip=G[30] + _other(G[29], skip=G[30]))), key=CODE.get)
    qa, qb = g(10, 30) + ia + g(30, 60), g(10, 30) + ib + g(30, 60)
    out.append(_case("tie-gap-smaller-code", S, [(ctg, 120, 0)], [(qa, 10, 0), (qb, 10, 0), (qa, 10, 0), (qb, 10, 0)], seq=ctg[:30] + ia + ctg[30:], gap={(30, CODE[ia]): 2, (30, CODE[ib]): 2}))
    # 2 * sum = span is not enough: two inserting reads under span 4 (chain + 2 + one plain read)
    out.append(_case("gap-needs-more-than-half", S, [(ctg, 120, 0)], [(qa, 10, 0), (qa, 10, 0), (g(10, 60), 10, 0)], seq=ctg))
    return out


def check_claims(case, out, st):
    """The claims of a hand case on one output; returns None or what does not hold."""
    for r, want in case["reads"].items():
        if want is not None and tuple(int(x) for x in out["reads"][r]) != tuple(want):
            return "read %d: %r, claimed %r" % (r, out["reads"][r], want)
        if want is None and int(out["reads"][r]["status"]) == VOTED and int(out["reads"][r]["dist"]) == 0:
            return "read %d aligned without a difference outside its band" % r
    if case["seq"] is not None and out["seqs"][0] != case["seq"]:
        return "polished %r, claimed %r" % (out["seqs"][0], case["seq"])
    for (c, b), v in case["col"].items():
        if int(out["col"][c][b]) != v:
            return "col[%d][%d] = %d, claimed %d" % (c, b, out["col"][c][b], v)
    for (gg, b), v in case["gap"].items():
        if int(out["gap"][gg][b]) != v:
            return "gap[%d][%d] = %d, claimed %d" % (gg, b, out["gap"][gg][b], v)
    for k, v in case["stats"].items():
        if st[k] != v:
            return "%s = %r, claimed %r" % (k, st[k], v)
    for k, v in case["counts"].items():
        if int(out[k][0]) != v:
            return "%s = %r, claimed %r" % (k, out[k][0], v)
    return None


def pairs_of_case(case):
    """The hand case as reads + the pairs of a string graph whose contig is its chain and whose other reads are contained in the chain
    read that holds the column they start at (a read that starts before column 0 in the first): (seqs, lens, (rows, cols, vals), cflags)."""
    chain, others, kind = case["chain"], case["others"], case["kind"]
    seqs = case["cin"]["seqs"]
    lens = [len(s) for s in seqs]
    nch = len(chain)
    pairs = dict(pu.edges_of_chains(lens, [[(r, p, st) for r, (_, p, st) in enumerate(chain)]], [kind]))
    starts = np.concatenate([[0], np.cumsum([p for _, p, _ in chain])])
    L = int(starts[-1])
    for x, (s, start, sx) in enumerate(others):
        lx = len(s)
        m = start % L if kind == cx.CIRCLE and start >= L else start   # (a negative start stays: the read hangs over the first chain read's begin)
        y = max(i for i in range(nch) if starts[i] <= max(m, 0))
        ly, sy = lens[y], chain[y][2]
        rel = m - int(starts[y])                                         # oriented offset of x's base 0 on y
        obx = max(0, -rel)
        ln = min(lx - obx, ly - (rel + obx))
        assert ln >= 0
        oby = rel + obx
        bx, ex = (lx - obx - ln, lx - obx) if sx else (obx, obx + ln)
        by, ey = (ly - oby - ln, ly - oby) if sy else (oby, oby + ln)
        pairs[(y, nch + x)] = pu.pair(by, ey, bx, ex, rc=sx ^ sy, score=ln, containedT=1)
    return seqs, lens, cu.upper(pairs), (cx.CIRCULAR if kind == cx.CIRCLE else 0) | (cx.SINGLETONS if kind == cx.SINGLE else 0)


# ---- planted errors ----------------------------------------------------------------------------------------------------------------
def mutate_truth(t, rng, nerr, spacing=12, margin=5, backbone=3):
    """Plants about `nerr` errors into the reads of a placement_util.truth_set, chain reads included, and returns (the mutated reads,
    the planted sites [(read, genome position, kind)]).  Read lengths, pairs and starts stay those of the error-free layout: an indel
    is planted together with the opposite indel `spacing` bases further on in the same read, both inside the read — for a chain read
    inside the stretch no neighbouring chain read overlaps, which is part of the read's prefix whichever way the contig is walked.  Every
    read is a chain read until `backbone` sites stand in chain reads, so that the unpolished contig carries errors.  Every
    site lies on a column at least three reads cover, at least `margin` bases inside its read and `spacing` columns from every other
    site of any read; a deleted base is not in a run of two or more equal bases and an inserted base differs from both its neighbours."""
    genome, glen, circ = t["genome"], len(t["genome"]), t["circular"]
    where, chain = t["where"], t["chain_ids"]
    src = genome * 3 if circ else genome
    cover = np.zeros(glen, dtype=np.int64)
    for a, b, _ in where.values():
        for x in range(a, b):
            cover[x % glen] += 1
    private = {}
    for i, r in enumerate(chain):
        a, b, _ = where[r]
        lo = where[chain[i - 1]][1] if (i > 0 or circ) else a
        hi = where[chain[(i + 1) % len(chain)]][0] if (i + 1 < len(chain) or circ) else b
        if circ and i == 0:
            lo -= glen
        if circ and i + 1 == len(chain):
            hi += glen
        private[r] = (max(a, lo), min(b, hi))
    taken = []

    def free(x):
        return all(min((x - y) % glen, (y - x) % glen) >= spacing for y in taken) if circ else all(abs(x - y) >= spacing for y in taken)

    def norun(x):
        return src[x - 1] != src[x] and src[x] != src[x + 1]

    edits, sites = {r: {} for r in where}, []
    reads = list(where)
    tries = 0
    while len(sites) < nerr and tries < 200 * nerr:
        tries += 1
        onchain = sum(1 for rr, _, _ in sites if rr in private)
        pool = chain if onchain < backbone and tries < 100 * nerr else reads
        r = pool[int(rng.integers(0, len(pool)))]
        a, b, _ = where[r]
        lo, hi = (private[r] if r in private else (a, b))
        lo, hi = max(lo, a + margin), min(hi, b - margin)
        if hi - lo < 1:
            continue
        x = int(rng.integers(lo, hi))
        if cover[x % glen] < 3 or not free(x):
            continue
        kind = int(rng.integers(0, 3))
        if kind == 0:
            edits[r][x] = ("sub", "ACGT"[(CODE[src[x]] + int(rng.integers(1, 4))) % 4])
            taken.append(x); sites.append((r, x, "sub"))
            continue
        y = x + spacing
        if y >= hi or cover[y % glen] < 3 or not free(y) or x < 1 or y + 1 >= len(src) or not norun(x) or not norun(y):
            continue
        ins = next((c for c in "ACGT" if c != src[y - 1] and c != src[y]), None)
        if kind == 1:
            edits[r][x] = ("del", None); edits[r][y] = ("ins", ins)
        else:
            ins = next((c for c in "ACGT" if c != src[x - 1] and c != src[x]), None)
            edits[r][x] = ("ins", ins); edits[r][y] = ("del", None)
        taken += [x, y]; sites += [(r, x, edits[r][x][0]), (r, y, edits[r][y][0])]
    seqs = [None] * len(t["seqs"])
    for r, (a, b, rc) in where.items():
        out = []
        for x in range(a, b):
            e = edits[r].get(x)
            if e is None:
                out.append(src[x])
            elif e[0] == "sub":
                out.append(e[1])
            elif e[0] == "ins":
                out.append(e[1] + src[x])
        s = "".join(out)
        assert len(s) == b - a
        seqs[r] = cu.revcomp(s) if rc else s
    return seqs, sites


def same_sequence(polished, genome, circular):
    """The polished contig is the genome, in either orientation and, circular, at any rotation."""
    if len(polished) != len(genome):
        return False
    for gseq in (genome, cu.revcomp(genome)):
        if (circular and polished in gseq + gseq) or polished == gseq:
            return True
    return False
