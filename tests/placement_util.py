"""Read placements and contig depth (elba_place_reads; the rule is stated in include/elba_amd.h) restated twice in Python, a PAF parser,
hand cases with their claims, graphs that realise given chains, and a ground-truth generator.  The two restatements share nothing with
elba_amd/csrc/place.hip nor with each other: place_loops visits pairs and reads one by one with dicts (in any order it is given) and counts
depth base by base; place_tables is vectorised numpy — masks for the candidates, one lexsort for the winners, difference arrays and a
cumulative sum for the depth.

Both take the same `inp` dict (inputs_of_export / inputs_of_chains): M, base, rows, cols, vals (the graph's input pairs, list order), lens,
read_flags, skip, chain_off, chain_read, chain_prefix, chain_strand, kinds, and return (placements, stats): placements as the dict
Engine.place_reads() returns, stats as the dict of elba_place_stats without its time."""
import numpy as np

import contig_ex_util as cx
import contig_util as cu
from oracle import pyoracle as po

PLACEMENT = np.dtype([("start", "<i8"), ("contig", "<i4"), ("anchor", "<u4"), ("score", "<i4"), ("strand", "u1"), ("kind", "u1"), ("flags", "u1"), ("reserved", "u1")])
STATS = ("nreads", "chain", "anchored", "unanchored", "skipped", "empty", "candidates", "clipped", "outside", "wrapped", "segments", "max_depth", "credited_bases")
GET_STATS = ("chain", "anchored", "unanchored", "skipped", "candidates", "clipped", "outside", "wrapped", "segments", "max_depth")      # elba_get_stat "place_<name>"
NONE, CHAIN, ANCHORED = 0, 1, 2
CLIPPED, OUTSIDE, WRAPPED = 1, 2, 4
CONTAINED = 2                                                    # read flag bit 1


class BadInterval(Exception):
    """A candidate with an interval outside [0, len] or with beg > end; .pair = the smallest such index of the input list."""


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def inputs_of_export(rows, cols, vals, got, read_flags, lens, skip=1, base=0):
    """From the pairs the graph was built from, Engine.export_contigs(), Engine.export_read_flags(M) and the read lengths."""
    return dict(M=len(lens), base=base, rows=np.asarray(rows, dtype=np.int64), cols=np.asarray(cols, dtype=np.int64), vals=np.asarray(vals), lens=np.asarray(lens, dtype=np.int64),
                read_flags=np.asarray(read_flags, dtype=np.uint8), skip=int(skip), chain_off=np.asarray(got["chain_off"], dtype=np.int64),
                chain_read=np.asarray(got["chain_read"], dtype=np.int64), chain_prefix=np.asarray(got["chain_prefix"], dtype=np.int64),
                chain_strand=np.asarray(got["chain_strand"], dtype=np.uint8), kinds=np.asarray(got["kinds"], dtype=np.uint8))


def inputs_of_chains(lens, chains, kinds, rows, cols, vals, read_flags=None, skip=1):
    """From chains [[(read, prefix, strand), ...], ...] as contig_ex_util.generate_contigs_ex returns them."""
    flat = [el for ch in chains for el in ch]
    M = len(lens)
    return dict(M=M, base=0, rows=np.asarray(rows, dtype=np.int64), cols=np.asarray(cols, dtype=np.int64), vals=np.asarray(vals), lens=np.asarray(lens, dtype=np.int64),
                read_flags=np.zeros(M, np.uint8) if read_flags is None else np.asarray(read_flags, dtype=np.uint8), skip=int(skip),
                chain_off=np.concatenate([[0], np.cumsum([len(c) for c in chains])]).astype(np.int64), chain_read=np.array([r for r, _, _ in flat], dtype=np.int64),
                chain_prefix=np.array([p for _, p, _ in flat], dtype=np.int64), chain_strand=np.array([s for _, _, s in flat], dtype=np.uint8),
                kinds=np.array(kinds, dtype=np.uint8))


def contig_lens(inp):
    co = inp["chain_off"]
    return np.array([int(inp["chain_prefix"][int(a):int(b)].sum()) for a, b in zip(co[:-1], co[1:])], dtype=np.int64)


def _pack(recs, seg, cr, cb, st):
    reads = np.zeros(len(recs), dtype=PLACEMENT)
    for r, t in enumerate(recs):
        reads[r] = tuple(t) + (0,)
    seg_off = np.concatenate([[0], np.cumsum([len(s) for s in seg])]).astype(np.int64)
    flat = [x for s in seg for x in s]
    st = dict(st)
    st["segments"] = len(flat); st["max_depth"] = max((d for _, d in flat), default=0); st["credited_bases"] = int(sum(cb))
    return dict(reads=reads, seg_off=seg_off, seg_start=np.array([a for a, _ in flat], dtype=np.int32), seg_depth=np.array([d for _, d in flat], dtype=np.int32),
                credited_reads=np.array(cr, dtype=np.int64), credited_bases=np.array(cb, dtype=np.int64)), st


# ---- restatement 1: loops ----------------------------------------------------------------------------------------------------------
def _oriented_begin(b, e, length, strand):
    return length - e if strand else b


def place_loops(inp, pair_order=None, read_order=None):
    M, base, lens, skip = inp["M"], inp["base"], inp["lens"], inp["skip"]
    co = inp["chain_off"]
    L = [int(x) for x in contig_lens(inp)]
    where = {}                                                   # chain read -> (contig, start, strand)
    for k in range(len(co) - 1):
        at = 0
        for e in range(int(co[k]), int(co[k + 1])):
            where[int(inp["chain_read"][e]) - base] = (k, at, int(inp["chain_strand"][e]))
            at += int(inp["chain_prefix"][e])
    eligible = lambda x: x not in where and not (int(inp["read_flags"][x]) & skip) and int(lens[x]) > 0
    best, bad, ncand = {}, [], 0                                 # best[x] = (max(score, 0), -index)
    for a in (range(len(inp["rows"])) if pair_order is None else pair_order):
        a = int(a)
        o, q, t = inp["vals"][a], int(inp["rows"][a]) - base, int(inp["cols"][a]) - base
        if not int(o["passed"]) or (q in where) == (t in where):
            continue
        x = t if q in where else q
        if not eligible(x):
            continue
        ncand += 1
        if not (0 <= int(o["begQ"]) <= int(o["endQ"]) <= int(lens[q]) and 0 <= int(o["begT"]) <= int(o["endT"]) <= int(lens[t])):
            bad.append(a)
            continue
        key = (max(int(o["score"]), 0), -a)
        if x not in best or key > best[x]:
            best[x] = key
    if bad:
        e = BadInterval("pair %d" % min(bad)); e.pair = min(bad)
        raise e
    st = dict.fromkeys(STATS, 0)
    st["nreads"], st["candidates"] = M, ncand
    recs = [None] * M
    depth = [np.zeros(n, dtype=np.int64) for n in L]
    cr, cb = [0] * len(L), [0] * len(L)
    for r in (range(M) if read_order is None else read_order):
        r = int(r)
        l = int(lens[r])
        if r in where:
            k, start, strand = where[r]
            kind, anchor, score = CHAIN, r, 0
            st["chain"] += 1
        elif int(inp["read_flags"][r]) & skip:
            recs[r] = (0, -1, r + base, 0, 0, NONE, 0); st["skipped"] += 1
            continue
        elif l == 0:
            recs[r] = (0, -1, r + base, 0, 0, NONE, 0); st["empty"] += 1
            continue
        elif r not in best:
            recs[r] = (0, -1, r + base, 0, 0, NONE, 0); st["unanchored"] += 1
            continue
        else:
            a = -best[r][1]
            o, q, t = inp["vals"][a], int(inp["rows"][a]) - base, int(inp["cols"][a]) - base
            y = t if q == r else q
            (bx, ex), (by, ey) = ((int(o["begQ"]), int(o["endQ"])), (int(o["begT"]), int(o["endT"])))
            if q != r:
                (bx, ex), (by, ey) = (by, ey), (bx, ex)
            k, ystart, ystrand = where[y]
            strand = ystrand ^ (1 if int(o["rc"]) else 0)
            start = ystart + _oriented_begin(by, ey, int(lens[y]), ystrand) - _oriented_begin(bx, ex, l, strand)
            kind, anchor, score = ANCHORED, y, int(o["score"])
            st["anchored"] += 1
        flags, credited = 0, 0
        if int(inp["kinds"][k]) == cx.CIRCLE:
            if l > L[k]:
                flags |= CLIPPED
            for i in range(min(l, L[k])):                        # base by base round the circle
                depth[k][(start + i) % L[k]] += 1
                credited += 1
            if credited == 0:
                flags |= OUTSIDE
            elif start % L[k] + credited > L[k]:
                flags |= WRAPPED
        else:
            lo, hi = max(start, 0), min(start + l, L[k])
            if (lo, hi) != (start, start + l):
                flags |= CLIPPED
            if hi <= lo:
                flags |= OUTSIDE
            else:
                depth[k][lo:hi] += 1
                credited = hi - lo
        st["clipped"] += bool(flags & CLIPPED); st["outside"] += bool(flags & OUTSIDE); st["wrapped"] += bool(flags & WRAPPED)
        cr[k] += credited > 0; cb[k] += credited
        recs[r] = (start, k, anchor + base, score, strand, kind, flags)
    seg = []
    for d in depth:
        runs = []
        for i, v in enumerate(d.tolist()):
            if i == 0 or v != runs[-1][1]:
                runs.append((i, v))
        seg.append(runs)
    return _pack(recs, seg, cr, cb, st)


# ---- restatement 2: tables, vectorised ---------------------------------------------------------------------------------------------
def place_tables(inp):
    M, base, lens, skip = inp["M"], inp["base"], inp["lens"].astype(np.int64), inp["skip"]
    co, cread = inp["chain_off"], inp["chain_read"] - base
    nc = len(co) - 1
    nel = np.diff(co)
    cof = np.repeat(np.arange(nc), nel)                          # contig of every chain element
    pre = inp["chain_prefix"].astype(np.int64)
    before = np.cumsum(pre) - pre                                # bases before every element, over all contigs
    L = np.zeros(nc, dtype=np.int64)
    np.add.at(L, cof, pre)
    first = before[co[:-1]] if nc else np.zeros(0, np.int64)
    contig = np.full(M, -1, dtype=np.int64); start = np.zeros(M, dtype=np.int64); strand = np.zeros(M, dtype=np.int64)
    contig[cread] = cof; start[cread] = before - np.repeat(first, nel); strand[cread] = inp["chain_strand"]
    onchain = contig >= 0
    anchor = np.arange(M, dtype=np.int64); score = np.zeros(M, dtype=np.int64); kind = np.where(onchain, CHAIN, NONE)
    off = ~onchain
    flagged = (inp["read_flags"].astype(np.int64) & skip) != 0
    elig = off & ~flagged & (lens > 0)
    q, t, o = inp["rows"] - base, inp["cols"] - base, inp["vals"]
    xq = onchain[t] & ~onchain[q]                                # x is the pair's Q
    x = np.where(xq, q, t)
    cand = (o["passed"] != 0) & (onchain[q] != onchain[t]) & elig[x]
    idx = np.flatnonzero(cand)
    bq, eq, bt, et = (o[f].astype(np.int64) for f in ("begQ", "endQ", "begT", "endT"))
    okiv = (0 <= bq) & (bq <= eq) & (eq <= lens[q]) & (0 <= bt) & (bt <= et) & (et <= lens[t])
    if (~okiv[idx]).any():
        e = BadInterval("pair"); e.pair = int(idx[~okiv[idx]].min())
        raise e
    if len(idx):
        order = np.lexsort((idx, -np.maximum(o["score"][idx].astype(np.int64), 0), x[idx]))      # by read, best score first, then smallest index
        s = idx[order]
        win = s[np.concatenate([[True], x[s][1:] != x[s][:-1]])]
        wx = x[win]; wy = np.where(xq[win], t[win], q[win])
        bx = np.where(xq[win], bq[win], bt[win]); ex = np.where(xq[win], eq[win], et[win])
        by = np.where(xq[win], bt[win], bq[win]); ey = np.where(xq[win], et[win], eq[win])
        sy = strand[wy]; sx = sy ^ (o["rc"][win] != 0)
        start[wx] = start[wy] + np.where(sy == 1, lens[wy] - ey, by) - np.where(sx == 1, lens[wx] - ex, bx)
        strand[wx] = sx; contig[wx] = contig[wy]; anchor[wx] = wy; score[wx] = o["score"][win]; kind[wx] = ANCHORED
    placed = kind != NONE
    st = dict.fromkeys(STATS, 0)
    st.update(nreads=M, candidates=len(idx), chain=int(onchain.sum()), anchored=int((kind == ANCHORED).sum()), skipped=int((off & flagged).sum()),
              empty=int((off & ~flagged & (lens == 0)).sum()), unanchored=int((elig & (kind == NONE)).sum()))
    r = np.flatnonzero(placed)
    k, s0, l = contig[r], start[r], lens[r]
    Lr = L[k]
    circ = inp["kinds"][k] == cx.CIRCLE if len(r) else np.zeros(0, dtype=bool)
    safe = np.where(Lr > 0, Lr, 1)
    m = np.where(circ, np.mod(s0, safe), 0)
    cred_c = np.minimum(l, Lr)
    lo = np.where(circ, m, np.clip(s0, 0, None)); hi = np.where(circ, np.minimum(m + cred_c, Lr), np.minimum(s0 + l, Lr))
    wrap = circ & (m + cred_c > Lr)
    hi2 = np.where(wrap, m + cred_c - Lr, 0)                     # the second interval [0, hi2)
    empty = hi <= lo
    lo, hi = np.where(empty, 0, lo), np.where(empty, 0, hi)      # an outside read credits nothing
    clipped = np.where(circ, l > Lr, (np.clip(s0, 0, None) != s0) | (np.minimum(s0 + l, Lr) != s0 + l))
    fl = clipped * CLIPPED + empty * OUTSIDE + wrap * WRAPPED
    flags = np.zeros(M, dtype=np.int64); flags[r] = fl
    st.update(clipped=int(clipped.sum()), outside=int(empty.sum()), wrapped=int(wrap.sum()))
    credited = (hi - lo) + hi2
    cr = np.bincount(k[credited > 0], minlength=nc) if len(r) else np.zeros(nc, dtype=np.int64)
    cb = np.bincount(k, weights=credited, minlength=nc).astype(np.int64) if len(r) else np.zeros(nc, dtype=np.int64)
    # depth: one difference array over all contigs laid end to end (one spare slot each for the ends at L)
    coff = np.concatenate([[0], np.cumsum(L + 1)])
    diff = np.zeros(int(coff[-1]) + 1, dtype=np.int64)
    np.add.at(diff, coff[k] + lo, 1); np.add.at(diff, coff[k] + hi, -1)
    np.add.at(diff, coff[k][wrap], 1); np.add.at(diff, coff[k][wrap] + hi2[wrap], -1)
    d = np.cumsum(diff)[:-1]
    seg_off, seg_start, seg_depth = [0], [], []
    for c in range(nc):
        dc = d[coff[c]:coff[c] + L[c]]
        if len(dc):
            heads = np.flatnonzero(np.concatenate([[True], dc[1:] != dc[:-1]]))
            seg_start.append(heads); seg_depth.append(dc[heads])
        seg_off.append(seg_off[-1] + (len(seg_start[-1]) if len(dc) else 0))
    seg_start = np.concatenate(seg_start).astype(np.int32) if seg_start else np.zeros(0, np.int32)
    seg_depth = np.concatenate(seg_depth).astype(np.int32) if seg_depth else np.zeros(0, np.int32)
    reads = np.zeros(M, dtype=PLACEMENT)
    reads["start"] = np.where(placed, start, 0); reads["contig"] = np.where(placed, contig, -1); reads["anchor"] = anchor + base; reads["score"] = score
    reads["strand"] = np.where(placed, strand, 0); reads["kind"] = kind; reads["flags"] = flags
    st.update(segments=len(seg_start), max_depth=int(seg_depth.max()) if len(seg_depth) else 0, credited_bases=int(cb.sum()))
    return dict(reads=reads, seg_off=np.array(seg_off, dtype=np.int64), seg_start=seg_start, seg_depth=seg_depth, credited_reads=cr.astype(np.int64), credited_bases=cb), st


def same_placements(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("reads", "seg_off", "seg_start", "seg_depth", "credited_reads", "credited_bases"))


def first_difference(a, b):
    """For assertion messages: the first field and index at which two placement dicts differ."""
    for k in ("reads", "seg_off", "seg_start", "seg_depth", "credited_reads", "credited_bases"):
        if len(a[k]) != len(b[k]):
            return "%s: %d against %d entries" % (k, len(a[k]), len(b[k]))
        ne = np.flatnonzero(a[k] != b[k])
        if len(ne):
            return "%s[%d]: %r against %r" % (k, ne[0], a[k][ne[0]], b[k][ne[0]])
    return None


def depth_of(pl, c, length):
    """Per-base depth of contig c from its segments."""
    a, b = int(pl["seg_off"][c]), int(pl["seg_off"][c + 1])
    st = pl["seg_start"][a:b].astype(np.int64)
    return np.repeat(pl["seg_depth"][a:b].astype(np.int64), np.diff(np.concatenate([st, [length]]))) if b > a else np.zeros(0, np.int64)


# ---- PAF ---------------------------------------------------------------------------------------------------------------------------
def parse_paf(path):
    out = []
    with open(path) as f:
        for line in f:
            c = line.rstrip("\n").split("\t")
            assert len(c) == 12, line
            out.append(dict(qname=c[0], qlen=int(c[1]), qbeg=int(c[2]), qend=int(c[3]), strand=c[4], tname=c[5], tlen=int(c[6]), tbeg=int(c[7]), tend=int(c[8]),
                            score=int(c[9]), block=int(c[10]), mapq=int(c[11])))
    return out


# ---- graphs that realise chains ----------------------------------------------------------------------------------------------------
def pair(begQ, endQ, begT, endT, rc=0, score=0, passed=1, containedQ=0, containedT=0, direction=-1, directionT=-1):
    o = np.zeros(1, dtype=po.OVERLAP_DTYPE)[0]
    o["begQ"], o["endQ"], o["begT"], o["endT"], o["rc"], o["score"], o["passed"] = begQ, endQ, begT, endT, rc, score, passed
    o["containedQ"], o["containedT"], o["direction"], o["directionT"] = containedQ, containedT, direction, directionT
    return o


def edges_of_chains(lens, chains, kinds):
    """Upper-triangle entries {(i, j): overlap} of a string graph whose contigs (elba_generate_contigs_ex) are exactly `chains`: a path
    [(read, prefix, strand), ...] must start at its smaller end and end in a whole read, a circle at its smallest read towards the smaller
    neighbour; single reads need no entry.  For the step cur -> next, S(cur, next) has direction = 2 * strand(cur) + (next as stored iff it
    is the last of a path with strand 0; 1 otherwise) and suffixT = prefix(cur); the upper entry holds it as it is when cur < next and
    transposed when not."""
    edges = {}
    for ch, kd in zip(chains, kinds):
        if kd == cx.SINGLE:
            continue
        steps = list(zip(ch[:-1], ch[1:])) + ([(ch[-1], ch[0])] if kd == cx.CIRCLE else [])
        for (cur, pre, st), (nxt, _, nst) in steps:
            last = kd == cx.PATH and nxt == ch[-1][0]
            d = 2 * st + ((1 - nst) if last else 1)
            key = (min(cur, nxt), max(cur, nxt))
            o = edges.get(key)
            if o is None:
                o = pair(0, 1, 0, 1, score=1, direction=0, directionT=0)
                o["suffix"], o["suffixT"] = int(lens[key[1]]), int(lens[key[0]])
            if cur < nxt:
                o["direction"], o["suffixT"] = d, pre
            else:
                o["directionT"], o["suffix"] = d, pre
            edges[key] = o
    return edges


# ---- hand cases --------------------------------------------------------------------------------------------------------------------
def _case(name, lens, chains, kinds, pairs, skip=1, read_flags=None, reads=None, stats=None, depth=None, credited=None):
    """pairs: [(q, t, overlap)] in list order (ascending (q, t)).  Claims: reads {read: (contig, start, strand, kind, flags[, anchor])},
    stats {name: value}, depth {contig: [per-base depth]}, credited {contig: (reads, bases)}."""
    pairs = sorted(pairs, key=lambda p: (p[0], p[1]))
    rf = np.zeros(len(lens), np.uint8) if read_flags is None else np.array(read_flags, dtype=np.uint8)
    for q, t, o in pairs:                                        # what the reduction's find_contained_reads would flag
        if int(o["passed"]) and int(o["containedQ"]): rf[q] |= CONTAINED
        if int(o["passed"]) and int(o["containedT"]): rf[t] |= CONTAINED
    vals = np.array([o for _, _, o in pairs], dtype=po.OVERLAP_DTYPE) if pairs else np.zeros(0, po.OVERLAP_DTYPE)
    inp = inputs_of_chains(lens, chains, kinds, [q for q, _, _ in pairs], [t for _, t, _ in pairs], vals, rf, skip)
    return dict(name=name, inp=inp, chains=chains, cflags=(cx.CIRCULAR if cx.CIRCLE in kinds else 0) | (cx.SINGLETONS if cx.SINGLE in kinds else 0),
                reads=reads or {}, stats=stats or {}, depth=depth or {}, credited=credited or {})


def orientation_cases():
    """All eight of (anchor strand, rc, x as Q / as T).  Reads 0 and 3 of 60 bases are off the chain, 1 and 2 of 100 bases are the path
    contig (1 gives 70 bases, so 2 starts at 70; L = 170).  Each is anchored on read 2 through [5, 45) of itself and [10, 50) of read 2:
    ob_y = 10 for strand 0 and 100 - 50 = 50 for strand 1; ob_x = 5 for strand 0 and 60 - 45 = 15 for strand 1; start = 70 + ob_y - ob_x."""
    want = {(0, 0): (75, 0), (0, 1): (65, 1), (1, 0): (105, 1), (1, 1): (115, 0)}      # (strand of 2, rc) -> (start, strand of x)
    out = []
    for (sy, rc), (start, sx) in want.items():
        chains = [[(1, 70, 0), (2, 100, sy)]]
        pairs = [(0, 2, pair(5, 45, 10, 50, rc=rc, score=40, containedQ=1)), (2, 3, pair(10, 50, 5, 45, rc=rc, score=40, containedT=1))]
        fl = CLIPPED if start + 60 > 170 else 0
        out.append(_case("orient-s%d-rc%d" % (sy, rc), [60, 100, 100, 60], chains, [cx.PATH], pairs,
                         reads={0: (0, start, sx, ANCHORED, fl, 2), 3: (0, start, sx, ANCHORED, fl, 2), 1: (0, 0, 0, CHAIN, 0, 1), 2: (0, 70, sy, CHAIN, 0, 2)},
                         stats=dict(chain=2, anchored=2, candidates=2, unanchored=0, clipped=2 * bool(fl))))
    return out


def hand_cases():
    out = orientation_cases()
    P, C, S = cx.PATH, cx.CIRCLE, cx.SINGLE
    # clipping on a path of L = 50 (reads 0 and 1 of 30 bases, prefixes 20 + 30): read 2 starts at -5, read 3 hangs over the end, 4 lies
    # beyond the end, 5 before the start, 6 (80 bases) covers everything
    lens = [30, 30, 20, 20, 10, 10, 80]
    pairs = [(0, 2, pair(0, 10, 5, 15, score=10, containedT=1)),      # start = 0 + 0 - 5 = -5: credits [0, 15)
             (1, 3, pair(20, 30, 0, 10, score=10, containedT=1)),     # start = 20 + 20 - 0 = 40: credits [40, 50), 10 bases cut
             (1, 4, pair(30, 30, 0, 0, score=0, containedT=1)),       # start = 20 + 30 - 0 = 50 = L: outside
             (0, 5, pair(0, 0, 10, 10, score=0, containedT=1)),       # start = 0 + 0 - 10 = -10, -10 + 10 <= 0: outside
             (0, 6, pair(0, 30, 20, 50, score=30, containedT=1))]     # start = -20: credits [0, 50) of [-20, 60)
    depth = [3] * 15 + [2] * 5 + [3] * 10 + [2] * 10 + [3] * 10      # 0: [0, 30), 1: [20, 50), 2: [0, 15), 3: [40, 50), 6: [0, 50)
    out.append(_case("clip-path", lens, [[(0, 20, 0), (1, 30, 0)]], [P], pairs,
                     reads={2: (0, -5, 0, ANCHORED, CLIPPED, 0), 3: (0, 40, 0, ANCHORED, CLIPPED, 1), 4: (0, 50, 0, ANCHORED, CLIPPED | OUTSIDE, 1),
                            5: (0, -10, 0, ANCHORED, CLIPPED | OUTSIDE, 0), 6: (0, -20, 0, ANCHORED, CLIPPED, 0), 0: (0, 0, 0, CHAIN, 0, 0), 1: (0, 20, 0, CHAIN, 0, 1)},
                     stats=dict(chain=2, anchored=5, clipped=5, outside=2, wrapped=0, candidates=5), depth={0: depth}, credited={0: (5, 30 + 30 + 15 + 10 + 50)}))
    # a chain read that runs over the end of its contig: the first read of 40 bases contributes 10 and the last read of 20 bases ends the
    # contig at 30, so read 0 is cut at 30
    out.append(_case("clip-chain-read", [40, 20], [[(0, 10, 1), (1, 20, 0)]], [P], [],
                     reads={0: (0, 0, 1, CHAIN, CLIPPED, 0), 1: (0, 10, 0, CHAIN, 0, 1)}, stats=dict(chain=2, clipped=1, candidates=0),
                     depth={0: [1] * 10 + [2] * 20}, credited={0: (2, 50)}))
    # a circle of 4 reads x 25 bases of prefix (L = 100, reads of 40 bases): read 3 starts at 75 and wraps; read 4 is anchored at a negative
    # start (-10 mod 100 = 90: wraps); read 5 of 130 bases is longer than the circle: 100 bases from its start mod L
    lens = [40, 40, 40, 40, 30, 130]
    chains = [[(0, 25, 0), (1, 25, 1), (2, 25, 0), (3, 25, 1)]]
    pairs = [(0, 4, pair(0, 20, 10, 30, score=20, containedT=1)),     # start = 0 + 0 - 10 = -10
             (1, 5, pair(0, 40, 50, 90, rc=1, score=40, containedT=1))]      # strand(1) = 1: ob_y = 40 - 40 = 0; strand(5) = 0: ob_x = 50; start = 25 - 50 = -25 -> 75
    d = np.zeros(100, dtype=np.int64)
    for s, n in ((0, 40), (25, 40), (50, 40), (75, 40), (90, 30), (75, 100)):
        for i in range(n):
            d[(s + i) % 100] += 1
    out.append(_case("circle", lens, chains, [C], pairs,
                     reads={3: (0, 75, 1, CHAIN, WRAPPED, 3), 4: (0, -10, 0, ANCHORED, WRAPPED, 0), 5: (0, -25, 0, ANCHORED, CLIPPED | WRAPPED, 1), 0: (0, 0, 0, CHAIN, 0, 0)},
                     stats=dict(chain=4, anchored=2, wrapped=3, clipped=1, outside=0), depth={0: d.tolist()}, credited={0: (6, 4 * 40 + 30 + 100)}))
    # ties and scores: read 4 has three candidates of score 7 (the first in the list wins: x as T of pair (0, 4)), read 5 a negative score
    # beside a zero score (both count as 0: the first wins), read 6 only a pair that did not pass, read 7 a pair with another off-chain read
    lens = [50, 50, 50, 50, 20, 20, 20, 20, 20]
    chains = [[(0, 30, 0), (1, 30, 0), (2, 30, 0), (3, 50, 0)]]
    pairs = [(0, 4, pair(10, 30, 0, 20, score=7, containedT=1)), (1, 4, pair(0, 20, 0, 20, score=7, containedT=1)), (2, 4, pair(5, 25, 0, 20, score=7, containedT=1)),
             (1, 5, pair(0, 20, 0, 20, score=-3, containedT=1)), (2, 5, pair(0, 20, 0, 20, score=0, containedT=1)),
             (3, 6, pair(0, 20, 0, 20, score=9, passed=0)), (6, 7, pair(0, 20, 0, 20, score=9)), (0, 3, pair(0, 1, 0, 1, score=99))]
    out.append(_case("ties", lens, chains, [P], pairs,
                     reads={4: (0, 10, 0, ANCHORED, 0, 0), 5: (0, 30, 0, ANCHORED, 0, 1), 6: (-1, 0, 0, NONE, 0, 6), 7: (-1, 0, 0, NONE, 0, 7), 8: (-1, 0, 0, NONE, 0, 8)},
                     stats=dict(chain=4, anchored=2, unanchored=3, candidates=5, skipped=0, empty=0)))
    # the skip mask, empty reads, single-read contigs: read 0 is a contig of its own; 1 is contained in it; 2 is contained and bad (flags 3);
    # 3 is empty
    lens = [40, 10, 10, 0]
    pairs = [(0, 1, pair(5, 15, 0, 10, score=10, containedT=1)), (0, 2, pair(20, 30, 0, 10, rc=1, score=10, containedT=1))]
    for skip, want in ((0, dict(anchored=2, skipped=0)), (1, dict(anchored=1, skipped=1)), (255, dict(anchored=0, skipped=2))):
        out.append(_case("skip-%d" % skip, lens, [[(0, 40, 0)]], [S], pairs, skip=skip, read_flags=[0, 0, 1, 0],
                         reads={0: (0, 0, 0, CHAIN, 0, 0), 3: (-1, 0, 0, NONE, 0, 3), **({1: (0, 5, 0, ANCHORED, 0, 0)} if skip != 255 else {}),
                                **({2: (0, 20, 1, ANCHORED, 0, 0)} if skip == 0 else {})},
                         stats=dict(chain=1, empty=1, unanchored=0, **want)))
    return out


# ---- ground truth ------------------------------------------------------------------------------------------------------------------
def truth_set(rng, glen, nchain, circular, ncontained, nextra):
    """An error-free layout: `nchain` reads tile a linear or circular genome, each overlapping only its neighbours (the string graph's
    path or circle); `ncontained` reads lie inside one chain read each (their pairs carry the contained flag); `nextra` reads hang over
    the junction of two chain reads without being contained (their pairs carry no direction, so the reduction drops them).  Every pair is
    a full Overlap derived from the layout alone: intervals in forward read coordinates, rc, score = the shared bases, passed.
    Returns dict(seqs, lens, edges {(i, j): overlap of the graph}, pairs (rows, cols, vals: the input list), genome, where {read: (begin,
    end, rc)} in unrolled genome coordinates, chain_ids (layout order), read_flags)."""
    M = nchain + ncontained + nextra
    ids = rng.permutation(M)
    genome = cx.random_genome(rng, glen)
    gaps = 12 + rng.multinomial(glen - 12 * nchain, np.ones(nchain) / nchain)
    p = np.concatenate([[0], np.cumsum(gaps)]).astype(np.int64)
    if circular:
        ov = [int(rng.integers(4, gaps[(i + 1) % nchain] - 2)) for i in range(nchain)]
        e = [int(p[i + 1]) + ov[i] for i in range(nchain)]
    else:
        ov = [int(rng.integers(4, gaps[i + 1] - 2)) for i in range(nchain - 1)]
        e = [int(p[i + 1]) + ov[i] for i in range(nchain - 1)] + [glen]
    src = genome * 3 if circular else genome
    where = {}
    for i in range(nchain):
        where[int(ids[i])] = (int(p[i]), e[i], int(rng.integers(0, 2)))
    chain_ids = [int(x) for x in ids[:nchain]]
    at = nchain
    for _ in range(ncontained):                                  # strictly inside one chain read
        i = int(rng.integers(0, nchain))
        b0, e0, _ = where[chain_ids[i]]
        a = int(rng.integers(b0 + 1, e0 - 6)); b = int(rng.integers(a + 4, e0))
        where[int(ids[at])] = (a, b, int(rng.integers(0, 2))); at += 1
    for _ in range(nextra):                                      # over the junction of chain reads i and i + 1, inside neither
        i = int(rng.integers(0, nchain if circular else nchain - 1))
        b0, e0, _ = where[chain_ids[i]]
        nb = int(p[i + 1])                                       # where the next chain read begins (unrolled)
        a = int(rng.integers(b0 + 1, nb)); b = int(rng.integers(e0 + 1, e0 + 3))
        if not circular:
            b = min(b, glen)
        where[int(ids[at])] = (a, b, int(rng.integers(0, 2))); at += 1
    seqs = [None] * M
    for r, (a, b, rc) in where.items():
        s = src[a:b]
        seqs[r] = cu.revcomp(s) if rc else s
    lens = [len(s) for s in seqs]

    def fwd(r, a, b, shift=0):                                   # the genome interval [a, b) in forward coordinates of read r
        b0, e0, rc = where[r]
        b0 += shift; e0 += shift
        return (e0 - b, e0 - a) if rc else (a - b0, b - b0)

    def overlap(x, y, shift_y=0):                                # x < y ids; y's interval shifted by shift_y turns
        (ax, bx, rx), (ay, by, ry) = where[x], where[y]
        a, b = max(ax, ay + shift_y), min(bx, by + shift_y)
        if b - a < 1:
            return None
        o = pair(*fwd(x, a, b), *fwd(y, a, b, shift_y), rc=rx ^ ry, score=b - a)
        return o

    edges, pairs = {}, {}
    for i in range(nchain if circular else nchain - 1):
        j = (i + 1) % nchain
        x, y = chain_ids[i], chain_ids[j]
        rci, rcj = where[x][2], where[y][2]
        turn = glen if j == 0 else 0
        step_f = (2 * rci + (1 - rcj), int(p[i + 1]) - int(p[i]))                  # i -> j, with the layout
        step_b = (2 * (1 - rcj) + rci, e[j] + turn - e[i])                         # j -> i, against it
        q2t, t2q = (step_f, step_b) if x < y else (step_b, step_f)
        o = overlap(min(x, y), max(x, y), (turn if y > x else -turn))
        o["direction"], o["suffixT"], o["directionT"], o["suffix"] = q2t[0], q2t[1], t2q[0], t2q[1]
        edges[(min(x, y), max(x, y))] = o
    pairs.update(edges)
    read_flags = np.zeros(M, dtype=np.uint8)
    turns = (-glen, 0, glen) if circular else (0,)
    for r in (int(x) for x in ids[nchain:]):
        contained = False
        for y in chain_ids:
            for tn in turns:
                lo, hi = min(r, y), max(r, y)
                o = overlap(lo, hi, (tn if hi == y else -tn))
                if o is None:
                    continue
                a0, b0, _ = where[r]
                ya, yb, _ = where[y]
                inside = ya + tn <= a0 and b0 <= yb + tn
                if inside:
                    o["containedQ" if lo == r else "containedT"] = 1
                    contained = True
                pairs[(lo, hi)] = o
        if contained:
            read_flags[r] |= CONTAINED
    rows, cols, vals = cu.upper(pairs)
    return dict(seqs=seqs, lens=lens, edges=edges, pairs=(rows, cols, vals), genome=genome, where=where, chain_ids=chain_ids, read_flags=read_flags, circular=circular)


def oriented(seq, strand):
    return cu.revcomp(seq) if strand else seq
