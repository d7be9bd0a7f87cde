"""A plain numpy restatement of the read pileup (elba_read_pileup, pileup.hip): per-base depth by np.add.at difference arrays, the profile as
(start, depth) segments, GetTrimmedInterval (src/PruneChimeras.cpp:31-69) transcribed line by line with the return fixed, the flags and
PruneFull.  Shares nothing with elba_amd/csrc/pileup.hip, in the spirit of string_graph_util.py.  Also: the reference's literal pileup of
the upper-triangular R (only the column read credited, :137-146) and its literal trim loop (the open run returned), to pin the two deviations."""
import numpy as np


class BadInterval(ValueError):
    pass


def accepted(vals, mode):
    return (vals["passed"] != 0) if mode == 0 else (vals["score"] > 0)


def intervals(lens, rows, cols, vals, mode=0, margin=0):
    """(read, beg, end) of every credited interval: both reads of every accepted pair, shrunk by margin, empty ones dropped."""
    lens = np.asarray(lens, dtype=np.int64)
    rows = np.asarray(rows, dtype=np.int64); cols = np.asarray(cols, dtype=np.int64)
    acc = accepted(vals, mode)
    r, c, v = rows[acc], cols[acc], vals[acc]
    for (who, b, e) in ((r, v["begQ"], v["endQ"]), (c, v["begT"], v["endT"])):
        b = b.astype(np.int64); e = e.astype(np.int64)
        bad = (b < 0) | (b > e) | (e > lens[who])
        if bad.any():
            raise BadInterval("interval outside [0, len] or beg > end at accepted pair %d" % int(np.flatnonzero(bad)[0]))
    reads = np.concatenate([r, c])
    beg = np.concatenate([v["begQ"], v["begT"]]).astype(np.int64) + margin
    end = np.concatenate([v["endQ"], v["endT"]]).astype(np.int64) - margin
    keep = beg < end
    return reads[keep], beg[keep], end[keep], int(acc.sum())


def depths(lens, reads, beg, end):
    """Per-base depth of every read, concatenated (read v at off[v] .. off[v] + lens[v]); np.add.at over a difference array of len + 1 per read."""
    lens = np.asarray(lens, dtype=np.int64)
    off1 = np.concatenate([[0], np.cumsum(lens + 1)])
    diff = np.zeros(int(off1[-1]) + 1, dtype=np.int64)
    np.add.at(diff, off1[reads] + beg, 1)
    np.add.at(diff, off1[reads] + end, -1)
    d = np.cumsum(diff[:-1])                                  # every read's deltas sum to 0: one global prefix sum
    keep = np.ones(len(d), dtype=bool)
    keep[off1[1:] - 1] = False                                 # the extra slot at len of every read
    return d[keep], np.concatenate([[0], np.cumsum(lens)])


def segments(depth, off):
    """(seg_off, seg_start, seg_depth): maximal runs of equal depth of every read."""
    n = len(off) - 1
    if len(depth) == 0:
        return np.zeros(n + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int32)
    first = np.zeros(len(depth), dtype=bool)
    first[off[:-1][off[1:] > off[:-1]]] = True
    change = first.copy()
    change[1:] |= depth[1:] != depth[:-1]
    idx = np.flatnonzero(change)
    read = np.searchsorted(off, idx, side="right") - 1
    seg_off = np.concatenate([[0], np.cumsum(np.bincount(read, minlength=n))]).astype(np.int64)
    return seg_off, (idx - off[read]).astype(np.int32), depth[idx].astype(np.int32)


def trimmed_interval_literal(pileup, threshold, maxlen=2500, fixed=True):
    """PileupVector::GetTrimmedInterval (src/PruneChimeras.cpp:30-69) line by line.  fixed=True returns the best run, half-open
    (beststart, bestend + 1), or (-1, -1); fixed=False returns what the reference returns: (start, end) of the run open at the last base."""
    length = len(pileup)
    beststart, bestend = -1, -1
    bestavg = 0.0
    curbases = 0
    start, end = -1, -1
    for i in range(length):
        if pileup[i] >= threshold:
            if start == -1:
                curbases = 0
                start = i
            end = i
            curbases += int(pileup[i])
            span = end - start + 1
            curavg = float(curbases) / float(span)
            if span > maxlen and curavg > bestavg:
                beststart = start
                bestend = end
                maxlen = span
                bestavg = curavg
        else:
            start = -1
            end = -1
    if not fixed:
        return (start, end)
    return (beststart, bestend + 1) if beststart >= 0 else (-1, -1)


def _runs(pileup, threshold):
    m = np.concatenate([[False], np.asarray(pileup) >= threshold, [False]])
    d = np.diff(m.astype(np.int8))
    return np.flatnonzero(d == 1), np.flatnonzero(d == -1)


def trimmed_interval(pileup, threshold, maxlen=2500):
    """The same rule as trimmed_interval_literal(fixed=True), vectorised per run: inside a run only bases with span > maxlen can replace
    the best, and from the first of them on every base is eligible (a replacement sets maxlen = span), so the replacements are the bases
    whose curavg beats the running maximum (bestavg included).  The CPU tests hold it equal to the literal loop."""
    pileup = np.asarray(pileup, dtype=np.int64)
    best = (-1, -1)
    bestavg = 0.0
    for s, e in zip(*_runs(pileup, threshold)):
        if e - s <= maxlen:
            continue
        cb = np.cumsum(pileup[s:e])
        span = np.arange(1, e - s + 1, dtype=np.int64)
        el = span > maxlen
        avg = cb[el].astype(np.float64) / span[el].astype(np.float64)
        run_max = np.maximum.accumulate(np.concatenate([[bestavg], avg]))[:-1]
        hit = np.flatnonzero(avg > run_max)
        if len(hit):
            j = int(hit[-1])
            i = int(np.flatnonzero(el)[j])
            best = (int(s), int(s + i + 1))
            maxlen = int(span[i])
            bestavg = float(avg[j])
    return best


def long_runs(pileup, threshold, min_run):
    s, e = _runs(pileup, threshold)
    return int(((e - s) >= min_run).sum())


def pileup(lens, rows, cols, vals, mode=0, margin=0, min_depth=1, min_run=1, trim_len=2500):
    """Everything elba_read_pileup computes: dict of seg_off, seg_start, seg_depth, trim_beg, trim_end, flags, and the stats."""
    lens = np.asarray(lens, dtype=np.int64)
    n = len(lens)
    reads, beg, end, used = intervals(lens, rows, cols, vals, mode, margin)
    depth, off = depths(lens, reads, beg, end)
    seg_off, seg_start, seg_depth = segments(depth, off)
    tb = np.full(n, -1, np.int32); te = np.full(n, -1, np.int32); flags = np.zeros(n, np.uint8)
    for v in range(n):
        p = depth[off[v]:off[v + 1]]
        lr = long_runs(p, min_depth, min_run)
        flags[v] = (1 if lr == 0 else 0) | (2 if lr >= 2 else 0)
        tb[v], te[v] = trimmed_interval(p, min_depth, trim_len)
    trimmed = ~((tb == 0) & (te == lens))
    st = dict(nreads=n, pairs=used, intervals=len(reads), segments=len(seg_start), max_depth=int(depth.max()) if len(depth) else 0,
              unsupported=int((flags & 1).astype(bool).sum()), split=int((flags & 2).astype(bool).sum()), trimmed=int(trimmed.sum()),
              trimmed_bases=int(np.where(tb >= 0, te.astype(np.int64) - tb, 0).sum()))
    return dict(n=n, seg_off=seg_off, seg_start=seg_start, seg_depth=seg_depth, trim_beg=tb, trim_end=te, flags=flags), st, depth, off


def profile_of(seg_off, seg_start, seg_depth, lens, v):
    """The per-base depth of read v rebuilt from its segments."""
    a, b = int(seg_off[v]), int(seg_off[v + 1])
    ends = np.concatenate([seg_start[a + 1:b], [lens[v]]]).astype(np.int64)
    return np.repeat(seg_depth[a:b].astype(np.int64), ends - seg_start[a:b])


def reference_upper_pileup(lens, rows, cols, vals, mode=0):
    """GetReadPileup (src/PruneChimeras.cpp:108-158) literally on the upper-triangular R: every column's nonzeros add their (begT, endT)
    to the COLUMN read only; the row read gets nothing from the pair.  Per-read lists of ints, as PileupVector holds them."""
    pv = [[0] * int(l) for l in lens]
    acc = accepted(vals, mode)
    for c, o, a in zip(cols, vals, acc):
        if not a:
            continue
        b, e = int(o["begT"]), int(o["endT"])
        assert b >= 0 and e <= len(pv[int(c)])
        for i in range(b, e):
            pv[int(c)][i] += 1
    return pv


def prune(rows, cols, vals, flags, mask):
    """R->PruneFull(x, x) for x = {v : flags[v] & mask}: the pairs with neither end in x, order kept."""
    bad = (np.asarray(flags) & mask) != 0
    keep = ~(bad[np.asarray(rows)] | bad[np.asarray(cols)])
    return np.asarray(rows)[keep], np.asarray(cols)[keep], vals[keep]
