"""Case builders for the boundary tests of contig polishing (polish.hip): reads aimed at one lane-level mechanism of one kernel each, with
what every case claims about itself.  No GPU and no pytest here: test_consensus_edges_cpu.py holds every claim, every structural condition
and every placement against the restatements (consensus_util.py, placement_util.py) before test_gpu_consensus_edges.py spends GPU time.

A case is built from parts, one per contig: each part is a consensus_util._case (a chain and the reads contained in it, with its claims
in the contig's own coordinates; part["via"] = {read: chain read} anchors a read on a chain read of its choice).  assemble() lays the parts side by side under one numbering of the reads, optionally with reads between
them that the polish never places (`unplaced`), and returns a dict:
  name, cin (the restatements' input), pairs (rows, cols, vals of the string graph's input), cflags, cutoff (of the transitive reduction:
  0.5 where a case has bad reads), skip, read_flags (string_graph_util.kept_edges: bit 0 bad, bit 1 contained), chains, kinds,
  parts [(part, {local read: global read})], stats (claims on the call's stats), structure (conditions on the walks, see check_structure),
  seq_off (claimed where every part claims its sequence: the polished contigs laid end to end),
  trace (settings of polish_trace_bytes under which the result must not change), loops (False: too large for polish_loops in a second)."""
import functools

import numpy as np

import consensus_util as cs
import contig_ex_util as cx
import contig_util as cu
import placement_util as pu
import string_graph_util as sgu

S, P, C = cx.SINGLE, cx.PATH, cx.CIRCLE
VOTED, REJECTED, OUTSIDE, NOT_PLACED = cs.VOTED, cs.REJECTED, cs.OUTSIDE, cs.NOT_PLACED
CODE = cs.CODE


def assemble(name, parts, unplaced=(), stats=None, structure=(), trace=(), loops=True, cutoff=0.0, skip=1):
    """unplaced: [(position in the final numbering, sequence, how)], ascending; how = "lone" (no pair at all) or ("bad", chain read as
    (part, local read), [three placed reads as (part, local read)]): a passed contained pair with the chain read and three pairs that
    did not pass, so (1 + 1) / (4 + 1) <= cutoff = 0.5 makes the read bad and skip_flags 1 keeps it from being placed.  Band, max_diff
    and min_depth are those of the first part."""
    tokens = [(k, r) for k, p in enumerate(parts) for r in range(len(p["cin"]["seqs"]))]
    for pos, seq, how in unplaced:
        tokens.insert(pos, ("u", seq, how))
    gid = {t: i for i, t in enumerate(tokens) if t[0] != "u"}
    M = len(tokens)
    seqs, recs, pairs, cflags = [None] * M, np.zeros(M, dtype=pu.PLACEMENT), {}, 0
    for k, p in enumerate(parts):
        ps, _, (rows, cols, vals), fl = cs.pairs_of_case(p)
        cflags |= fl
        for r, s in enumerate(ps):
            seqs[gid[(k, r)]] = s
            rec = p["cin"]["reads"][r].copy()
            rec["contig"] = k
            recs[gid[(k, r)]] = rec
        for a, b, o in zip(rows, cols, vals):
            if int(b) not in p.get("via", {}):
                pairs[(gid[(k, int(a))], gid[(k, int(b))])] = o
        for r, y in p.get("via", {}).items():
            pairs[(gid[(k, y)], gid[(k, r)])] = _pair_through(p, r, y)
    for i, t in enumerate(tokens):
        if t[0] != "u":
            continue
        _, seq, how = t
        seqs[i] = seq
        recs[i] = (0, -1, i, 0, 0, pu.NONE, 0, 0)
        if how == "lone":
            continue
        _, y, failed = how
        y, l = gid[y], len(seq)
        assert y < i and len(seqs[y]) >= l
        pairs[(y, i)] = pu.pair(0, l, 0, l, score=l, containedT=1)
        for z in failed:
            z = gid[z]
            pairs[(min(z, i), max(z, i))] = pu.pair(0, 1, 0, 1, score=1, passed=0)
    first = parts[0]["cin"]
    cin = cs.inputs_of(seqs, [p["cin"]["contigs"][0] for p in parts], [p["kind"] for p in parts], recs, first["band"], first["max_diff_q16"] / 65536.0, first["min_depth"])
    rows, cols, vals = cu.upper(pairs)
    chains = [[(gid[(k, r)], pre, st) for r, (_, pre, st) in enumerate(p["chain"])] for k, p in enumerate(parts)]
    return dict(name=name, cin=cin, pairs=(rows, cols, vals), cflags=cflags, cutoff=cutoff, skip=skip, read_flags=sgu.kept_edges(M, rows, cols, vals, cutoff)[1], chains=chains,
                kinds=[p["kind"] for p in parts], parts=[(p, {r: gid[(k, r)] for r in range(len(p["cin"]["seqs"]))}) for k, p in enumerate(parts)], stats=stats or {},
                structure=list(structure), trace=list(trace), loops=loops,
                seq_off=[sum(len(p["seq"]) for p in parts[:k]) for k in range(len(parts) + 1)] if all(p["seq"] is not None for p in parts) else None)


def _pair_through(part, r, y):
    """The pair that anchors other read r of a part on chain read y at the start the part writes down, not reduced by a turn of the ring
    (consensus_util.pairs_of_case takes the chain read that holds the start modulo L)."""
    chain, nch = part["chain"], len(part["chain"])
    s, start, sx = part["others"][r - nch]
    sy, ly, lx = chain[y][2], len(chain[y][0]), len(s)
    rel = start - sum(pre for _, pre, _ in chain[:y])
    obx = max(0, -rel)
    ln = min(lx - obx, ly - (rel + obx))
    assert ln > 0
    oby = rel + obx
    bx, ex = (lx - obx - ln, lx - obx) if sx else (obx, obx + ln)
    by, ey = (ly - oby - ln, ly - oby) if sy else (oby, oby + ln)
    return pu.pair(by, ey, bx, ex, rc=sx ^ sy, score=ln, containedT=1)


def check_claims(case, out, st):
    """Every part's claims (consensus_util._case: reads, seq, col, gap, counts, in the part's own coordinates) and the case's stats on one
    output of the whole call; None or what does not hold."""
    for k, (p, gid) in enumerate(case["parts"]):
        at = int(out["col_off"][k])
        for r, want in p["reads"].items():
            if any(w is not None and int(x) != w for x, w in zip(out["reads"][gid[r]], want)):       # (None: no claim on that field)
                return "contig %d read %d: %r, claimed %r" % (k, gid[r], out["reads"][gid[r]], want)
        if p["seq"] is not None and out["seqs"][k] != p["seq"]:
            return "contig %d polished %r, claimed %r" % (k, out["seqs"][k], p["seq"])
        for (c, b), v in p["col"].items():
            if int(out["col"][at + c][b]) != v:
                return "contig %d col[%d][%d] = %d, claimed %d" % (k, c, b, out["col"][at + c][b], v)
        for (g, b), v in p["gap"].items():
            if int(out["gap"][at + k + g][b]) != v:
                return "contig %d gap[%d][%d] = %d, claimed %d" % (k, g, b, out["gap"][at + k + g][b], v)
        for f, v in p["counts"].items():
            if int(out[f][k]) != v:
                return "contig %d %s = %d, claimed %d" % (k, f, out[f][k], v)
    for f, v in case["stats"].items():
        if st[f] != v:
            return "%s = %r, claimed %r" % (f, st[f], v)
    if case["seq_off"] is not None:
        got = out["seq_off"] if "seq_off" in out else np.concatenate([[0], np.cumsum([len(x) for x in out["seqs"]])])
        if [int(x) for x in got] != case["seq_off"]:
            return "seq_off = %r, claimed %r" % (list(got), case["seq_off"])
    return None


def check_structure(case, walks, out):
    """The conditions of case["structure"] on the walks of consensus_util.walked_steps; None or what does not hold.
      ("left", read, run, first cell, last cell)   the walk has one run of left steps: `run` cells of one row, band cells first .. last
      ("up", read, run, first row, last row, column)   one run of up steps: rows first .. last at that column
      ("block", read)   an up run of the read covers a whole block of 64 rows counted from the read's last row
      ("seam", read, which, d)   the first (which = 0) or last (1) row of the read's longest up run is row n - 64 k + d for some k
      ("endj", read, below)   the read's end_j lies below `below`"""
    for cond in case["structure"]:
        what, r = cond[0], cond[1]
        if what == "endj":
            if int(out["reads"][r]["end_j"]) >= cond[2]:
                return "read %d: end_j %d, wanted one below %d" % (r, out["reads"][r]["end_j"], cond[2])
            continue
        steps = walks.get(r)
        if steps is None:
            return "read %d did not vote" % r
        n = steps[0][1]
        lefts, ups = cs.runs_of(steps, 2), cs.runs_of(steps, 1)
        if what == "left":
            _, _, run, b0, b1 = cond
            if [(x[1] - x[0], x[3] - x[2] + 1, x[4], x[5]) for x in lefts] != [(0, run, b0, b1)]:
                return "read %d: left runs %r, wanted one of %d over cells %d .. %d" % (r, lefts, run, b0, b1)
        elif what == "up":
            _, _, run, i0, i1, j = cond
            if [(x[0], x[1], x[2], x[3]) for x in ups] != [(i0, i1, j, j)] or i1 - i0 + 1 != run:
                return "read %d: up runs %r, wanted rows %d .. %d at column %d" % (r, ups, i0, i1, j)
        elif what == "block":
            if not any(any(x[0] <= n - 64 * k - 63 and n - 64 * k <= x[1] for k in range(n // 64 + 1)) for x in ups):
                return "read %d: no up run %r covers a whole block below row %d" % (r, ups, n)
        elif what == "seam":
            _, _, which, d = cond
            x = max(ups, key=lambda u: u[1] - u[0])
            if (n + d - x[which]) % 64:
                return "read %d: row %d of the up run is not row n - 64 k %+d of n = %d" % (r, x[which], d, n)
    return None


# ---- building blocks ---------------------------------------------------------------------------------------------------------------
def _seq(seed, n, first=None, last=None):
    """n bases without two equal neighbours, with a given first and / or last base."""
    s = list(cs._genome(seed, n))
    if first is not None and s[0] != first:
        s[0] = first
        if n > 1 and s[1] == first:
            s[1] = cs._other(first, skip=s[2] if n > 2 else "")
    if last is not None and s[-1] != last:
        s[-1] = last
        if n > 1 and s[-2] == last:
            s[-2] = cs._other(last, skip=s[-3] if n > 2 else "")
    assert all(a != b for a, b in zip(s, s[1:]))
    return "".join(s)


def _sub(s, i):
    return s[:i] + cs._other(s[i]) + s[i + 1:]


def _stored(s, strand):
    return cu.revcomp(s) if strand else s


def _region(run):
    return ("AC" * run)[:run]


# ---- A: left runs across the lane groups of the prefix-minimum scan ------------------------------------------------------------------
def left_run_part(W, run, c0):
    """contig = head + region + tail, two reads (one per strand) = head[W:] + tail[:arm], placed so that the head runs on band cell c0:
    the region's `run` columns are one run of left steps in row len(head) - W over band cells c0 + 1 .. c0 + run.  The head ends in G, the
    region is ACAC.., the tail starts with T: no base of the run can be matched instead.  Arms of 3 x run keep the free begin and end from
    paying for a mismatched arm instead."""
    arm = max(3 * run, 16)
    head, region, tail = _seq(3 * W + run, arm + W, last="G"), _region(run), _seq(5 * W + run, arm + W // 2 + 7, first="T")
    contig, read = head + region + tail, head[W:] + tail[:arm]
    start = W + W // 2 - c0
    hl, n = len(head), 2 * arm
    return cs._case("left-%d-from-%d" % (run, c0), S, [(contig, len(contig), 0)], [(_stored(read, 0), start, 0), (_stored(read, 1), start, 1)], band=W, max_diff=1.0, min_depth=1,
                    reads={1: (run, n, hl + run + arm, VOTED), 2: (run, n, hl + run + arm, VOTED)}, seq=head + tail, col={(hl, 4): 2, (hl + run - 1, 4): 2, (hl - 1, CODE["G"]): 3},
                    counts=dict(deleted=run, voters=3, inserted=0, substituted=0))


@functools.lru_cache(None)
def left_run_cases():
    out = []
    for Cc in (1, 2, 4):
        W = 64 * Cc
        variants = [("all-lane-groups", W - 8 - (2 if Cc > 1 else 0), 3)]
        variants += [("only-%d" % (q * Cc), 4 * Cc, q * Cc - 2 * Cc) for q in (16, 32, 48)]
        variants.append(("ends-on-the-last-cell", 4 * Cc + 3, W - 1 - (4 * Cc + 3)))
        for tag, run, c0 in variants:
            part = left_run_part(W, run, c0)
            out.append(assemble("left-band-%d-%s" % (W, tag), [part], structure=[("left", r, run, c0 + 1, c0 + run) for r in (1, 2)], loops=W == 64, stats=dict(voted=3, sum_dist=2 * run)))
    return out


def lane_groups_crossed(b0, b1, Cc):
    """Which of the cells 16 C, 32 C, 48 C a run over band cells b0 .. b1 crosses: the left neighbour of b0 lies below it, b1 on or above."""
    return [q for q in (16, 32, 48) if b0 - 1 < q * Cc <= b1]


# ---- B: up runs across the blocks of the walk ---------------------------------------------------------------------------------------
def up_run_part(W, run, tails):
    """contig = head + tail, reads = head[W:] + region + tail[:t] for t in tails, strands alternating, the head on band cell W - 3: one
    run of `run` up steps at column len(head), one gap vote for the region's first base."""
    arm = max(3 * run, 16)
    head, region, tail = _seq(7 * W + run, arm + W, last="G"), _region(run), _seq(9 * W + run, max(tails) + run + 9, first="T")
    contig = head + tail
    hl, start = len(head), W // 2 + 3
    others = [(_stored(head[W:] + region + tail[:t], x & 1), start, x & 1) for x, t in enumerate(tails)]
    m = len(tails)
    enough = 2 * m > m + 1
    return cs._case("up-%d" % run, S, [(contig, len(contig), 0)], others, band=W, max_diff=1.0, min_depth=1,
                    reads={1 + x: (run, arm + run + t, hl + t, VOTED) for x, t in enumerate(tails)}, seq=head + ("A" if enough else "") + tail, gap={(hl, CODE["A"]): m},
                    counts=dict(inserted=int(enough), deleted=0, voters=m + 1, substituted=0))


def _tail_for(arm, want):
    """The smallest t >= arm with t = want (mod 64)."""
    return arm + (want - arm) % 64


@functools.lru_cache(None)
def up_run_cases():
    """Per band six reads on one contig: the run's last row on n - 64 k - 1, n - 64 k, n - 64 k + 1 (t = 1, 0, -1 mod 64) and its first row
    on the same three (t + run - 1 = 1, 0, -1 mod 64).  The six agree, so the base is emitted.  The run is the longest the band holds
    from cell W - 3 with a few cells to spare: 56, 124 and 246 rows (an up step moves one band cell down, so no run exceeds W - 3 rows:
    over_long_up_run_part); at band 256 every read has a whole block of up steps, at band 128 at least five of the six."""
    out = []
    for W, run in ((64, 56), (128, 124), (256, 246)):
        arm = 3 * run
        seams = [(1, -1, 1), (1, 0, 0), (1, 1, -1), (0, -1, 2 - run), (0, 0, 1 - run), (0, 1, -run)]
        tails = [_tail_for(arm, t) for _, _, t in seams]
        part = up_run_part(W, run, tails)
        hl = arm + W
        st = [("up", 1 + x, run, arm + 1, arm + run, hl) for x in range(6)] + [("seam", 1 + x, which, d) for x, (which, d, _) in enumerate(seams)]
        # a whole block of up steps: block k holds the rows n - 64 k - 63 .. n - 64 k, the run the rows n - t - run + 1 .. n - t: certain from
        # 127 rows on, at band 128 a matter of where the seams fall
        whole = [x for x, t in enumerate(tails) if any(t <= 64 * k and 64 * k + 63 <= t + run - 1 for k in range(t // 64, t // 64 + 3))]
        assert len(whole) >= {64: 0, 128: 5, 256: 6}[W], whole
        st += [("block", 1 + x) for x in whole]
        out.append(assemble("up-band-%d-run-%d" % (W, run), [part], structure=st, loops=W == 64, stats=dict(voted=7, sum_dist=6 * run)))
    one = up_run_part(64, 40, [130])
    out.append(assemble("up-one-vote-of-two", [one], structure=[("up", 1, 40, 121, 160, 184)], stats=dict(voted=2)))
    return out


# ---- C: a long deletion and a long insertion in one read, inside batches that start off a multiple of four ---------------------------
def both_runs_case(W, c0, d, u):
    """contig = head + regionD + mid + tail, long read = head[W:] + mid + regionI + tail[:arm]: a left run of d cells from band cell c0,
    then an up run of u rows back to cell c0 + d - u.  Reads 3, 6 and 9 are the long read (strands 0, 1, 0) between pairs of short exact
    reads; the settings of polish_trace_bytes cut the batches at ra = 0, 1, 3, 4, 6, 7, 9 and at ra = 0, 1, 4, 7."""
    arm = 3 * max(d, u)
    head, mid, tail = _seq(11 * W, arm + W, last="G"), _seq(13 * W, arm, first="T", last="G"), _seq(17 * W, arm + W // 2 + u + 5, first="T")
    contig = head + _region(d) + mid + tail
    long_read = head[W:] + mid + _region(u) + tail[:arm]
    start, n = W + W // 2 - c0, 3 * arm + u
    hl = len(head)
    others, reads, st = [], {}, []
    for x in range(9):
        rid = 1 + x
        if rid in (3, 6, 9):
            strand = int(rid == 6)
            others.append((_stored(long_read, strand), start, strand))
            reads[rid] = (d + u, n, hl + d + 2 * arm, VOTED)
            st += [("left", rid, d, c0 + 1, c0 + d), ("up", rid, u, 2 * arm + 1, 2 * arm + u, hl + d + arm)]
        else:
            a = 40 + 23 * x
            others.append((_stored(contig[a:a + 25], x & 1), a, x & 1))
            reads[rid] = (0, 25, a + 25, VOTED)
    part = cs._case("both", S, [(contig, len(contig), 0)], others, band=W, max_diff=1.0, min_depth=1, reads=reads, seq=head + mid + "A" + tail,
                    gap={(hl + d + arm, CODE["A"]): 3}, col={(hl, 4): 3, (hl + d - 1, 4): 3}, counts=dict(deleted=d, inserted=1, voters=10))
    return assemble("both-runs-band-%d" % W, [part], structure=st, trace=[n * (W // 4), (n + 60) * (W // 4)], loops=W == 64, stats=dict(voted=10, sum_dist=3 * (d + u)))


def batch_starts(rows, W, nbytes):
    """The first read of every batch: consecutive reads whose rows fit nbytes of choices (W / 4 bytes per row), at least one read."""
    cap, out, ra = nbytes // (W // 4), [], 0
    while ra < len(rows):
        rb = ra
        while rb < len(rows) and sum(rows[ra:rb + 1]) <= cap:
            rb += 1
        rb = max(rb, ra + 1)
        if sum(rows[ra:rb]):
            out.append(ra)
        ra = rb
    return out


@functools.lru_cache(None)
def both_run_cases():
    """(at band 256 too large for polish_loops in a second: 1 400 rows of 256 cells; polish_tables alone)"""
    return [both_runs_case(64, 10, 30, 35), both_runs_case(256, 60, 100, 140)]


# ---- D: rings shorter than the band --------------------------------------------------------------------------------------------------
def short_ring_part(L, W):
    """A ring of four chain reads (prefixes L / 4, each reaching to the start of the next but one), the insertion x at gap 0 (between
    column L - 1 and column 0) in four reads that cross the origin: one longer than the ring (n = L), one at a negative start, one five
    columns before the origin and one on the reverse strand, which also carries a substitution that the others outvote; a fifth, exact
    read on the reverse strand ends below column 0, and a sixth starts at column 0: column 0 is then deeper than twice the four votes
    and column L - 1 is not, so the gap emits only if its left neighbour is taken round the origin.  A seventh, exact and on the reverse
    strand, is placed above L, at L + 2: it is anchored on the last chain read, which runs over the origin (part["via"])."""
    ring = next(g for g in (_seq(100 * x + L, L) for x in range(1, 50)) if g[0] != g[-1])
    rr = ring * 4
    pre = [L // 4 + (1 if i < L % 4 else 0) for i in range(4)]
    at = [sum(pre[:i]) for i in range(4)]
    chain = [(_stored(rr[at[i]:at[i] + pre[i] + pre[(i + 1) % 4] - 1], i & 1), pre[i], i & 1) for i in range(4)]
    x = cs._other(ring[-1], skip=ring[0])
    h = L // 2
    with_x = lambda a, n: rr[L + a:2 * L] + x + rr[2 * L:2 * L + n - (L - a) - 1]          # n bases from column a, x behind column L - 1
    longr = with_x(L - 7, L + 9)                                       # longer than the ring: its first L bases vote
    neg = with_x(L - h, L - 3)                                         # placed at L - h - L = -h
    above = with_x(L - 5, L - 6)
    rev = _sub(with_x(L - 9, L - 2), L - 8)                            # the substitution stands at column L - 9 + (L - 8) - 1 - L = L - 18
    others = [(longr, L - 7, 0), (neg, -h, 0), (above, L - 5, 0), (_stored(rev, 1), L - 9, 1), (_stored(rr[3:3 + L - 1], 1), 3 - L, 1), (rr[0:13], 0, 0), (_stored(rr[2:2 + h], 1), L + 2, 1)]
    part = cs._case("ring", C, chain, others, band=W, max_diff=0.25, min_depth=1, seq=x + ring, gap={(0, CODE[x]): 4}, counts=dict(inserted=1, deleted=0, substituted=0, voters=11),
                    reads={10: (0, L // 2, None, VOTED), 9: (0, 13, None, VOTED), 4: (1, L, None, VOTED), 5: (1, L - 3, None, VOTED), 6: (1, L - 6, None, VOTED), 7: (2, L - 2, None, VOTED), 8: (0, L - 1, None, VOTED)})
    part["via"] = {10: 3}
    return part


def short_ring_case(L, W):
    return assemble("ring-%d-band-%d" % (L, W), [short_ring_part(L, W)], structure=[("endj", 8, 3)], stats=dict(voted=11, rejected=0, sum_dist=5))


@functools.lru_cache(None)
def short_ring_cases():
    return [short_ring_case(L, W) for L in (33, 40, 64, 65, 127) for W in (64, 128, 256) if L < W]


# ---- E: slices clipped at the contig's ends, on both strands ------------------------------------------------------------------------
def clipped_part(kind, W=64):
    """Reads that hang over the start (i0 = 7 and 5), over the end, and over both (i0 = 6), each on its own strand or on both, lengths 33,
    35, 33, 37 and 114: the slice's first base is substituted (a diagonal step with a mismatch in row 1: column 0) and so is its last
    (in the last row the mismatch ties with an up step that ends one column earlier, and the smaller end wins: gap L - 1)."""
    g = _seq(77, 97)
    L = 97
    chain = [(g, L, 0)] if kind == S else [(g[0:41], 30, 0), (cu.revcomp(g[30:69]), 30, 1), (g[60:97], 37, 0)]
    nch = len(chain)
    x0, xl = cs._other(g[0]), cs._other(g[96], skip=g[95])
    junk = _seq(78, 40)
    a = junk[:7] + x0 + g[1:26]
    b = junk[7:12] + x0 + g[1:30]
    c = g[70:96] + xl + junk[12:18]
    d = g[70:96] + xl + junk[18:28]
    e = junk[28:34] + x0 + g[1:96] + xl + junk[29:40]
    others = [(_stored(a, 0), -7, 0), (_stored(b, 1), -5, 1), (_stored(c, 0), 70, 0), (_stored(d, 1), 70, 1), (_stored(e, 0), -6, 0), (_stored(e, 1), -6, 1)]
    assert [len(o[0]) for o in others] == [33, 35, 33, 37, 114, 114]
    reads = {nch: (1, 26, 26, VOTED), nch + 1: (1, 30, 30, VOTED), nch + 2: (1, 27, 96, VOTED), nch + 3: (1, 27, 96, VOTED), nch + 4: (2, 97, 96, VOTED), nch + 5: (2, 97, 96, VOTED)}
    return cs._case("clipped", kind, chain, others, band=W, max_diff=0.25, min_depth=1, reads=reads, col={(0, CODE[x0]): 4, (0, CODE[g[0]]): 1, (96, CODE[g[96]]): 1},
                    gap={(96, CODE[xl]): 4}, seq=x0 + g[1:96] + xl + g[96], counts=dict(substituted=1, inserted=1, deleted=0, voters=nch + 6))


@functools.lru_cache(None)
def clipped_cases():
    return [assemble("clipped-%s" % {S: "single", P: "path"}[k], [clipped_part(k)], stats=dict(voted=6 + (1 if k == S else 3), sum_dist=8)) for k in (P, S)]


# ---- G: the seams between contigs in the call and the write ---------------------------------------------------------------------------
def deleted_last_column_part(L=40, W=64):
    """A ring whose column L - 1 three reads across the origin lack: one base vote of the chain read against three deletions, the polished
    ring is one base shorter and its slot L - 1 emits nothing right before the next contig's slot 0.  (Only a ring can lose its last
    column: on a path the alignment's free end stops one column earlier instead of stepping left.)"""
    ring = next(g for g in (_seq(300 * x + L, L) for x in range(1, 50)) if g[0] != g[-1] and g[-2] != g[0])
    rr = ring * 4
    pre = [L // 4 + (1 if i < L % 4 else 0) for i in range(4)]
    at = [sum(pre[:i]) for i in range(4)]
    chain = [(_stored(rr[at[i]:at[i] + pre[i] + pre[(i + 1) % 4] - 1], i & 1), pre[i], i & 1) for i in range(4)]
    without = lambda a, n: rr[L + a:2 * L - 1] + rr[2 * L:2 * L + n - (L - a - 1)]          # n bases from column a, none for column L - 1
    others = [(without(L - 12, 25), L - 12, 0), (_stored(without(L - 9, 21), 1), L - 9, 1), (without(L - 15, 27), L - 15, 0)]
    return cs._case("ring-without-its-last-column", C, chain, others, band=W, max_diff=0.25, min_depth=1, seq=ring[:L - 1], col={(L - 1, 4): 3, (L - 1, CODE[ring[-1]]): 1},
                    reads={4: (1, 25, None, VOTED), 5: (1, 21, None, VOTED), 6: (1, 27, None, VOTED)}, counts=dict(deleted=1, inserted=0, substituted=0, voters=7))


@functools.lru_cache(None)
def seam_cases():
    """Six contigs in one call: a path whose gap L takes an agreed insertion (its slot L is the last before the ring's slot 0), a ring
    shorter than the band with an agreed insertion at its gap 0 (whose left neighbour is the ring's own column L - 1, not the path's gap
    L), a ring whose last column is deleted, a single-read contig with an agreed insertion at its gap 0 right behind it, a single-read
    contig whose only voter is its chain read, and the clipped single-read contig of group E.  seq_off is claimed for all of them."""
    g = _seq(91, 97)
    chain = [(g[0:41], 30, 0), (cu.revcomp(g[30:69]), 30, 1), (g[60:97], 37, 0)]
    xL = cs._other(g[96])
    path = cs._case("path", P, chain, [(g[67:97] + xL, 66, 0), (cu.revcomp(g[71:97] + xL), 70, 1)], band=64, max_diff=0.25, min_depth=1,
                    reads={3: (1, 31, 97, VOTED), 4: (1, 27, 97, VOTED)}, gap={(97, CODE[xL]): 2}, seq=g + xL, counts=dict(inserted=1, deleted=0, substituted=0, voters=5))
    f = _seq(93, 83)
    x0 = cs._other(f[0])
    front = cs._case("gap-0", S, [(f, 83, 0)], [(x0 + f[0:39], 0, 0), (cu.revcomp(x0 + f[0:29]), 0, 1)], band=64, max_diff=0.25, min_depth=1,
                     reads={1: (1, 40, 39, VOTED), 2: (1, 30, 29, VOTED)}, gap={(0, CODE[x0]): 2}, seq=x0 + f, counts=dict(inserted=1, deleted=0, substituted=0, voters=3))
    alone = _seq(92, 45)
    lone = cs._case("alone", S, [(alone, 45, 0)], [], band=64, max_diff=0.25, min_depth=1, reads={0: (0, 45, 45, VOTED)}, seq=alone, counts=dict(voters=1, inserted=0, deleted=0, substituted=0))
    parts = [path, short_ring_part(40, 64), deleted_last_column_part(), front, lone, clipped_part(S)]
    return [assemble("seams-path-ring-ring-single-single-single", parts, stats=dict(voted=5 + 11 + 7 + 3 + 1 + 7, rejected=0, outside=0))]


# ---- F: reads that do not vote among the voters ---------------------------------------------------------------------------------------
@functools.lru_cache(None)
def non_voter_cases():
    """The geometry of placement's clip-path case (a path of two chain reads; a read anchored by a zero-length pair at column L and one that
    ends at column 0 are OUTSIDE) with seven voters round them, and between those by read id two bad reads (skip_flags 1 takes them out)
    and a read without any pair: the row offsets of the voters' choices repeat across the non-voters, batches begin and end on them."""
    g, junk = _seq(55, 100), _seq(56, 40)
    chain = [(g[0:60], 40, 0), (g[40:100], 60, 0)]
    others = [(_sub(g[10:40], 7), 10, 0), (junk[0:10], 100, 0), (_stored(_sub(g[50:85], 3), 1), 50, 1), (junk[10:20], -10, 0), (g[20:55], 20, 0),
              (_stored(junk[20:25] + g[0:25], 1), -5, 1), (g[60:95], 60, 0), (g[5:30], 5, 0), (_stored(g[70:99], 1), 70, 1)]
    reads = {2: (1, 30, 40, VOTED), 3: (0, 0, 0, OUTSIDE), 4: (1, 35, 85, VOTED), 5: (0, 0, 0, OUTSIDE), 6: (0, 35, 55, VOTED), 7: (0, 25, 25, VOTED), 8: (0, 35, 95, VOTED),
             9: (0, 25, 30, VOTED), 10: (0, 29, 99, VOTED)}
    part = cs._case("path", P, chain, others, band=64, max_diff=0.25, min_depth=2, reads=reads, seq=g, counts=dict(voters=9, substituted=0, inserted=0, deleted=0))
    unplaced = [(3, g[3:23], ("bad", (0, 0), [(0, 2), (0, 4), (0, 6)])), (6, junk[25:40], "lone"), (8, g[30:52], ("bad", (0, 0), [(0, 7), (0, 8), (0, 9)]))]
    return [assemble("non-voters-among-voters", [part], unplaced, stats=dict(voted=9, rejected=0, outside=2, nreads=14, sum_dist=2), trace=[70 * 16, 1], cutoff=0.5)]


# ---- H: launch edges: slots and reads around one 256-lane block -------------------------------------------------------------------------
def slot_edge_case(X):
    """Two single-read contigs of 150 and X - 152 bases: X = bases + contigs slots, one lane each in k_po_call and k_po_write.  min_depth is
    2 and exact reads cover parts of each contig, so the columns outside them are low-depth: at X = 255, 256, 257 up to the last column
    (slot X - 2), at X = 320 also the slots 246 .. 265 on both sides of the block edge between lanes 255 and 256."""
    a, L1 = _seq(200 + X, 150), X - 152
    b = _seq(300 + X, L1)
    cover = [(10, 95), (115, L1 - 12)] if X > 300 else [(10, L1 - 12)]
    pa = cs._case("a", S, [(a, 150, 0)], [(a[20:120], 20, 0)], band=64, max_diff=0.25, min_depth=2, seq=a, counts=dict(voters=2, inserted=0, deleted=0, substituted=0))
    pb = cs._case("b", S, [(b, L1, 0)], [(_stored(b[lo:hi], x & 1), lo, x & 1) for x, (lo, hi) in enumerate(cover)], band=64, max_diff=0.25, min_depth=2, seq=b,
                  counts=dict(voters=1 + len(cover), inserted=0, deleted=0, substituted=0))
    low = 50 + L1 - sum(hi - lo for lo, hi in cover)
    return assemble("slots-%d" % X, [pa, pb], stats=dict(low_depth_columns=low, bases_before=X - 2, bases_after=X - 2, sum_dist=0))


def low_depth_slots(case, out):
    """The slots (contig offset + contig + column) of the columns below min_depth."""
    depth = out["col"].sum(axis=1)
    off = [int(x) for x in out["col_off"]]
    return [off[k] + k + c for k in range(len(off) - 1) for c in range(off[k + 1] - off[k]) if int(depth[off[k] + c]) < case["cin"]["min_depth"]]


def read_edge_case(M):
    """M reads, one lane each in k_po_plan and one wavefront each (four per workgroup) in k_po_align: the contig's own read, M - 4 exact
    reads of 12 .. 19 bases on both strands, and as the last three reads ones anchored at column L by a pair of no length: OUTSIDE,
    counted per wavefront on both sides of lane 255 / 256."""
    g, junk = _seq(400 + M, 150), _seq(500 + M, 40)
    others = []
    for x in range(M - 4):
        lo, l = (7 * x) % 130, 12 + x % 8
        others.append((_stored(g[lo:lo + l], x & 1), lo, x & 1))
    others += [(junk[10 * x:10 * x + 9 + x], 150, 0) for x in range(3)]
    reads = {M - 3: (0, 0, 0, OUTSIDE), M - 2: (0, 0, 0, OUTSIDE), M - 1: (0, 0, 0, OUTSIDE), M - 4: (0, 12 + (M - 5) % 8, None, VOTED)}
    part = cs._case("reads", S, [(g, 150, 0)], others, band=64, max_diff=0.25, min_depth=3, reads=reads, seq=g, counts=dict(voters=M - 3, inserted=0, deleted=0, substituted=0))
    return assemble("reads-%d" % M, [part], stats=dict(nreads=M, voted=M - 3, outside=3, rejected=0, sum_dist=0), trace=[1], loops=False)


@functools.lru_cache(None)
def launch_edge_cases():
    """(reads-M run through polish_tables alone: 250 reads in a dict per cell take polish_loops two seconds a case)"""
    return [slot_edge_case(X) for X in (255, 256, 257, 320)] + [read_edge_case(M) for M in (255, 256, 257)]


def over_long_up_run_part(W=128):
    """The construction of up_run_part with a region of W - 2 bases: from cell W - 3 there are W - 3 cells to step down through, one fewer
    than the run needs."""
    return assemble("up-run-longer-than-the-band", [up_run_part(W, W - 2, [3 * (W - 2)])], loops=False)


def all_cases():
    return left_run_cases() + up_run_cases() + both_run_cases() + short_ring_cases() + clipped_cases() + non_voter_cases() + seam_cases() + launch_edge_cases()
