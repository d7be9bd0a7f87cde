"""Inputs that take the late stages past their second size boundary: a grid capped at a multiple of the CU count, whose lanes then walk a
grid-stride loop, and a two-level sum whose second level is a fixed number of lanes.  Plain numpy, no device; every builder takes the CU
count `cus` as a parameter (the library reads it from the device properties, the GPU tests from torch).

  placement_pairs   k_pl_candidates (place.hip): 16 x cus workgroups of 256 lanes, so T = 16 * cus * 256 pairs fill one trip
  links_graph       k_gl_links<0> / k_gl_sum (graph_links.hip): one partial per count-pass workgroup of 256 columns, added up by 256 lanes
                    in four wavefronts, 256 partials a trip
  fasta_text, fastq_text   the line and record kernels of text_index.hip: 8 x cus workgroups of 256 lanes over lines or records

What a test may claim about an input is computed here from the construction (which pair was given the best score, how many structures
of which kind went into which workgroup's columns, which record was broken), never from a restatement of the rule."""
import numpy as np

import contig_ex_util as cx
import contig_util as cu
import gfa_util as gu
import placement_util as pu
import text_index_util as tx
from oracle import pyoracle as po


# ---- placement ---------------------------------------------------------------------------------------------------------------------------
def placement_trip(cus):
    """Pairs that one trip of k_pl_candidates' grid takes."""
    return 16 * int(cus) * 256


EDGE, CAND, LAST, CHAIN_CHAIN, OFF_OFF = range(5)                # what a pair of the list is
ROLES = ("last", "best_above", "best_below", "tie", "t_then_q", "third_trip")


def _build_pairs(cus, extra, ring, bad, seed):
    rng = np.random.default_rng(seed)
    T = placement_trip(cus)
    n = T + int(extra)
    noff = 1000 if n >= 200000 else 60
    npool = 12
    nchain = -(-11 * n // (10 * (noff - 1))) + 8                 # about 10 % more chain x off pairs than the list needs
    M = nchain + noff
    # ids: read 0 and read M - 2 are chain reads, read M - 1 is off the chain; the others are mixed
    off_ids = np.sort(np.concatenate([1 + rng.choice(M - 3, noff - 1, replace=False), [M - 1]])).astype(np.int64)
    is_off = np.zeros(M, dtype=bool); is_off[off_ids] = True
    chain_ids = np.flatnonzero(~is_off).astype(np.int64)
    assert len(chain_ids) == nchain and not is_off[0] and not is_off[M - 2]
    lens = rng.integers(30, 60, M).astype(np.int64)
    ring_ids = np.sort(rng.choice(chain_ids[1:-1], 24, replace=False)) if ring else np.zeros(0, np.int64)
    path_ids = chain_ids[~np.isin(chain_ids, ring_ids)]

    def chain_of(ids, closed):
        ch = [(int(r), int(rng.integers(1, lens[r])), int(rng.integers(0, 2))) for r in ids]
        if not closed:
            ch[-1] = (ch[-1][0], int(lens[ch[-1][0]]), ch[-1][2])
        return ch
    chains, kinds = [chain_of(path_ids, False)], [cx.PATH]
    if ring:                                                     # contigs come out by ascending start read
        chains.append(chain_of(ring_ids, True)); kinds.append(cx.CIRCLE)
    er, ec, ev = cu.upper(pu.edges_of_chains(lens, chains, kinds))
    # every chain read with every off-chain read but the last one, which meets read M - 2 alone
    X = off_ids[:-1]
    pool = X[-npool:]                                            # the designated reads: large ids, so their pairs lie all over the list
    yy, xx = np.repeat(chain_ids, len(X)), np.tile(X, nchain)
    ncc = noo = 200 if n >= 200000 else 20
    a, b = rng.choice(chain_ids, ncc), rng.choice(chain_ids, ncc)
    cc = np.unique(np.stack([np.minimum(a, b), np.maximum(a, b)], axis=1)[a != b], axis=0)
    edge_keys = set(zip(er.tolist(), ec.tolist()))
    cc = np.array([p for p in cc.tolist() if tuple(p) not in edge_keys], dtype=np.int64).reshape(-1, 2)
    a, b = rng.choice(X, noo), rng.choice(X, noo)
    oo = np.unique(np.stack([np.minimum(a, b), np.maximum(a, b)], axis=1)[a != b], axis=0).astype(np.int64)
    fixed = len(er) + 1 + len(cc) + len(oo)
    drop = fixed + len(yy) - n
    removable = np.flatnonzero(~np.isin(xx, pool))
    assert 0 <= drop <= len(removable) // 2, (drop, len(removable))
    keep = np.ones(len(yy), dtype=bool); keep[rng.choice(removable, drop, replace=False)] = False
    yy, xx = yy[keep], xx[keep]
    q = np.concatenate([er, np.minimum(yy, xx), [M - 2], cc[:, 0], oo[:, 0]])
    t = np.concatenate([ec, np.maximum(yy, xx), [M - 1], cc[:, 1], oo[:, 1]])
    what = np.concatenate([np.full(len(er), EDGE), np.full(len(yy), CAND), [LAST], np.full(len(cc), CHAIN_CHAIN), np.full(len(oo), OFF_OFF)])
    src = np.concatenate([np.arange(len(er)), np.full(n - len(er), -1)])      # where an edge's entry comes from
    order = np.lexsort((t, q))
    q, t, what, src = q[order], t[order], what[order], src[order]
    assert len(q) == n and ((q[1:] > q[:-1]) | ((q[1:] == q[:-1]) & (t[1:] > t[:-1]))).all() and (q < t).all()
    if any(what[i] != CAND for i in bad):
        return None
    vals = np.zeros(n, dtype=po.OVERLAP_DTYPE)
    bq, bt = rng.integers(0, 10, n), rng.integers(0, 10, n)
    vals["begQ"], vals["endQ"], vals["begT"], vals["endT"] = bq, bq + 20, bt, bt + 20
    vals["rc"] = rng.integers(0, 2, n); vals["score"] = rng.integers(-2, 31, n); vals["passed"] = 1
    vals["direction"] = -1; vals["directionT"] = -1
    x = np.where(is_off[q], q, t)                                # (of a candidate: its off-chain read)
    cand = (what == CAND) | (what == LAST)
    vals["containedQ"] = cand & (x == q); vals["containedT"] = cand & (x == t)
    vals[what == EDGE] = ev[src[what == EDGE]]
    idx_cc = np.flatnonzero(what == CHAIN_CHAIN)
    vals["passed"][idx_cc[::2]] = 0                              # chain - chain: half did not pass, half have no direction
    plain = np.flatnonzero((what == CAND) & ~np.isin(x, pool))
    plain = plain[~np.isin(plain, list(bad))]
    vals["passed"][rng.choice(plain, len(plain) // 32, replace=False)] = 0      # chain - off pairs that did not pass
    assert (np.bincount(x[cand & (vals["passed"] != 0)], minlength=M)[off_ids] > 0).all()      # every off-chain read stays contained
    # the designated reads
    anchors, index = {"last": (M - 1, M - 2)}, {"last": n - 1}
    assert what[n - 1] == LAST
    free = list(pool[::-1])
    other = lambda a: int(t[a] if q[a] == x[a] else q[a])

    def plant(role, winner, losers, tied=()):
        r = int(x[winner])
        mine = np.flatnonzero(cand & (x == r))
        vals["score"][mine] = rng.integers(-2, 31, len(mine))
        vals["score"][winner] = 90
        vals["score"][list(tied)] = 90
        vals["score"][list(losers)] = 80
        anchors[role] = (r, other(winner)); index[role] = int(winner)

    def candidates_of(r):
        ci = np.flatnonzero(cand & (x == r))
        return ci[ci < T], ci[(ci >= T) & (ci < 2 * T)], ci[ci >= 2 * T]
    for role in ("third_trip", "t_then_q", "best_above", "best_below", "tie"):      # (the scarcest candidates first: few reads reach the third trip)
        for r in free:
            lo, hi, hi2 = candidates_of(r)
            if role == "best_above" and len(lo) and len(hi):
                plant(role, hi[len(hi) // 2], [lo[len(lo) // 3]])
            elif role == "best_below" and len(lo) and len(hi):
                plant(role, lo[2 * len(lo) // 3], [hi[0], hi[-1]])
            elif role == "tie" and len(lo) > 1 and len(hi):
                plant(role, lo[len(lo) // 2], [], tied=[lo[-1], hi[0], hi[-1]])
            elif role == "t_then_q" and len(lo) and (q[lo] != r).any() and ((q[hi] == r).any() or (q[hi2] == r).any()):
                asq = np.concatenate([hi[q[hi] == r], hi2[q[hi2] == r]])
                plant(role, asq[0], [lo[q[lo] != r][-1]])
            elif role == "third_trip" and len(lo) and len(hi) and len(hi2):
                plant(role, hi2[len(hi2) // 2], [lo[0], hi[-1]])
            else:
                continue
            free.remove(r)
            break
    for i in bad:
        vals["endQ"][i] = lens[q[i]] + 1
    return dict(cus=int(cus), T=T, n=n, M=M, lens=lens, pairs=(q, t, vals), chains=chains, kinds=kinds, cflags=cx.CIRCULAR if ring else 0,
                off=off_ids, nchain=nchain, candidates=int((cand & (vals["passed"] != 0)).sum()), anchors=anchors, index=index, what=what,
                bad=min(bad) if bad else None)


def placement_pairs(cus, extra, ring=False, bad=(), seed=0):
    """T + extra pairs over one path chain (ring: and a circle of 24 reads) and about a thousand contained off-chain reads (60 below
    200 000 pairs).  The list holds the chains' own entries, every chain read with nearly every off-chain read (one in 32 of them did
    not pass), chain - chain pairs that did not pass or have no direction, and off - off pairs; only the chain - off pairs that passed
    are candidates, `candidates` of them.  anchors = {role: (read, its anchor)} and index = {role: the winning pair} for the designated
    reads, as far as the list reaches: `last` (read M - 1, whose only pair is the last of the list); `best_above` (score 90 in the
    second trip, 80 in the first); `best_below` (the reverse); `tie` (90 twice in the first trip and twice in the second: the smallest
    index wins); `t_then_q` (the read is T of an 80 in the first trip and Q of the 90 behind it); `third_trip` (90 at an index >= 2 T).
    bad: candidate indices whose Q interval ends one base behind the read; `bad` of the result is the one to be named.  The first seed
    from `seed` on at which all of `bad` are chain - off pairs is taken."""
    for s in range(seed, seed + 64):
        out = _build_pairs(cus, extra, ring, tuple(int(i) for i in bad), s)
        if out is not None:
            return out
    raise AssertionError("no seed puts candidates at %r" % (bad,))


def placement_input(case):
    """The `inp` of placement_util's restatements from the construction alone (the chains as built, the off-chain reads contained)."""
    rf = np.zeros(case["M"], dtype=np.uint8); rf[case["off"]] = pu.CONTAINED
    return pu.inputs_of_chains(case["lens"], case["chains"], case["kinds"], *case["pairs"], rf, 1)


# ---- links -------------------------------------------------------------------------------------------------------------------------------
LINK_COUNTERS = ("candidates", "links", "closures", "twisted", "unplaced", "clamped", "asymmetric")
PER_COPY = {3: dict(candidates=12, links=11, closures=1, twisted=1, unplaced=0, clamped=1, asymmetric=1),      # under CIRCULAR | SINGLETONS
            1: dict(candidates=12, links=0, closures=1, twisted=0, unplaced=12, clamped=0, asymmetric=0)}      # under CIRCULAR: no branch read has a contig
COPY_READS = 26


def _copy_edges(rng):
    """One copy of every structure, as (labels, {(i, j): entry}) lists.  Reads have 20 bases and a step takes a prefix of 12.  A Y of three
    two-read paths at a branch (3 links, any direction code); the same with one path's last read carried the other way (2 links and a
    twisted edge); a star with an entry whose two directions disagree (3 links, 1 asymmetric); a star with a prefix beyond its read (3
    links, 1 clamped); a ring of four (1 closure).  Without SINGLETONS the branch and lone reads are in no contig: 12 unplaced candidates."""
    E = lambda d, p=12, dT=None: gu.E(d, p, 12, dT)
    d = int(rng.integers(0, 4))
    inner = 1 - (d >> 1)
    return [(7, {(0, 1): E(inner), (2, 3): E(inner), (4, 5): E(inner), (1, 6): E(d), (3, 6): E(d), (5, 6): E(d)}),
            (7, {(0, 1): E(1), (2, 3): E(1), (4, 5): E(1), (1, 6): E(2), (3, 6): E(1), (5, 6): E(1)}),
            (4, {(0, 1): E(1, dT=0), (0, 2): E(1), (0, 3): E(1)}),
            (4, {(0, 1): E(1, p=30), (0, 2): E(1), (0, 3): E(1)}),
            (4, {(0, 1): E(1), (1, 2): E(1), (2, 3): E(1), (0, 3): E(2)})]


def links_graph(nb, hot_blocks, seed=0):
    """M = 256 nb - 1 reads of 4 .. 24 bases: the count pass of elba_export_assembly_links runs exactly nb workgroups.  Every read is
    alone but for those of the workgroups in hot_blocks: the j-th of them (ascending) holds j + 1 copies of every structure of
    _copy_edges, all of a structure's reads among the workgroup's columns 256 b .. 256 b + 254, so every record and every count of it
    lands in that workgroup's partial.  content = {block: copies}; expected[flags] = the counters under contig flags 3 and 1."""
    rng = np.random.default_rng(seed + 1000 * nb + sum(hot_blocks))
    hot = sorted(set(int(b) for b in hot_blocks))
    assert hot and 0 <= hot[0] and hot[-1] < nb and COPY_READS * len(hot) <= 255
    M = 256 * nb - 1
    lens = rng.integers(4, 25, M).astype(np.int64)
    edges, content = {}, {}
    for j, b in enumerate(hot):
        content[b] = j + 1
        ids = 256 * b + rng.permutation(255)[:COPY_READS * (j + 1)]
        lens[ids] = 20
        at = 0
        for _ in range(j + 1):
            for k, es in _copy_edges(rng):
                mine = np.sort(ids[at:at + k]); at += k
                for (i, jj), o in es.items():
                    edges[(int(mine[i]), int(mine[jj]))] = o
    expected = {f: {k: v * sum(content.values()) for k, v in PER_COPY[f].items()} for f in PER_COPY}
    return dict(nb=nb, M=M, lens=lens, pairs=cu.upper(edges), content=content, expected=expected)


def links_cases():
    """(nb, hot_blocks): each of {0}, {63}, {64}, {255}, {256}, {nb - 1} alone and all of them together, wherever the index is below nb."""
    out = []
    for nb in (64, 65, 256, 257, 600):
        single = sorted({b for b in (0, 63, 64, 255, 256, nb - 1) if b < nb})
        out += [(nb, (b,)) for b in single] + [(nb, tuple(single))]
    return out


# ---- text --------------------------------------------------------------------------------------------------------------------------------
def text_trip(cus):
    """Lines or records that one trip of a line / record kernel's grid takes."""
    return 8 * int(cus) * 256


def _seqs(rng, R, lo, hi):
    n = rng.integers(lo, hi + 1, R)
    n[[0, 5, R // 2, R - 3]] = 0                                 # empty reads, one of them in the second trip
    n[R - 1] = max(int(n[R - 1]), 2)
    al = np.frombuffer(b"ACGTacgtNn", dtype=np.uint8)
    flat = al[rng.integers(0, len(al), int(n.sum()))].tobytes()
    off = np.concatenate([[0], np.cumsum(n)])
    return [flat[int(off[i]):int(off[i + 1])] for i in range(R)]


def _name(i):
    return b"r%d d" % i if i % 5 == 0 else b"r%d" % i


def _fasta_record(i, s, width):
    if width <= 0 or not s:
        return b">" + _name(i) + b"\n" + s + b"\n"
    return b">" + _name(i) + b"\n" + b"".join(s[a:a + width] + b"\n" for a in range(0, len(s), width))


def _fastq_record(i, s):
    return b"@" + _name(i) + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n"


def _joined(chunks, final_newline):
    data = b"".join(chunks)
    return data if final_newline else data[:-1]


def fasta_text(cus, multi=False, final_newline=True, broken=(), seed=0):
    """R = 8 * cus * 256 + 3 FASTA records (a line and a record more than one trip of every kernel that walks them; the header flags run
    over lines + 1 elements).  multi: sequences of 4 .. 9 bases in lines of 3, so 2 - 3 sequence lines per record and headers in the
    second trip of the line kernels; else one line of 0 .. 8 bases.  Some reads are empty.  broken: records whose last sequence line is
    made longer than their first, a SHAPE violation at that line; error = (kind, file offset, record) of the one to be named."""
    rng = np.random.default_rng(seed)
    R = text_trip(cus) + 3
    seqs = _seqs(rng, R, 4 if multi else 0, 9 if multi else 8)
    chunks = [_fasta_record(i, s, 3 if multi else 0) for i, s in enumerate(seqs)]
    error = None
    for r in sorted(broken, reverse=True):
        chunks[r] = b">" + _name(r) + b"\nAC\nACG\n"
        at = sum(len(c) for c in chunks[:r]) + len(_name(r)) + 2 + 3
        error = (tx.SHAPE, at, r)
    return dict(data=_joined(chunks, final_newline), R=R, fmt="fasta", error=error)


def fastq_text(cus, final_newline=True, broken=(), seed=0):
    """R FASTQ records of 0 .. 8 bases.  broken: records whose quality line is one byte long, an FQ_QUAL violation at the record's '@'."""
    rng = np.random.default_rng(seed + 1)
    R = text_trip(cus) + 3
    seqs = _seqs(rng, R, 0, 8)
    chunks = [_fastq_record(i, s) for i, s in enumerate(seqs)]
    error = None
    for r in sorted(broken, reverse=True):
        chunks[r] = chunks[r][:-1] + b"I\n"
        error = (tx.FQ_QUAL, sum(len(c) for c in chunks[:r]), r)
    return dict(data=_joined(chunks, final_newline), R=R, fmt="fastq", error=error)
