"""-m gpu: read placements and contig depth on the GPU (elba_place_reads, place.hip) against the two restatements of placement_util.py, fed
with the GPU's own exports (contigs, read flags) and the pairs the graph was loaded from: record for record, segment for segment, count for
count.  The graphs come from placement_util.edges_of_chains (a string graph whose contigs are given chains) and from its ground-truth
layouts; off-chain reads are contained reads (their pairs carry the flag, the reduction prunes them) or reads whose pairs have no direction
(the reduction drops such entries).

ELBA_ERR_UNSUPPORTED is tested through read ids beyond 32 bit (a first_global_id of 2^32 under the context's own alignments).  Its other
conditions are not: a contig of 2^31 bases, 2^32 pairs and 4 x reads + contigs >= 2^32 need gigabytes of input and none fits a test of a
few seconds.  ELBA_ERR_STATE for missing pairs or reads cannot be reached by replacing them — every call that does drops the graph first —
but elba_dist_set_all_reads keeps the graph while it drops the context's alignments, or changes the replicated reads: both are tested."""
import ctypes as C

import numpy as np
import pytest

import contig_ex_util as cx
import contig_util as cu
import elba_amd
import placement_util as pu
from elba_amd import capi

pytestmark = pytest.mark.gpu

INVALID_ARG, STATE, UNSUPPORTED = 1, 5, 6                                   # ELBA_ERR_* of include/elba_amd.h

HAND = [c for c in pu.hand_cases() if not c["name"].startswith("skip-")]      # (the skip mask needs a bad read: its own test below)


def _packed(rng, lens):
    """Random reads of the given lengths in the 2-bit layout."""
    lens = np.asarray(lens, dtype=np.uint32)
    nb = (lens.astype(np.int64) + 3) // 4
    off = np.zeros(len(lens), dtype=np.uint64)
    off[1:] = np.cumsum(nb)[:-1].astype(np.uint64)
    packed = rng.integers(0, 256, int(nb.sum()) + 16).astype(np.uint8)
    packed[-16:] = 0
    return packed, off, lens


def _load(e, reads, pairs, cflags, cutoff=0.0):
    """set_reads + set_overlaps + transitive_reduction(cutoff, 0) + generate_contigs; returns the contig export."""
    packed, off, lens = reads
    e.set_reads(packed, off, lens)
    e.set_overlaps(len(lens), *pairs)
    e.transitive_reduction(cutoff, 0)
    e.generate_contigs(circular=bool(cflags & 1), singletons=bool(cflags & 2))
    return e.export_contigs()


def _check(e, pairs, lens, skip=1, loops=True, got=None, base=0):
    """The device's records, segments and counts are those of the restatements on the device's own contigs and read flags."""
    got = e.export_contigs() if got is None else got
    inp = pu.inputs_of_export(*pairs, got, e.export_read_flags(len(lens)), lens, skip, base)
    pl, st = e.place_reads(skip)
    assert pl["reads"].dtype == capi.PLACEMENT_DTYPE and st["ms_total"] > 0
    for f in ((pu.place_loops, pu.place_tables) if loops else (pu.place_tables,)):
        want, wst = f(inp)
        assert {k: st[k] for k in pu.STATS} == wst, (st, wst)
        assert pu.same_placements(pl, want), pu.first_difference(pl, want)
    for k in pu.GET_STATS:
        assert e.get_stat("place_" + k) == st[k]
    assert st["chain"] + st["anchored"] + st["unanchored"] + st["skipped"] + st["empty"] == st["nreads"] == len(lens)
    return pl, st, inp


def _case_pairs(case):
    """The case's chains as string-graph entries merged with its own pairs (a pair between two neighbours of a chain would be both)."""
    inp = case["inp"]
    pairs = dict(pu.edges_of_chains(inp["lens"], case["chains"], [int(k) for k in inp["kinds"]]))
    for q, t, o in zip(inp["rows"], inp["cols"], inp["vals"]):
        assert (int(q), int(t)) not in pairs
        pairs[(int(q), int(t))] = o
    return cu.upper(pairs)


@pytest.mark.parametrize("case", HAND, ids=[c["name"] for c in HAND])
def test_hand_cases(case):
    """Orientation (all eight of anchor strand x rc x Q / T, with hand-computed starts), clipping at both ends, reads outside, a read longer
    than its contig, a chain read over the end, wraps, a negative start modulo L, len >= L, ties and scores."""
    rng = np.random.default_rng(7)
    lens = case["inp"]["lens"]
    pairs = _case_pairs(case)
    e = elba_amd.Engine(17, 2, 8)
    got = _load(e, _packed(rng, lens), pairs, case["cflags"])
    chains = [[(int(got["chain_read"][i]), int(got["chain_prefix"][i]), int(got["chain_strand"][i])) for i in range(int(a), int(b))]
              for a, b in zip(got["chain_off"][:-1], got["chain_off"][1:])]
    assert chains == case["chains"] and (e.export_read_flags(len(lens)) == case["inp"]["read_flags"]).all()
    pl, st, _ = _check(e, pairs, lens, got=got)
    for r, want in case["reads"].items():
        p = pl["reads"][r]
        assert (int(p["contig"]), int(p["start"]), int(p["strand"]), int(p["kind"]), int(p["flags"]), int(p["anchor"])) == tuple(want), (r, p, want)
    for k, v in case["stats"].items():
        assert st[k] == v, (k, st[k], v)
    L = pu.contig_lens(case["inp"])
    for c, d in case["depth"].items():
        assert pu.depth_of(pl, c, int(L[c])).tolist() == list(d)
    for c, (nr, nb) in case["credited"].items():
        assert (int(pl["credited_reads"][c]), int(pl["credited_bases"][c])) == (nr, nb)
    e.close()


def _star(rng, nchain, ncand, M):
    """A path of `nchain` reads in the middle of the ids and one off-chain read x between them with `ncand` candidates (chain reads on both
    sides of x, so that x is Q of some and T of others), all of one score; the other reads have no pair.  Returns (lens, pairs dict, x,
    chain ids, chain)."""
    lens = rng.integers(30, 60, M)
    x = M // 2
    ids = [i for i in range(M) if i != x]
    lo = [i for i in ids if i < x][-(nchain // 2):]
    chain = sorted(lo + [i for i in ids if i > x][:nchain - len(lo)])
    ch = [(r, int(rng.integers(1, lens[r])), int(rng.integers(0, 2))) for r in chain]
    ch[-1] = (ch[-1][0], int(lens[ch[-1][0]]), ch[-1][2])
    pairs = dict(pu.edges_of_chains(lens, [ch], [cx.PATH]))
    for y in chain[:ncand]:
        bx, by = int(rng.integers(0, 10)), int(rng.integers(0, 10))
        iv = (bx, bx + 20, by, by + 20) if x < y else (by, by + 20, bx, bx + 20)
        pairs[(min(x, y), max(x, y))] = pu.pair(*iv, rc=int(rng.integers(0, 2)), score=5, **{"containedQ" if x < y else "containedT": 1})
    return lens, pairs, x, chain, ch


@pytest.mark.parametrize("ncand", [0, 1, 2, 65, 300])
def test_equal_scores_the_smallest_index_wins(ncand):
    """A read with 0, 1, 2, 65 and 300 candidates of one score: its anchor is the first of them in the input list, whichever lane got there
    first; with candidates on both sides the tie is between pairs where x is Q and pairs where it is T."""
    rng = np.random.default_rng(ncand)
    M = 340
    lens, pairs, x, chain, ch = _star(rng, 320, ncand, M)
    pairs = cu.upper(pairs)
    e = elba_amd.Engine(17, 2, 8)
    _load(e, _packed(rng, lens), pairs, 0)
    pl, st, inp = _check(e, pairs, lens)
    assert st["candidates"] == ncand and st["chain"] == 320 and st["anchored"] == (ncand > 0) and st["unanchored"] == M - 320 - (ncand > 0)
    if ncand:
        first = min(a for a in range(len(pairs[0])) if x in (int(pairs[0][a]), int(pairs[1][a])) and int(pairs[2][a]["containedQ"]) + int(pairs[2][a]["containedT"]))
        y = int(pairs[0][first]) if int(pairs[1][first]) == x else int(pairs[1][first])
        assert int(pl["reads"][x]["anchor"]) == y and (ncand < 2 or y < x)
    e.close()


def test_a_tie_between_q_and_t_and_a_negative_score_beside_zero():
    """x = read 2 is T of the pair with read 0 and Q of the pair with read 3, same score: pair (0, 2) comes first in the list.  Read 5 has a
    candidate of score -4 (list index smaller) and one of score 0: both count as 0, the negative one wins and its score is reported; read 6
    has a candidate of score 1 behind one of score -9: the positive one wins."""
    rng = np.random.default_rng(3)
    lens = [50, 50, 30, 50, 50, 30, 30]
    ch = [(0, 40, 0), (1, 40, 1), (3, 40, 0), (4, 50, 1)]
    pairs = dict(pu.edges_of_chains(lens, [ch], [cx.PATH]))
    pairs[(0, 2)] = pu.pair(10, 30, 0, 20, score=6, containedT=1); pairs[(2, 3)] = pu.pair(0, 20, 5, 25, score=6, containedQ=1)
    pairs[(1, 5)] = pu.pair(0, 20, 0, 20, score=-4, containedT=1); pairs[(3, 5)] = pu.pair(0, 20, 0, 20, score=0, containedT=1)
    pairs[(1, 6)] = pu.pair(0, 20, 0, 20, score=-9, containedT=1); pairs[(4, 6)] = pu.pair(0, 20, 0, 20, rc=1, score=1, containedT=1)
    pairs = cu.upper(pairs)
    e = elba_amd.Engine(17, 2, 8)
    _load(e, _packed(rng, lens), pairs, 0)
    pl, st, _ = _check(e, pairs, lens)
    r = pl["reads"]
    assert (int(r[2]["anchor"]), int(r[2]["start"]), int(r[2]["score"])) == (0, 10, 6)
    assert (int(r[5]["anchor"]), int(r[5]["score"]), int(r[5]["start"])) == (1, -4, 40 + 30 - 10)   # strand(1) = 1, rc 0: ob_y = 50 - 20, ob_x = 30 - 20
    assert (int(r[6]["anchor"]), int(r[6]["score"]), int(r[6]["strand"])) == (4, 1, 0)
    e.close()


@pytest.mark.parametrize("M", [63, 64, 65])
def test_reads_and_pairs_around_one_wavefront(M):
    """63, 64 and 65 reads with as many pairs: a path of 20 reads (19 entries) and M - 19 candidates spread over the other reads."""
    rng = np.random.default_rng(M)
    lens = rng.integers(30, 60, M)
    chain = sorted(int(x) for x in rng.permutation(M)[:20])
    ch = [(r, int(rng.integers(1, lens[r])), int(rng.integers(0, 2))) for r in chain]
    ch[-1] = (ch[-1][0], int(lens[ch[-1][0]]), ch[-1][2])
    pairs = dict(pu.edges_of_chains(lens, [ch], [cx.PATH]))
    others = [r for r in range(M) if r not in chain]
    while len(pairs) < M:
        x, y = int(rng.choice(others)), int(rng.choice(chain))
        b = [int(v) for v in rng.integers(0, 10, 2)]
        iv = (b[0], b[0] + 20, b[1], b[1] + 20)
        pairs[(min(x, y), max(x, y))] = pu.pair(*iv, rc=int(rng.integers(0, 2)), score=int(rng.integers(-2, 30)), **{"containedQ" if x < y else "containedT": 1})
    pairs = cu.upper(pairs)
    assert len(pairs[0]) == M
    e = elba_amd.Engine(17, 2, 8)
    _load(e, _packed(rng, lens), pairs, 0)
    pl, st, _ = _check(e, pairs, lens)
    assert st["candidates"] == M - 19 and st["anchored"] > 10
    e.close()


def test_contig_kinds_and_the_calls_without_flags():
    """A ring of 6 reads with two contained reads, a path of 3 with one, and 4 lone reads.  Without flags the ring's reads are in no contig
    and the reads that overlap only them are unanchored; with CIRCULAR they are placed; with SINGLETONS the lone reads are contigs of one
    read, and a read contained in one is anchored on it."""
    rng = np.random.default_rng(11)
    lens = [40] * 6 + [40] * 3 + [30] * 4 + [12] * 4                      # ring 0-5, path 6-8, lone 9-12, contained 13-16
    ring = [(0, 20, 0), (1, 20, 1), (2, 20, 0), (3, 20, 0), (4, 20, 1), (5, 20, 0)]
    path = [(6, 25, 1), (7, 25, 0), (8, 40, 0)]
    pairs = dict(pu.edges_of_chains(lens, [ring, path], [cx.CIRCLE, cx.PATH]))
    pairs[(1, 13)] = pu.pair(5, 17, 0, 12, score=12, containedT=1); pairs[(5, 14)] = pu.pair(15, 27, 0, 12, rc=1, score=12, containedT=1)      # 14 wraps, as read 5 does: 100 + 15 + 12 > 120
    pairs[(7, 15)] = pu.pair(0, 12, 0, 12, score=12, containedT=1); pairs[(10, 16)] = pu.pair(3, 15, 0, 12, rc=1, score=12, containedT=1)
    pairs = cu.upper(pairs)
    e = elba_amd.Engine(17, 2, 8)
    reads = _packed(rng, lens)
    want = {0: dict(chain=3, anchored=1, unanchored=13), 1: dict(chain=9, anchored=3, unanchored=5, wrapped=2), 2: dict(chain=7, anchored=2, unanchored=8),
            3: dict(chain=13, anchored=4, unanchored=0, wrapped=2)}
    for cflags in (0, 1, 2, 3):
        got = _load(e, reads, pairs, cflags)
        pl, st, _ = _check(e, pairs, lens, got=got)
        for k, v in want[cflags].items():
            assert st[k] == v, (cflags, k, st[k], v)
        if not cflags & 1:
            assert (pl["reads"]["contig"][:6] == -1).all() and (pl["reads"]["kind"][[13, 14]] == pu.NONE).all()
        if cflags & 2:
            k = int(pl["reads"][10]["contig"])
            assert int(got["kinds"][k]) == cx.SINGLE and (int(pl["reads"][16]["contig"]), int(pl["reads"][16]["start"]), int(pl["reads"][16]["strand"])) == (k, 3, 1)
            assert (int(pl["credited_reads"][k]), int(pl["credited_bases"][k])) == (2, 42)
    e.close()


def test_the_skip_mask():
    """Read 4 is bad (one pair passed out of four: (1 + 1) / (4 + 1) <= 0.5; its entries are pruned before contained reads are looked for,
    so that is its only flag); read 5 is contained.  skip_flags 0 anchors both, 1 (the default) skips the bad one, 2 the contained one, 255
    both."""
    rng = np.random.default_rng(5)
    lens = [60, 60, 60, 60, 20, 20]
    ch = [(0, 30, 0), (1, 30, 0), (2, 30, 1), (3, 60, 0)]
    pairs = dict(pu.edges_of_chains(lens, [ch], [cx.PATH]))
    pairs[(0, 4)] = pu.pair(10, 30, 0, 20, score=20, containedT=1)
    for y in (1, 2, 3):
        pairs[(y, 4)] = pu.pair(0, 20, 0, 20, score=50, passed=0)
    pairs[(2, 5)] = pu.pair(5, 25, 0, 20, rc=1, score=20, containedT=1)
    pairs = cu.upper(pairs)
    e = elba_amd.Engine(17, 2, 8)
    got = _load(e, _packed(rng, lens), pairs, 0, cutoff=0.5)
    assert e.export_read_flags(6).tolist() == [0, 0, 0, 0, 1, 2] and got["n"] == 1
    for skip, anchored, skipped in ((0, 2, 0), (1, 1, 1), (255, 0, 2), (2, 1, 1), (4, 2, 0)):
        pl, st, _ = _check(e, pairs, lens, skip=skip, got=got)
        assert (st["anchored"], st["skipped"], st["candidates"]) == (anchored, skipped, anchored)
    pl, st = e.place_reads()                                     # the default is 1
    assert st["skipped"] == 1 and (int(pl["reads"][4]["kind"]), int(pl["reads"][5]["kind"]), int(pl["reads"][5]["start"])) == (pu.NONE, pu.ANCHORED, 60 + 35)
    e.close()


def test_after_cleaning_removed_reads_anchor_on_the_path_that_stayed():
    """A path of 24 reads with a tip of two reads at read 6 and a bubble between reads 12 and 16 whose second arm has one read.  After
    clip_tips + pop_bubbles the path is one contig; the tip's first read and the popped arm anchor on it through the entries they had (the
    graph's input still holds them), the tip's second read reaches no chain read and stays unanchored."""
    rng = np.random.default_rng(21)
    M = 27
    lens = rng.integers(40, 80, M)
    ids = rng.permutation(M)
    main, tip, arm = [int(x) for x in ids[:24]], [int(x) for x in ids[24:26]], int(ids[26])
    edges = {}

    def add(u, v):
        i, j = min(u, v), max(u, v)
        o = cu.edge(rng, int(lens[i]), int(lens[j]))
        o["begQ"], o["endQ"], o["begT"], o["endT"], o["score"], o["rc"] = int(rng.integers(0, 5)), int(lens[i]) - 3, 2, int(lens[j]) - int(rng.integers(0, 5)), int(rng.integers(1, 50)), int(rng.integers(0, 2))
        edges[(i, j)] = o

    for u, v in zip(main[:-1], main[1:]):
        add(u, v)
    add(main[6], tip[0]); add(tip[0], tip[1])
    add(main[12], arm); add(arm, main[16])
    pairs = cu.upper(edges)
    e = elba_amd.Engine(17, 2, 8)
    packed, off, lens = _packed(rng, lens)
    e.set_reads(packed, off, lens)
    e.set_overlaps(M, *pairs)
    e.transitive_reduction(0.0, 0)
    assert e.export_string_graph()["n"] == 2 * len(edges)
    t, b = e.clip_tips(4, 4), e.pop_bubbles(8, 4)
    assert t["reads_removed"] == 2 and b["reads_removed"] == 1
    e.generate_contigs(circular=True, singletons=True)
    flags = e.export_read_flags(M)
    assert flags[tip[0]] == 4 and flags[tip[1]] == 4 and flags[arm] == 8
    pl, st, _ = _check(e, pairs, lens)
    assert st["chain"] == 24 and st["anchored"] == 2 and st["unanchored"] == 1 and e.export_contigs()["n"] == 1
    assert int(pl["reads"][tip[0]]["anchor"]) == main[6] and int(pl["reads"][arm]["anchor"]) in (main[12], main[16]) and int(pl["reads"][tip[1]]["kind"]) == pu.NONE
    assert st["skipped"] == 0 and e.place_reads(4)[1]["skipped"] == 2 and e.place_reads(8)[1]["skipped"] == 1
    e.close()


def _pile(nleft, nright):
    """A path contig of 2000 bases (reads 0 and 1 of 1000); `nleft` reads of 100 bases end at 900, `nright` begin there."""
    M = 2 + nleft + nright
    lens = np.full(M, 100); lens[:2] = 1000
    pairs = dict(pu.edges_of_chains(lens, [[(0, 1000, 0), (1, 1000, 0)]], [cx.PATH]))
    for x in range(2, M):
        b = 800 if x < 2 + nleft else 900
        pairs[(0, x)] = pu.pair(b, b + 100, 0, 100, score=100, containedT=1)
    return lens, cu.upper(pairs)


@pytest.mark.parametrize("nright", [2999, 3000, 3001])
def test_three_thousand_reads_end_where_as_many_start(nright):
    """The depth at 900 falls by one, stays, or rises by one: with 3000 ends and 3000 starts in one group of keys no segment begins there."""
    rng = np.random.default_rng(nright)
    lens, pairs = _pile(3000, nright)
    e = elba_amd.Engine(17, 2, 8)
    _load(e, _packed(rng, lens), pairs, 0)
    pl, st, _ = _check(e, pairs, lens, loops=False)
    assert pl["seg_start"].tolist() == ([0, 800, 1000] if nright == 3000 else [0, 800, 900, 1000])
    assert pl["seg_depth"].tolist() == ([1, 3001, 1] if nright == 3000 else [1, 3001, nright + 1, 1]) and st["max_depth"] == max(3001, nright + 1)
    assert int(pl["credited_reads"][0]) == 2 + 3000 + nright and int(pl["credited_bases"][0]) == 2000 + 100 * (3000 + nright)
    e.close()


@pytest.mark.parametrize("n", [255, 256, 257, 511, 513])
def test_credited_intervals_around_the_block_edge(n):
    """n crediting reads on a circle (4 chain reads, the rest contained, every third of them wrapping: two intervals each), then the same
    count with some reads outside on a path: interval slots and endpoint keys on both sides of a 256-lane block."""
    rng = np.random.default_rng(n)
    lens = np.full(n, 30); lens[:4] = 60
    ring = [(0, 50, 0), (1, 50, 1), (2, 50, 0), (3, 50, 1)]
    pairs = dict(pu.edges_of_chains(lens, [ring], [cx.CIRCLE]))
    for x in range(4, n):
        y = 3 if x % 3 == 0 else int(rng.integers(0, 3))
        by = int(rng.integers(0, 5)) if y == 3 else int(rng.integers(0, 20))          # read 3 starts at 150 of 200 and is reversed: its first bases lie over the origin
        pairs[(y, x)] = pu.pair(by, by + 30, 0, 30, rc=int(rng.integers(0, 2)), score=30, containedT=1)
    pairs = cu.upper(pairs)
    e = elba_amd.Engine(17, 2, 8)
    reads = _packed(rng, lens)
    _load(e, reads, pairs, 1)
    pl, st, _ = _check(e, pairs, lens)
    assert st["anchored"] == n - 4 and st["wrapped"] >= (n - 4) // 3 and int(pl["credited_reads"][0]) == n
    path = [(0, 50, 0), (1, 50, 1), (2, 50, 0), (3, 60, 1)]
    pairs = dict(pu.edges_of_chains(lens, [path], [cx.PATH]))
    for x in range(4, n):
        y = int(rng.integers(0, 4))
        bx = int(rng.integers(0, 31))
        pairs[(y, x)] = pu.pair(0, 0, bx, bx, score=0, containedT=1) if x % 5 == 0 else pu.pair(10, 40, 0, 30, score=30, containedT=1)      # (empty intervals: the read hangs over the start of read y)
    pairs = cu.upper(pairs)
    _load(e, reads, pairs, 0)
    pl, st, _ = _check(e, pairs, lens)
    assert st["anchored"] == n - 4 and st["clipped"] > 0 and int(pl["credited_reads"][0]) == n - st["outside"]
    e.close()


@pytest.mark.parametrize("nsingle,long_len,bits", [(0, (1 << 20) + 77, 23), (65537, (1 << 15) + 5, 34), (65537, (1 << 20) + 77, 39)])
def test_sort_keys_of_about_22_34_and_40_bits(nsingle, long_len, bits):
    """One contig of more than 2^20 bases (two reads); 65 537 single-read contigs beside one of more than 2^15 bases; and beside the long
    one.  The endpoint keys take 1 + position bits + contig bits."""
    rng = np.random.default_rng(bits)
    ncont = 300
    M = nsingle + 2 + ncont
    a, b = nsingle // 2, nsingle // 2 + 1                          # the long contig's reads, in the middle of the ids
    lens = rng.integers(4, 25, M)
    half = long_len // 2
    lens[a], lens[b] = half + 100, long_len - half
    contained = np.arange(M - ncont, M)
    lens[contained] = 20
    pairs = dict(pu.edges_of_chains(lens, [[(a, half, 0), (b, long_len - half, 1)]], [cx.PATH]))
    for x in contained:
        y = int(rng.choice([a, b])) if nsingle == 0 or x % 2 else int(rng.integers(0, a))
        by = int(rng.integers(0, lens[y] - 19)) if y in (a, b) else 0
        n = 20 if y in (a, b) else int(min(20, lens[y]))
        pairs[(y, int(x))] = pu.pair(by, by + n, 0, n, rc=int(rng.integers(0, 2)), score=n, containedT=1)
    pairs = cu.upper(pairs)
    e = elba_amd.Engine(17, 2, 8)
    got = _load(e, _packed(rng, lens), pairs, 2)
    assert got["n"] == nsingle + 1 and int(np.diff(got["seq_off"]).max()) == long_len
    nc, pb = got["n"], int(long_len).bit_length()
    assert 1 + pb + max(1, int(nc).bit_length()) == bits
    pl, st, _ = _check(e, pairs, lens, got=got)
    assert st["anchored"] == ncont and st["chain"] == nsingle + 2 and st["unanchored"] == 0
    k = int(pl["reads"][a]["contig"])
    assert pu.depth_of(pl, k, long_len).min() >= 1 and int(pl["credited_reads"][k]) >= 2
    e.close()


def test_one_context_over_changing_sizes_repeats_and_leaves_the_pileup_alone():
    rng = np.random.default_rng(8)
    e = elba_amd.Engine(17, 2, 8)
    for seed, glen, nchain, circular, ncont, nextra in ((1, 900, 12, False, 15, 6), (4, 6000, 60, True, 400, 30), (3, 700, 5, False, 0, 0), (5, 1500, 20, False, 30, 12)):
        t = pu.truth_set(np.random.default_rng(seed), glen, nchain, circular, ncont, nextra)
        packed, off, lens = cu.pack(t["seqs"])
        e.set_reads(packed, off, lens)
        e.set_overlaps(len(lens), *t["pairs"])
        e.read_pileup(mode=0, margin=0, min_depth=1, min_run=1, trim_len=0)
        before = e.export_pileup()
        e.transitive_reduction(0.0, 0)
        assert e.export_string_graph()["n"] == 2 * len(t["edges"])             # the pairs without a direction are gone, the contained reads too
        e.generate_contigs(circular=True)
        assert (e.export_read_flags(len(lens)) == t["read_flags"]).all()
        pl, st, _ = _check(e, t["pairs"], lens)
        assert st["chain"] == nchain and st["anchored"] == ncont + nextra
        got = e.export_contigs()
        contig, L = got["seqs"][0], glen
        assert got["n"] == 1 and len(contig) == glen
        for r, p in enumerate(pl["reads"]):                      # every read reads like the contig where it was placed
            s, start = pu.oriented(t["seqs"][r], int(p["strand"])), int(p["start"])
            assert s == ((contig * 3)[start % L:start % L + len(s)] if circular else contig[start:start + len(s)]), r
        for _ in range(2):
            again, st2 = e.place_reads()
            assert pu.same_placements(again, pl) and {k: st2[k] for k in pu.STATS} == {k: st[k] for k in pu.STATS}
            assert again["reads"].tobytes() == pl["reads"].tobytes()
        after = e.export_pileup()
        assert all(np.array_equal(before[k], after[k]) for k in before if k != "n") and before["n"] == after["n"]
        e.release_workspace()
        again, _ = e.place_reads()
        assert pu.same_placements(again, pl)
    e.close()


def test_errors():
    rng = np.random.default_rng(2)
    case = next(c for c in pu.hand_cases() if c["name"] == "ties")
    lens = case["inp"]["lens"]
    rows, cols, vals = _case_pairs(case)
    e = elba_amd.Engine(17, 2, 8)
    reads = _packed(rng, lens)
    e.set_reads(*reads)
    e.set_overlaps(len(lens), rows, cols, vals)
    e.transitive_reduction(0.0, 0)
    with pytest.raises(elba_amd.ElbaError) as err:               # no contigs yet
        e.place_reads()
    assert err.value.status == STATE and e.get_stat("place_chain") == 0
    e.generate_contigs()
    pl, st = e.place_reads()
    assert e.get_stat("place_chain") == 4 == st["chain"]
    for bad in (dict(reserved=(1, 0, 0)), dict(reserved=(0, 0, 7)), dict(skip_flags=256), dict(skip_flags=-1)):
        with pytest.raises(elba_amd.ElbaError) as err:
            e.place_reads(**bad)
        assert err.value.status == INVALID_ARG and e.get_stat("place_chain") == 0      # nothing of the failed call is left
    o, s = capi.Placements(), capi.PlaceStats()
    assert e.L.elba_place_reads(e.h, None, C.byref(o), C.byref(s)) == INVALID_ARG and not o.reads
    assert e.L.elba_place_reads(e.h, C.byref(capi.PlaceCfg(1)), None, C.byref(s)) == INVALID_ARG
    e.place_reads()
    e.clip_tips(2, 1)                                            # the contigs are gone: the counts read 0, the call is out of order
    assert e.get_stat("place_chain") == 0 and e.get_stat("place_segments") == 0
    with pytest.raises(elba_amd.ElbaError) as err:
        e.place_reads()
    assert err.value.status == STATE
    with pytest.raises(elba_amd.ElbaError):
        e.get_stat("place_nothing")
    # intervals: the smallest bad CANDIDATE is named; pairs that are no candidates are not looked at
    keys = list(zip(rows.tolist(), cols.tolist()))
    for (q, t), field, value in (((0, 4), "endQ", 51), ((1, 4), "begT", -1), ((1, 5), "begT", 21), ((2, 5), "endT", 21)):
        v = vals.copy()
        a = keys.index((q, t))
        v[field][a] = value
        v["endT"][keys.index((2, 5))] = 21                       # a second bad candidate behind it
        v["endQ"][keys.index((6, 7))] = 1000; v["begT"][keys.index((3, 6))] = -7      # off-off and not passed: no candidates
        e.set_overlaps(len(lens), rows, cols, v)
        e.transitive_reduction(0.0, 0)
        e.generate_contigs()
        with pytest.raises(elba_amd.ElbaError) as err:
            e.place_reads()
        assert err.value.status == INVALID_ARG and "pair %d (%d, %d)" % (a, q, t) in str(err.value) and e.get_stat("place_chain") == 0
        with pytest.raises(pu.BadInterval) as want:
            pu.place_tables(pu.inputs_of_export(rows, cols, v, e.export_contigs(), e.export_read_flags(len(lens)), lens))
        assert want.value.pair == a
    e.close()


def _replicate(e, packed, off, lens, n):
    """elba_dist_set_all_reads with the first n reads (the call copies them: the device arrays are freed again).  Device memory comes from
    the HIP runtime the library is linked to, looked up through its handle as capi._copy_from_device does."""
    L = e.L
    L.hipMalloc.restype = C.c_int; L.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    L.hipMemcpy.restype = C.c_int; L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    L.hipFree.restype = C.c_int; L.hipFree.argtypes = [C.c_void_p]
    L.elba_dist_set_all_reads.restype = C.c_int
    L.elba_dist_set_all_reads.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64]
    dev = []
    for a in (np.ascontiguousarray(packed, dtype=np.uint8), np.ascontiguousarray(off, dtype=np.uint64), np.ascontiguousarray(lens, dtype=np.uint32)):
        p = C.c_void_p()
        assert L.hipMalloc(C.byref(p), max(a.nbytes, 16)) == 0 and L.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0      # 1: host to device
        dev.append(p)
    try:
        e._check(L.elba_dist_set_all_reads(e.h, dev[0], len(packed) - 16, dev[1], dev[2], n))
    finally:
        for p in dev:
            L.hipFree(p)


@pytest.mark.parametrize("error_rate,base", [(0.0, 0), (0.01, 0), (0.0, 1000)])
def test_end_to_end(error_rate, base):
    """Synthetic reads of a 30 kb genome through the whole pipeline (k-mers, overlaps, alignment, reduction, cleaning, contigs): the
    placements are those of the restatement on the device's own alignments, contigs and flags.  Without errors every placed read also
    reads like its contig over its credited part.  With a first_global_id of 1000 the exported pairs, the chain reads and the anchors carry
    it, the records stay one per local read.  At the end the context's alignments are dropped under the graph (elba_dist_set_all_reads
    does that): the pairs are missing, ELBA_ERR_STATE."""
    packed, off, lens, info = elba_amd.synth_reads(77, 30000, 14, 2500, 400, error_rate=error_rate)
    M = len(lens)
    e = elba_amd.Engine(17, 2, 30)
    e.set_reads(packed, off, lens, first_global_id=base)
    e.count_kmers(); e.create_kmer_matrix(); e.create_seed_matrix()
    e.align_seeds()
    ov = e.export_overlaps()
    e.transitive_reduction(0.65, 1000)
    e.simplify_graph(4, 8)
    e.generate_contigs(circular=True, singletons=True)
    pairs = (ov["rows"], ov["cols"], ov["vals"])
    assert int(ov["rows"].min()) >= base and int(ov["cols"].max()) < base + M
    pl, st, inp = _check(e, pairs, lens, base=base)
    placed = pl["reads"]["kind"] != pu.NONE
    assert (pl["reads"]["anchor"] >= base).all() and (pl["reads"]["anchor"][~placed] == np.arange(M)[~placed] + base).all()
    assert st["chain"] > 0 and st["anchored"] > st["chain"] and st["anchored"] + st["chain"] > 0.9 * M       # most reads are off the chains and find a place
    got = e.export_contigs()
    L = np.diff(got["seq_off"])
    for c in range(got["n"]):
        if int(got["kinds"][c]) != cx.CIRCLE and L[c]:
            assert pu.depth_of(pl, c, int(L[c])).min() >= 1     # chain reads tile a path contig
    if error_rate == 0.0:
        seqs = cu.seqs_of(packed, off, lens)
        for r, p in enumerate(pl["reads"]):
            if not int(p["kind"]):
                continue
            c, start = int(p["contig"]), int(p["start"])
            s, contig = pu.oriented(seqs[r], int(p["strand"])), got["seqs"][c]
            if int(got["kinds"][c]) == cx.CIRCLE:
                n = min(len(s), len(contig))
                assert s[:n] == (contig * 3)[start % len(contig):start % len(contig) + n], r
            else:
                lo, hi = max(start, 0), min(start + len(s), len(contig))
                assert s[max(lo - start, 0):max(hi - start, 0)] == contig[lo:max(hi, lo)], r
    _replicate(e, packed, off, lens, M)                          # the alignments go, S and its contigs stay
    assert e.get_stat("contig_count") == got["n"]
    with pytest.raises(elba_amd.ElbaError) as err:
        e.place_reads()
    assert err.value.status == STATE and "no overlaps" in str(err.value) and e.get_stat("place_chain") == 0
    e.close()


def test_replicated_reads_serve_the_lengths_and_are_missed_when_they_change():
    """A context that holds a shard of the reads places from the replicated set (elba_dist_set_all_reads); once that set holds other reads
    the graph's reads are on the context no more: ELBA_ERR_STATE, the graph and its contigs still valid."""
    t = pu.truth_set(np.random.default_rng(5), 1500, 20, False, 30, 12)
    packed, off, lens = cu.pack(t["seqs"])
    M = len(lens)
    e = elba_amd.Engine(17, 2, 8)
    e.set_reads(*cu.pack(t["seqs"][:3]))
    _replicate(e, packed, off, lens, M)
    e.set_overlaps(M, *t["pairs"])
    e.transitive_reduction(0.0, 0)
    e.generate_contigs(circular=True)
    pl, st, _ = _check(e, t["pairs"], lens)
    assert st["chain"] == 20 and st["anchored"] == 42
    _replicate(e, *cu.pack(t["seqs"][:3]), 3)
    assert e.get_stat("contig_count") == 1
    with pytest.raises(elba_amd.ElbaError) as err:
        e.place_reads()
    assert err.value.status == STATE and "reads" in str(err.value) and e.get_stat("place_chain") == 0
    e.close()


def test_read_ids_beyond_32_bit_are_unsupported():
    """The context's own alignments under a first_global_id of 2^32: the graph and its contigs carry 64-bit ids, the placement's anchors are
    32-bit.  ELBA_ERR_UNSUPPORTED, *out zeroed, the counters read 0; the same reads at id 0 are placed."""
    packed, off, lens, info = elba_amd.synth_reads(78, 20000, 12, 2500, 400, error_rate=0.0)
    e = elba_amd.Engine(17, 2, 30)
    for base in (0, 1 << 32, (1 << 32) - len(lens) - 2):
        e.set_reads(packed, off, lens, first_global_id=base)
        e.count_kmers(); e.create_kmer_matrix(); e.create_seed_matrix()
        e.align_seeds()
        e.transitive_reduction(0.65, 1000)
        e.generate_contigs(circular=True, singletons=True)
        got = e.export_contigs()
        assert got["n"] > 0 and int(got["chain_read"].min()) >= base
        if base != 1 << 32:                                      # (the last is the largest base that fits: ids up to 2^32 - 3)
            pl, st = e.place_reads()
            assert st["chain"] == len(got["chain_read"]) == e.get_stat("place_chain") and base <= int(pl["reads"]["anchor"].min()) and int(pl["reads"]["anchor"].max()) <= base + len(lens) - 1
            continue
        with pytest.raises(elba_amd.ElbaError) as err:
            e.place_reads()
        assert err.value.status == UNSUPPORTED and "32 bit" in str(err.value)
        o, s = capi.Placements(), capi.PlaceStats()
        o.nreads, o.reads = 7, 8                                 # (stale values: the call zeroes them)
        assert e.L.elba_place_reads(e.h, C.byref(capi.PlaceCfg(1)), C.byref(o), C.byref(s)) == UNSUPPORTED
        assert o.nreads == 0 and o.ncontigs == 0 and not (o.reads or o.seg_off or o.seg_start or o.seg_depth or o.credited_reads or o.credited_bases)
        for k in pu.GET_STATS:
            assert e.get_stat("place_" + k) == 0
    e.close()
