"""-m gpu: elba_pop_bubbles (elba_amd/csrc/bubbles.hip) against the restatement of its rule in bubble_util.py: every entry of the popped S
in order, every field, the read flags and the stats, exactly.  Graphs are loaded with elba_set_overlaps with suffixes the reduction does
not remove at fuzz 0 (every suffix in [5, 9]: a two-edge walk is at least 10), which each test asserts from the exported S first."""
import ctypes as C
import functools

import numpy as np
import pytest

import bubble_util as bu
import contig_util as cu
import elba_amd
import rounds_util as ru
import string_graph_util as sg
import tip_util as tu
from elba_amd import capi
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

CASES = bu.hand_cases()


SG_TILE, SG_THREADS, SCAN_TILE = ru.SG_TILE, ru.SG_THREADS, ru.SCAN_TILE                 # read from sg_rounds.hpp and prims.hip


def _same_S(g, rows, cols, vals):
    assert g["n"] == len(rows) and (g["rows"] == rows).all() and (g["cols"] == cols).all()
    assert g["vals"].tobytes() == np.asarray(vals).tobytes()


def _load(e, M, rows, cols, vals, cutoff=0.0, fuzz=0, kept=True):
    e.set_overlaps(M, rows, cols, vals)
    s = e.transitive_reduction(cutoff, fuzz)
    if kept:
        assert s["nnz"] == 2 * len(rows)                        # the reduction keeps the graph as built
    return s


def _pop(e, M, mx, rounds=1):
    """pop_bubbles on the engine's S equals the restatement on the S exported before the call.  Returns (stats, restatement's result)."""
    g = e.export_string_graph()
    f0 = e.export_read_flags(M)
    want = bu.pop_bubbles(M, g["rows"], g["cols"], g["vals"], mx, rounds)
    st = e.pop_bubbles(mx, rounds)
    for k in bu.STATS:
        assert st[k] == want[4][k], (k, st, want[4])
    assert st["ms_total"] >= 0 and st["ms_compact"] >= 0
    _same_S(e.export_string_graph(), want[0], want[1], want[2])
    assert (e.export_read_flags(M) == (f0 | want[3])).all()
    return st, want


@pytest.fixture(scope="module")
def eng():
    e = elba_amd.Engine(17, 2, 8)
    yield e
    e.close()


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_rule_one_clause_per_case(eng, name):
    case = CASES[name]
    M, rows, cols, vals = tu.case_overlaps(case, np.random.default_rng(3), extra_reads=2)      # two isolated reads behind the graph
    _load(eng, M, rows, cols, vals)
    st, want = _pop(eng, M, case["max"], case["rounds"])
    flags = eng.export_read_flags(M)
    assert set(np.flatnonzero(flags == 8).tolist()) == case["removed"] and st["rounds_run"] == case["rounds_run"]
    assert st["reads_removed"] == len(case["removed"]) and flags.sum() == 8 * len(case["removed"])
    after = np.bincount(eng.export_string_graph()["cols"], minlength=M)
    for v, d in case["deg_after"].items():
        assert after[v] == d


@pytest.mark.parametrize("name", ["tip_on_an_arm", "bubble_inside_a_dead_end_chain"])
def test_simplify_graph_alternates_the_two_calls(eng, name):
    case = CASES[name]
    M, rows, cols, vals = tu.case_overlaps(case, np.random.default_rng(4), extra_reads=2)
    _load(eng, M, rows, cols, vals)
    g = eng.export_string_graph()
    want = bu.simplify(M, g["rows"], g["cols"], g["vals"], case["max_tip"], case["max"])
    got = eng.simplify_graph(case["max_tip"], case["max"])
    assert len(got) == len(want[4]) == 2
    for (t, b), (wt, wb) in zip(got, want[4]):
        assert all(t[k] == wt[k] for k in tu.STATS) and all(b[k] == wb[k] for k in bu.STATS)
    _same_S(eng.export_string_graph(), want[0], want[1], want[2])
    flags = eng.export_read_flags(M)
    assert (flags == want[3]).all() and {int(v): int(flags[v]) for v in np.flatnonzero(flags)} == case["removed_simplify"]
    _load(eng, M, rows, cols, vals)
    assert len(eng.simplify_graph(case["max_tip"], case["max"], passes=1)) == 1                # `passes` bounds it


def test_cycle_with_one_bubble_becomes_a_circular_contig():
    g = tu.Graph()
    cyc = g.chain(g.new(8), closed=True)
    extra = bu.between(g, cyc[1], cyc[4], 1)                     # beside cyc[2], cyc[3]
    rng = np.random.default_rng(4)
    M, rows, cols, vals = g.overlaps(rng)
    packed, off, lens = cu.random_packed(rng, M, 20, 40)
    e = elba_amd.Engine(17, 2, 8)
    e.set_reads(packed, off, lens)
    _load(e, M, rows, cols, vals)
    st0 = e.generate_contigs(circular=True)
    assert st0["cycles"] == 0 and st0["branches"] == 2 and st0["contigs"] == 2 and (e.export_contigs()["kinds"] == 1).sum() == 0
    st, _ = _pop(e, M, 2)
    assert st["bubbles"] == 1 and e.export_read_flags(M)[extra[0]] == 8
    with pytest.raises(elba_amd.ElbaError) as err:              # the contigs of the unpopped graph are gone
        e.export_contigs()
    assert err.value.status == 5
    st1 = e.generate_contigs(circular=True)
    got = e.export_contigs()
    assert st1["cycles"] == 1 and got["n"] == 1 and got["kinds"].tolist() == [1] and st1["contig_reads"] == 8
    e.close()


def test_flags_of_bad_contained_and_clipped_reads_stay_beside_popped_ones(eng):
    """A contained read and a bad read hang on the losing arm's read in the input (the prunes take them), a tip hangs on the bubble's
    anchor: after clip_tips and pop_bubbles every read carries its own flag."""
    g = tu.Graph()
    a, b, ch = bu._bubble(g, [1, 2])
    tip = g.arm(a, 1)[0]
    x = ch[0][0]
    rng = np.random.default_rng(5)
    M, rows, cols, vals = g.overlaps(rng, M=g.n + 3)
    iso, w, z = g.n, g.n + 1, g.n + 2
    edges = {(int(r), int(c)): v for r, c, v in zip(rows, cols, vals)}
    edges[(x, w)] = cu.edge(rng, 20, 20); edges[(x, w)]["containedT"] = 1
    edges[(x, z)] = cu.edge(rng, 20, 20); edges[(x, z)]["passed"] = 0
    r2, c2, v2 = cu.upper(edges)
    s = _load(eng, M, r2, c2, v2, cutoff=0.5, kept=False)
    assert s["nnz"] == 2 * len(rows) and s["bad_reads"] == 1 and s["contained_reads"] == 1
    f0 = eng.export_read_flags(M)
    assert f0[z] == 1 and f0[w] == 2 and f0[iso] == 0 and f0[x] == 0
    st, _ = _pop(eng, M, 3)
    assert st["reads_removed"] == 1 and st["anchors"] == 2
    assert eng.clip_tips(1)["reads_removed"] == 1                # a second call of the other kind goes on from there
    f = eng.export_read_flags(M)
    assert f[x] == 8 and f[tip] == 4 and f[z] == 1 and f[w] == 2 and f[iso] == 0 and f.sum() == 15
    st, _ = _pop(eng, M, 3)
    assert st["reads_removed"] == 0 and (eng.export_read_flags(M) == f).all()


def _hub_pair(n_arms):
    g = tu.Graph()
    a, b, ch = bu._bubble(g, [1] * n_arms)
    return g, a, b, ch


@pytest.mark.parametrize("n", [255, 256, 257, 3000])
def test_one_pair_of_anchors_with_many_one_read_arms(eng, n):
    """The pick looks through a column of n + 1 entries for every one of its n arms: across wavefronts and workgroups."""
    g, a, b, ch = _hub_pair(n)
    M, rows, cols, vals = g.overlaps(np.random.default_rng(n))
    _load(eng, M, rows, cols, vals)
    st, _ = _pop(eng, M, 1, 2)
    assert st["arms"] == n and st["bubbles"] == 1 and st["arms_removed"] == n - 1 and st["reads_removed"] == n - 1 and st["rounds_run"] == 2      # (in round 2 the two are no anchors)
    flags = eng.export_read_flags(M)
    assert flags[ch[0][0]] == 0 and (flags[[c[0] for c in ch[1:]]] == 8).all()                 # the arm with the smallest first read stays
    assert st["nnz_after"] == st["nnz_before"] - 4 * (n - 1)


@pytest.mark.parametrize("mx,gone", [(999, 0), (1000, 1), (65535, 1)])
def test_an_arm_of_1000_reads_beside_a_one_read_arm(eng, mx, gone):
    g = tu.Graph()
    a, b, ch = bu._bubble(g, [1000, 1])
    M, rows, cols, vals = g.overlaps(np.random.default_rng(11), perm=np.random.default_rng(12).permutation(g.n))
    _load(eng, M, rows, cols, vals)
    st, _ = _pop(eng, M, mx)
    assert st["reads_removed"] == gone and st["arms"] == 1 + gone and st["bubbles"] == gone and st["anchors"] == 2


@pytest.mark.parametrize("M", [1, 64, 65, 65537])
def test_read_counts_at_wavefront_and_block_edges(eng, M):
    z = np.zeros(0, dtype=po.OVERLAP_DTYPE)
    if M == 1:
        _load(eng, 1, np.zeros(0, np.int64), np.zeros(0, np.int64), z)
        st, _ = _pop(eng, 1, 3, 2)
        assert st["nnz_before"] == 0 and st["rounds_run"] == 1
        return
    g = tu.Graph()
    a, b, ch = bu._bubble(g, [1, 2])
    x = ch[0][0]
    rest = [v for v in range(g.n) if v not in (a, x)]
    perm = np.zeros(g.n, dtype=np.int64)
    perm[a], perm[x] = 0, M - 1
    perm[rest] = np.arange(M - 1 - len(rest), M - 1)            # the graph's other reads next to the last one, isolated reads between
    Mx, rows, cols, vals = g.overlaps(np.random.default_rng(M), perm=perm, M=M)
    _load(eng, M, rows, cols, vals)
    st, _ = _pop(eng, M, 2)
    assert eng.export_read_flags(M)[M - 1] == 8 and st["reads_removed"] == 1


@pytest.mark.parametrize("nnz", [SG_TILE - 2, SG_TILE - 1, SG_TILE, SG_TILE + 1, SG_TILE + 2, SCAN_TILE - 2, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, SCAN_TILE + 2,
                                 2 * SCAN_TILE - 2, 2 * SCAN_TILE - 1, 2 * SCAN_TILE, 2 * SCAN_TILE + 1, 2 * SCAN_TILE + 2])
def test_nnz_at_the_block_sizes_of_scan_and_compaction(eng, nnz):
    """nnz(S) round SG_TILE (= SG_THREADS: k_sg_scatter's tile, the flat kernels' workgroup) and the scan's SCAN_TILE.  The scan and
    k_sg_keep run over nnz + 1 elements, so nnz = tile - 1 gives them exactly a tile.  An odd nnz comes from one pair whose directionT is -1:
    the reduction keeps one image of it, a column of one entry whose row has an empty column."""
    assert SG_TILE == 256 and SG_THREADS == 256 and SCAN_TILE == 2048
    odd = nnz % 2
    g = tu.Graph()
    a, b, ch = bu._bubble(g, [1, 2], tails=(5, (nnz - odd) // 2 - 10))
    perm = np.random.default_rng(nnz + 1).permutation(g.n + 2 * odd)
    M, rows, cols, vals = g.overlaps(np.random.default_rng(nnz), perm=perm, M=g.n + 2 * odd)
    if odd:
        x, y = sorted((int(perm[g.n]), int(perm[g.n + 1])))
        edges = {(int(r), int(c)): v for r, c, v in zip(rows, cols, vals)}
        edges[(x, y)] = cu.edge(np.random.default_rng(nnz), 20, 20, directionT=-1)
        rows, cols, vals = cu.upper(edges)
    s = _load(eng, M, rows, cols, vals, kept=False)
    assert s["nnz"] == nnz
    if odd:
        S = eng.export_string_graph()
        assert ((S["rows"] == x) & (S["cols"] == y)).sum() == 1 and ((S["rows"] == y) & (S["cols"] == x)).sum() == 0
    st, _ = _pop(eng, M, 2, 3)
    assert st["reads_removed"] == 1 and st["nnz_after"] == nnz - 4 and st["rounds_run"] == 2 and st["anchors"] == 2 and st["bubbles"] == 1


@functools.lru_cache(maxsize=None)
def _layout_with_bubbles(seed, M, nbubbles):
    """The layout graph of the string graph's scale tests with nbubbles pairs of reads the prunes keep, 40 reads apart, each joined by two
    chains of new reads of different lengths (1 to 3): whatever the reduction leaves between the two, the two chains are a bubble."""
    rng = np.random.default_rng(seed)
    rows, cols, vals = sg.layout_overlaps(rng, M, 8)
    deg, flags = sg.kept_degrees(M, rows, cols, vals, 0.65)
    ok = np.flatnonzero((flags[:-40] == 0) & (deg[:-40] > 0) & (flags[40:] == 0) & (deg[40:] > 0))
    u = np.sort(rng.choice(ok, nbubbles, replace=False))
    pairs = [(int(x), int(x) + 40) for x in u for _ in range(2)]
    lengths = np.array([[1, 2], [1, 3], [2, 3]])[rng.integers(0, 3, nbubbles)].reshape(-1)
    M2, r2, c2, v2, planted = bu.plant_bubbles(rng, M, rows, cols, vals, pairs, lengths)
    return M2, r2, c2, v2, planted, lengths


def test_empty_graph_and_context_without_reads(eng):
    z = np.zeros(0, dtype=po.OVERLAP_DTYPE)
    for M in (5, 0):
        _load(eng, M, np.zeros(0, np.int64), np.zeros(0, np.int64), z)
        st, _ = _pop(eng, M, 3, 4)
        assert st["nnz_after"] == 0 and st["reads_removed"] == 0 and st["rounds_run"] == 1 and st["nreads"] == M and st["anchors"] == 0
        assert eng.export_string_graph()["n"] == 0


def test_one_context_over_graphs_of_changing_size():
    e = elba_amd.Engine(17, 2, 8)
    z = np.zeros(0, dtype=po.OVERLAP_DTYPE)
    big = _layout_with_bubbles(1, 40000, 500)
    small = tu.case_overlaps(CASES["three_arms_1_2_3"], np.random.default_rng(1))
    for M, rows, cols, vals, kept, fuzz in ((big[0], big[1], big[2], big[3], False, 1000), small + (True, 0), (7, np.zeros(0, np.int64), np.zeros(0, np.int64), z, True, 0),
                                            (big[0], big[1], big[2], big[3], False, 1000)):
        _load(e, M, rows, cols, vals, cutoff=0.65 if not kept else 0.0, fuzz=fuzz, kept=kept)
        st, _ = _pop(e, M, 3, 2)
        if M == big[0]:
            assert st["bubbles"] >= 250 and st["reads_removed"] >= 250
    # a second call on the popped graph goes on from there: after rounds to the end, nothing is left to remove
    _pop(e, big[0], 3, 64)
    st, _ = _pop(e, big[0], 3, 64)
    assert st["reads_removed"] == 0 and st["rounds_run"] == 1 and st["nnz_after"] == st["nnz_before"]
    e.close()


def test_errors_leave_S_flags_and_contigs_untouched():
    e = elba_amd.Engine(17, 2, 8)
    L = e.L
    cfg = capi.BubbleCfg(3, 1, (C.c_int32 * 2)(0, 0))
    st = capi.BubbleStats()
    assert L.elba_pop_bubbles(e.h, C.byref(cfg), C.byref(st)) == 5                    # no S
    rng = np.random.default_rng(2)
    M, rows, cols, vals = tu.case_overlaps(CASES["three_arms_1_2_3"], rng)
    packed, off, lens = cu.random_packed(rng, M, 20, 40)
    e.set_reads(packed, off, lens)
    e.set_overlaps(M, rows, cols, vals)
    assert L.elba_pop_bubbles(e.h, C.byref(cfg), C.byref(st)) == 5                    # an edge list is not an S
    _load(e, M, rows, cols, vals)
    g = e.export_string_graph()
    f = e.export_read_flags(M)
    e.generate_contigs()
    contigs = e.export_contigs()
    assert contigs["n"] > 0

    def unchanged():
        _same_S(e.export_string_graph(), g["rows"], g["cols"], g["vals"])
        assert (e.export_read_flags(M) == f).all()
        now = e.export_contigs()
        assert now["n"] == contigs["n"] and now["seqs"] == contigs["seqs"] and (now["chain_read"] == contigs["chain_read"]).all()

    assert L.elba_pop_bubbles(e.h, None, C.byref(st)) == 1
    unchanged()
    for mx, rounds, res in ((0, 1, (0, 0)), (65536, 1, (0, 0)), (3, 0, (0, 0)), (3, 65, (0, 0)), (3, 1, (1, 0)), (3, 1, (0, 7)), (-1, 1, (0, 0))):
        bad = capi.BubbleCfg(mx, rounds, (C.c_int32 * 2)(*res))
        assert L.elba_pop_bubbles(e.h, C.byref(bad), C.byref(st)) == 1, (mx, rounds, res)
        unchanged()
    assert L.elba_pop_bubbles(e.h, C.byref(cfg), None) == 0                            # stats are optional
    assert e.export_string_graph()["n"] == g["n"] - 10                                # the arms of 1 and 2 reads: 3 reads, 5 pairs
    with pytest.raises(elba_amd.ElbaError) as err:
        e.export_contigs()
    assert err.value.status == 5
    e.close()


def test_what_it_is_for_planted_bubbles_do_not_break_contigs():
    """A path of 20 000 reads; 200 one-read arms planted across stretches of three reads, 97 reads apart.  Unpopped, both ends of every
    stretch are branches and the path falls into 401 contigs; after pop_bubbles(4, 1) S is, byte for byte, the path's, and so is the contig."""
    n, nb = 20000, 200
    g = tu.Graph()
    g.chain(g.new(n))
    M, rows, cols, vals = g.overlaps(np.random.default_rng(21))
    rng = np.random.default_rng(22)
    starts = 50 + 97 * np.arange(nb)
    assert starts[-1] + 4 < n and (np.diff(starts) - 4 >= 10).all()
    M2, r2, c2, v2, planted = bu.plant_bubbles(rng, M, rows, cols, vals, [(int(s), int(s) + 4) for s in starts], [1] * nb)
    packed, off, lens = cu.random_packed(rng, M2, 20, 40)
    nbytes = int(off[M - 1]) + (int(lens[M - 1]) + 3) // 4
    base_packed = np.concatenate([packed[:nbytes], np.zeros(16, np.uint8)])

    e0 = elba_amd.Engine(17, 2, 8)
    e0.set_reads(base_packed, off[:M], lens[:M])
    _load(e0, M, rows, cols, vals)
    g0 = e0.export_string_graph()
    assert g0["n"] == 2 * (n - 1) and np.bincount(g0["cols"], minlength=M).max() == 2          # one clean path
    st0 = e0.generate_contigs()
    base = e0.export_contigs()
    assert st0["contigs"] == 1 and st0["contig_reads"] == n
    e0.close()

    e = elba_amd.Engine(17, 2, 8)
    e.set_reads(packed, off, lens)
    _load(e, M2, r2, c2, v2)
    S = e.export_string_graph()
    assert S["n"] == g0["n"] + 4 * nb
    want_before = cu.generate_contigs(M2, S["rows"], S["cols"], S["vals"], cu.seqs_of(packed, off, lens))[3]
    st = e.generate_contigs()
    assert st["contigs"] == want_before["contigs"] == 2 * nb + 1 and st["branches"] == want_before["branches"] == 2 * nb      # before, stretch, after: at every bubble
    bs, _ = _pop(e, M2, 4, 1)
    assert bs["bubbles"] == nb and bs["arms"] == 2 * nb and bs["reads_removed"] == nb and bs["anchors"] == 2 * nb and bs["rounds_run"] == 1
    flags = e.export_read_flags(M2)
    assert (flags[planted] == 8).all() and flags.sum() == 8 * nb
    _same_S(e.export_string_graph(), g0["rows"], g0["cols"], g0["vals"])
    for single in (False, True):
        e.generate_contigs(singletons=single)
        got = e.export_contigs()
        assert got["n"] == base["n"] == 1 and got["seqs"] == base["seqs"]                      # the popped reads are not emitted as singletons
        for k in ("chain_read", "chain_prefix", "chain_strand", "kinds"):
            assert (got[k] == base[k]).all(), k
    e.close()
