"""-m gpu: elba_cut_weak_overlaps (elba_amd/csrc/weak.hip) against the literal restatement of its rule in weak_util.py: every entry of the
cut S in order, every byte of every value, the stats, and the read flags, which must not change.  Graphs are loaded with elba_set_overlaps
with suffixes the reduction does not remove at fuzz 0 (every suffix in [5, 9]: a two-edge walk is at least 10); score, direction and
directionT are set explicitly, and each load asserts that the exported S is the one weak_util.S_of expects."""
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
import weak_util as wu
from elba_amd import capi
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

CASES = wu.hand_cases()


SG_TILE, SCAN_TILE = ru.SG_TILE, ru.SCAN_TILE                   # read from sg_rounds.hpp and prims.hip


def _same_S(g, rows, cols, vals):
    assert g["n"] == len(rows) and (g["rows"] == rows).all() and (g["cols"] == cols).all()
    assert g["vals"].tobytes() == np.asarray(vals).tobytes()


def _load(e, M, rows, cols, vals, cutoff=0.0, fuzz=0, exact=True):
    e.set_overlaps(M, rows, cols, vals)
    s = e.transitive_reduction(cutoff, fuzz)
    if exact:
        _same_S(e.export_string_graph(), *wu.S_of(rows, cols, vals))      # the reduction keeps the graph as built, one-image pairs included
    return s


def _cut(e, M, q16, restate=wu.cut_weak):
    """cut_weak_overlaps on the engine's S equals the restatement on the S exported before the call.  Returns (stats, restatement's result)."""
    g = e.export_string_graph()
    f0 = e.export_read_flags(M)
    want = restate(M, g["rows"], g["cols"], g["vals"], q16)
    st = e.cut_weak_overlaps(q16 / 65536)                       # exact: q16 / 65536 * 65536 is q16 again
    for k in wu.STATS:
        assert st[k] == want[3][k], (k, st, want[3])
    assert st["ms_total"] >= 0 and st["ms_compact"] >= 0
    _same_S(e.export_string_graph(), want[0], want[1], want[2])
    assert (e.export_read_flags(M) == f0).all()
    return st, want


@pytest.fixture(scope="module")
def eng():
    e = elba_amd.Engine(17, 2, 8)
    yield e
    e.close()


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_rule_one_clause_per_case(eng, name):
    case = CASES[name]
    (M, rows, cols, vals), S = wu.case_S(case, np.random.default_rng(3), extra_reads=2)        # two isolated reads behind the graph
    _load(eng, M, rows, cols, vals)
    before = eng.export_string_graph()
    st, want = _cut(eng, M, case["q16"])
    after = eng.export_string_graph()
    gone = {(int(r), int(c)) for r, c in zip(before["rows"], before["cols"])} - {(int(r), int(c)) for r, c in zip(after["rows"], after["cols"])}
    assert {frozenset(p) for p in gone} == case["removed"]
    assert st["weak_entries"] == len(case["weak"]) and st["branch_sides"] == case["branch_sides"] and st["sides_emptied"] == case["sides_emptied"]
    assert st["entries_removed"] == len(gone) and eng.export_read_flags(M).sum() == 0
    st2, _ = _cut(eng, M, case["q16"])                          # the pass is its own fixed point
    assert st2["entries_removed"] == 0 and st2["weak_entries"] == 0 and st2["nnz_after"] == st["nnz_after"]


def test_the_removed_set_grows_with_the_ratio_on_the_device(eng):
    rng = np.random.default_rng(8)
    M = 300
    rows, cols, vals = cu.random_string_graph(rng, M, np.full(M, 20))
    vals["score"] = rng.integers(-3, 40, len(vals))
    vals["suffix"] = rng.integers(5, 10, len(vals)); vals["suffixT"] = rng.integers(5, 10, len(vals))
    kept = []
    for q16 in (1, 16384, 32768, wu.Q07, 65536):
        _load(eng, M, rows, cols, vals)
        _cut(eng, M, q16)
        g = eng.export_string_graph()
        kept.append({(int(r), int(c)) for r, c in zip(g["rows"], g["cols"])})
    assert all(large <= small for small, large in zip(kept[:-1], kept[1:])) and len(kept[-1]) < len(kept[0])


@pytest.mark.parametrize("M", [1, 64, 65, 65537])
def test_read_counts_at_wavefront_and_block_edges(eng, M):
    if M == 1:
        _load(eng, 1, np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, dtype=po.OVERLAP_DTYPE))
        st, _ = _cut(eng, 1, wu.Q07)
        assert st["nnz_before"] == 0 and st["entries_removed"] == 0
        return
    g = wu.WeakGraph()
    a, (x, y) = wu._y(g, 2, (100, 69), (1, 1))
    rest = [v for v in range(g.n) if v not in (a, y)]
    perm = np.zeros(g.n, dtype=np.int64)
    perm[a], perm[y] = 0, M - 1                                 # the branch side is side 1 of read 0, the emptied one side 0 of read M - 1
    perm[rest] = np.arange(M - 1 - len(rest), M - 1)            # the graph's other reads next to the last one, isolated reads between
    Mx, rows, cols, vals = g.overlaps(np.random.default_rng(M), perm=perm, M=M)
    _load(eng, M, rows, cols, vals)
    st, _ = _cut(eng, M, wu.Q07)
    assert st["entries_removed"] == 2 and st["weak_entries"] == 1 and st["sides_emptied"] == 1 and st["branch_sides"] == 1
    after = eng.export_string_graph()
    assert not ((after["rows"] == M - 1) & (after["cols"] == 0)).any() and not ((after["rows"] == 0) & (after["cols"] == M - 1)).any()


@pytest.mark.parametrize("nnz", [SG_TILE - 1, SG_TILE, SG_TILE + 1, SG_TILE + 3, 4 * SG_TILE - 1, 4 * SG_TILE, 4 * SG_TILE + 1, 4 * SG_TILE + 3,
                                 SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, SCAN_TILE + 3])
def test_nnz_at_the_block_sizes_of_scan_and_compaction(eng, nnz):
    """nnz(S) round SG_TILE (k_sg_scatter's tile and the flat kernels' workgroup), four of them, and the scan's SCAN_TILE, with an odd count
    just above each.  The scan and k_weak_keep run over nnz + 1 elements, so nnz = tile - 1 gives them exactly a tile.  An odd nnz comes from
    one pair whose directionT is -1."""
    assert SG_TILE == 256 and SCAN_TILE == 2048
    odd = nnz % 2
    g = wu.WeakGraph()
    a, (x, y) = wu._y(g, 2, (100, 69), (1, 1))
    g.chain(g.new(nnz // 2 - len(g.pairs) + 1))
    if odd:
        p, q = g.new(2)
        g.link(p, q, 30, one_image=True)
    assert 2 * len(g.pairs) - odd == nnz
    Mx, rows, cols, vals = g.overlaps(np.random.default_rng(nnz), perm=np.random.default_rng(nnz + 1).permutation(g.n))
    s = _load(eng, Mx, rows, cols, vals)
    assert s["nnz"] == nnz
    st, _ = _cut(eng, Mx, wu.Q07)
    assert st["entries_removed"] == 2 and st["nnz_after"] == nnz - 2 and st["branch_sides"] == 1


@pytest.mark.parametrize("n", [255, 256, 257, 3000])
def test_one_column_of_many_entries_with_the_best_in_its_last_lanes(eng, n):
    """Read 0 has n neighbours, alternately on its two sides; the best of each side is in the last two entries of the column, whose lanes
    fold them into tables that n - 2 other lanes of several wavefronts and workgroups hit as well."""
    g = wu.WeakGraph()
    hub = g.new()[0]
    leaves = g.new(n)
    score = [600 + (i * 37) % 400 for i in range(n)]
    score[-1] = score[-2] = 1000
    for i, v in enumerate(leaves):
        g.link(hub, v, score[i], su=i & 1, sv=0)
    Mx, rows, cols, vals = g.overlaps(np.random.default_rng(n))
    _load(eng, Mx, rows, cols, vals)
    st, want = _cut(eng, Mx, wu.Q07)
    low = sum(1 for s in score if s < 700)
    assert low > n // 8 and st["weak_entries"] == low and st["entries_removed"] == 2 * low and st["branch_sides"] == 2 and st["sides_emptied"] == low
    assert (np.bincount(want[1], minlength=Mx)[0] == n - low)


def test_read_flags_1_2_4_8_are_present_and_stay(eng):
    """A contained read and a bad read hang on the losing arm's read in the input (the prunes take them), a tip hangs on the bubble's
    anchor, and a weak overlap lies beside: after pop_bubbles and clip_tips the flags 1, 2, 4 and 8 are all there, and the cut leaves them."""
    g = wu.WeakGraph()
    a, b, ch = bu._bubble(g, [1, 2])
    tip = g.arm(a, 1)[0]
    x = ch[0][0]
    ya, (yx, yy) = wu._y(g, 2, (100, 30), (1, 1))
    rng = np.random.default_rng(5)
    M, rows, cols, vals = g.overlaps(rng, M=g.n + 3)
    iso, w, z = g.n, g.n + 1, g.n + 2
    edges = {(int(r), int(c)): v for r, c, v in zip(rows, cols, vals)}
    edges[(x, w)] = cu.edge(rng, 20, 20); edges[(x, w)]["containedT"] = 1
    edges[(x, z)] = cu.edge(rng, 20, 20); edges[(x, z)]["passed"] = 0
    r2, c2, v2 = cu.upper(edges)
    s = _load(eng, M, r2, c2, v2, cutoff=0.5, exact=False)
    assert s["nnz"] == 2 * len(rows) and s["bad_reads"] == 1 and s["contained_reads"] == 1
    assert eng.pop_bubbles(3)["reads_removed"] == 1 and eng.clip_tips(1)["reads_removed"] == 1
    f = eng.export_read_flags(M)
    assert f[x] == 8 and f[tip] == 4 and f[z] == 1 and f[w] == 2 and f[iso] == 0 and f.sum() == 15
    st, _ = _cut(eng, M, wu.Q07)                                # (_cut holds the flags after against the flags before)
    assert st["entries_removed"] == 2 and (eng.export_read_flags(M) == f).all()


def test_empty_graph_and_context_without_reads(eng):
    z = np.zeros(0, dtype=po.OVERLAP_DTYPE)
    for M in (5, 0):
        _load(eng, M, np.zeros(0, np.int64), np.zeros(0, np.int64), z)
        st, _ = _cut(eng, M, wu.Q07)
        assert st["nnz_after"] == 0 and st["entries_removed"] == 0 and st["nreads"] == M and st["branch_sides"] == 0 and st["sides_emptied"] == 0
        assert eng.export_string_graph()["n"] == 0


@functools.lru_cache(maxsize=None)
def _layout(seed, M):
    rng = np.random.default_rng(seed)
    rows, cols, vals = sg.layout_overlaps(rng, M, 8)
    return rows, cols, vals


def test_one_context_over_graphs_of_changing_size():
    e = elba_amd.Engine(17, 2, 8)
    z = np.zeros(0, dtype=po.OVERLAP_DTYPE)
    big = (40000,) + _layout(1, 40000)
    small = wu.case_S(CASES["best_at_its_column_weak_at_its_row"], np.random.default_rng(1))[0]
    for (M, rows, cols, vals), exact, fuzz in ((big, False, 1000), (small, True, 0), ((7, np.zeros(0, np.int64), np.zeros(0, np.int64), z), True, 0), (big, False, 1000)):
        _load(e, M, rows, cols, vals, cutoff=0.0 if exact else 0.65, fuzz=fuzz, exact=exact)
        st, _ = _cut(e, M, wu.Q07, restate=wu.cut_weak if M < 1000 else wu.cut_weak_sorted)
        if M == big[0]:
            assert st["entries_removed"] >= 1000 and st["branch_sides"] >= 1000
    # a second call on the cut graph finds nothing; a larger ratio goes on from there
    st, _ = _cut(e, big[0], wu.Q07, restate=wu.cut_weak_sorted)
    assert st["entries_removed"] == 0 and st["nnz_after"] == st["nnz_before"]
    st, _ = _cut(e, big[0], 65536, restate=wu.cut_weak)        # and once the literal restatement at this size
    assert st["entries_removed"] > 0
    e.close()


def test_errors_leave_S_flags_and_contigs_untouched():
    e = elba_amd.Engine(17, 2, 8)
    L = e.L
    cfg = capi.WeakCfg(wu.Q07, (C.c_int32 * 3)(0, 0, 0))
    st = capi.WeakStats()
    assert L.elba_cut_weak_overlaps(e.h, C.byref(cfg), C.byref(st)) == 5              # no S
    rng = np.random.default_rng(2)
    (M, rows, cols, vals), _ = wu.case_S(CASES["y_same_side_100_69_cut"], rng)
    packed, off, lens = cu.random_packed(rng, M, 20, 40)
    e.set_reads(packed, off, lens)
    e.set_overlaps(M, rows, cols, vals)
    assert L.elba_cut_weak_overlaps(e.h, C.byref(cfg), C.byref(st)) == 5              # an edge list is not an S
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

    assert L.elba_cut_weak_overlaps(e.h, None, C.byref(st)) == 1
    unchanged()
    for q16, res in ((0, (0, 0, 0)), (65537, (0, 0, 0)), (-1, (0, 0, 0)), (-2 ** 31, (0, 0, 0)), (2 ** 31 - 1, (0, 0, 0)), (wu.Q07, (1, 0, 0)), (wu.Q07, (0, 7, 0)),
                     (wu.Q07, (0, 0, -1))):
        bad = capi.WeakCfg(q16, (C.c_int32 * 3)(*res))
        assert L.elba_cut_weak_overlaps(e.h, C.byref(bad), C.byref(st)) == 1, (q16, res)
        unchanged()
    with pytest.raises(ValueError):                             # the binding refuses before the library sees it
        e.cut_weak_overlaps(1.5)
    unchanged()
    assert L.elba_cut_weak_overlaps(e.h, C.byref(cfg), None) == 0                      # stats are optional
    assert e.export_string_graph()["n"] == g["n"] - 2
    with pytest.raises(elba_amd.ElbaError) as err:              # contigs made before are invalid after ELBA_OK
        e.export_contigs()
    assert err.value.status == 5
    for q16 in (1, 65536):                                      # both ends of the range are accepted
        assert L.elba_cut_weak_overlaps(e.h, C.byref(capi.WeakCfg(q16, (C.c_int32 * 3)(0, 0, 0))), C.byref(st)) == 0 and st.entries_removed == 0
    e.close()


def _tip_after_cut_graph():
    """main[6] - t0 - t1 ~ other[6]: the last overlap is weak at other[6], so after the cut t0, t1 is a tip of two reads at main[6]; beside
    it a bubble of arms 1 and 2 whose overlaps all tie."""
    g = wu.WeakGraph()
    main = g.chain(g.new(12))
    t = g.chain(g.new(2))
    g.link(main[6], t[0], 100, su=1, sv=0)
    other = g.chain(g.new(12))
    g.link(t[1], other[6], 30, su=1, sv=0)
    a, b, ch = bu._bubble(g, [1, 2])
    return g, main, t, other, ch


def test_clip_tips_and_pop_bubbles_go_on_from_the_cut_S(eng):
    g, main, t, other, ch = _tip_after_cut_graph()
    M, rows, cols, vals = g.overlaps(np.random.default_rng(6))
    _load(eng, M, rows, cols, vals)
    assert eng.clip_tips(3, 64)["reads_removed"] == 0           # t1 has degree 2: no tip yet
    st, _ = _cut(eng, M, wu.Q07)
    assert st["entries_removed"] == 2 and st["sides_emptied"] == 1
    S = eng.export_string_graph()
    want = tu.clip_tips(M, S["rows"], S["cols"], S["vals"], 3, 64)
    ts = eng.clip_tips(3, 64)
    assert all(ts[k] == want[4][k] for k in tu.STATS) and ts["reads_removed"] == 2
    _same_S(eng.export_string_graph(), want[0], want[1], want[2])
    S = eng.export_string_graph()
    want = bu.pop_bubbles(M, S["rows"], S["cols"], S["vals"], 3, 64)
    bs = eng.pop_bubbles(3, 64)
    assert all(bs[k] == want[4][k] for k in bu.STATS) and bs["reads_removed"] == 1
    _same_S(eng.export_string_graph(), want[0], want[1], want[2])
    f = eng.export_read_flags(M)
    assert f[t[0]] == 4 and f[t[1]] == 4 and f[ch[0][0]] == 8 and f.sum() == 16
    st, _ = _cut(eng, M, wu.Q07)
    assert st["entries_removed"] == 0


def test_simplify_graph_with_a_ratio_runs_the_three_calls(eng):
    g, main, t, other, ch = _tip_after_cut_graph()
    M, rows, cols, vals = g.overlaps(np.random.default_rng(7))
    _load(eng, M, rows, cols, vals)
    S = eng.export_string_graph()
    want = wu.simplify(M, S["rows"], S["cols"], S["vals"], 3, 3, wu.Q07)
    got = eng.simplify_graph(3, 3, min_overlap_ratio=0.7)
    assert len(got) == len(want[4]) == 3                        # the bubble and the cut; then the tip the cut made; then nothing
    for p, wp in zip(got, want[4]):
        assert len(p) == 3
        assert all(p[0][k] == wp[0][k] for k in tu.STATS) and all(p[1][k] == wp[1][k] for k in bu.STATS) and all(p[2][k] == wp[2][k] for k in wu.STATS)
    assert got[0][2]["entries_removed"] == 2 and got[1][0]["reads_removed"] == 2 and got[0][1]["reads_removed"] == 1
    _same_S(eng.export_string_graph(), want[0], want[1], want[2])
    assert (eng.export_read_flags(M) == want[3]).all()
    _load(eng, M, rows, cols, vals)
    assert len(eng.simplify_graph(3, 3, passes=1, min_overlap_ratio=0.7)) == 1                 # `passes` bounds it
    with pytest.raises(ValueError):
        eng.simplify_graph(3, 3, min_overlap_ratio=0.0)


def test_simplify_graph_without_a_ratio_does_what_it_did(eng):
    g, main, t, other, ch = _tip_after_cut_graph()
    M, rows, cols, vals = g.overlaps(np.random.default_rng(7))
    _load(eng, M, rows, cols, vals)
    S = eng.export_string_graph()
    want = bu.simplify(M, S["rows"], S["cols"], S["vals"], 3, 3)
    for got in (eng.simplify_graph(3, 3), None):
        if got is None:
            _load(eng, M, rows, cols, vals)
            got = eng.simplify_graph(3, 3, 16, None)
        assert len(got) == len(want[4]) == 2
        for p, wp in zip(got, want[4]):
            assert len(p) == 2 and all(p[0][k] == wp[0][k] for k in tu.STATS) and all(p[1][k] == wp[1][k] for k in bu.STATS)
        _same_S(eng.export_string_graph(), want[0], want[1], want[2])
        assert (eng.export_read_flags(M) == want[3]).all()
    assert eng.export_string_graph()["n"] == S["n"] - 4         # the losing arm's read; the weak overlap is still there


def test_what_it_is_for_planted_weak_overlaps_do_not_break_contigs():
    """A path of 20 000 reads with overlaps of score 100; 200 overlaps of score 30 planted between reads 5001 apart, each on a side of
    either read that the path already uses.  Uncut, both reads of every planted pair are branches and the path falls into pieces; after one
    cut_weak_overlaps(0.7) S is, byte for byte, the path's, and so is the contig."""
    n, nw = 20000, 200
    g = wu.WeakGraph()
    g.chain(g.new(n))
    M, rows, cols, vals = g.overlaps(np.random.default_rng(21))
    rng = np.random.default_rng(22)
    u = 50 + 97 * np.arange(nw)
    v = (u + 5001) % n
    pairs = [(int(min(a, b)), int(max(a, b))) for a, b in zip(u, v)]
    ends = np.array(pairs).reshape(-1)
    assert len(set(ends.tolist())) == 2 * nw and ends.min() > 0 and ends.max() < n - 1 and all(b - a > 2 for a, b in pairs)     # distinct inner reads, far apart
    r2, c2, v2 = wu.plant_weak_edges(M, rows, cols, vals, pairs, 30, rng.integers(0, 4, (nw, 2)).tolist())
    packed, off, lens = cu.random_packed(rng, M, 20, 40)

    e0 = elba_amd.Engine(17, 2, 8)
    e0.set_reads(packed, off, lens)
    _load(e0, M, rows, cols, vals)
    g0 = e0.export_string_graph()
    assert g0["n"] == 2 * (n - 1) and np.bincount(g0["cols"], minlength=M).max() == 2          # one clean path
    st0 = e0.generate_contigs()
    base = e0.export_contigs()
    assert st0["contigs"] == 1 and st0["contig_reads"] == n
    e0.close()

    e = elba_amd.Engine(17, 2, 8)
    e.set_reads(packed, off, lens)
    _load(e, M, r2, c2, v2)
    S = e.export_string_graph()
    assert S["n"] == g0["n"] + 2 * nw
    want_before = cu.generate_contigs(M, S["rows"], S["cols"], S["vals"], cu.seqs_of(packed, off, lens))[3]
    st = e.generate_contigs()
    assert st["contigs"] == want_before["contigs"] and st["branches"] == want_before["branches"] == 2 * nw and st["contigs"] > nw      # it falls into many contigs
    ws, _ = _cut(e, M, wu.Q07)
    assert ws["weak_entries"] == 2 * nw and ws["entries_removed"] == 2 * nw and ws["branch_sides"] == 2 * nw and ws["sides_emptied"] == 0
    _same_S(e.export_string_graph(), g0["rows"], g0["cols"], g0["vals"])
    assert e.export_read_flags(M).sum() == 0
    e.generate_contigs()
    got = e.export_contigs()
    assert got["n"] == base["n"] == 1 and got["seqs"] == base["seqs"]
    for k in ("chain_read", "chain_prefix", "chain_strand", "kinds"):
        assert (got[k] == base[k]).all(), k
    e.close()


def test_cycle_with_planted_chords_becomes_one_circular_contig():
    g = wu.WeakGraph()
    cyc = g.chain(g.new(12), closed=True)
    g.link(cyc[1], cyc[6], 40, su=1, sv=0)
    g.link(cyc[3], cyc[9], 55, su=0, sv=1)
    rng = np.random.default_rng(4)
    M, rows, cols, vals = g.overlaps(rng)
    packed, off, lens = cu.random_packed(rng, M, 20, 40)
    e = elba_amd.Engine(17, 2, 8)
    e.set_reads(packed, off, lens)
    _load(e, M, rows, cols, vals)
    st0 = e.generate_contigs(circular=True)
    assert st0["cycles"] == 0 and st0["branches"] == 4 and (e.export_contigs()["kinds"] == 1).sum() == 0
    st, _ = _cut(e, M, wu.Q07)
    assert st["entries_removed"] == 4 and st["weak_entries"] == 4 and st["sides_emptied"] == 0
    with pytest.raises(elba_amd.ElbaError) as err:              # the contigs of the uncut graph are gone
        e.export_contigs()
    assert err.value.status == 5
    st1 = e.generate_contigs(circular=True)
    got = e.export_contigs()
    assert st1["cycles"] == 1 and got["n"] == 1 and got["kinds"].tolist() == [1] and st1["contig_reads"] == 12
    e.close()
