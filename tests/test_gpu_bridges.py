"""-m gpu: elba_cut_bridges (elba_amd/csrc/bridges.hip) against the literal restatement of its rule in bridge_util.py: every entry of the cut
S in order, every byte of every value, the read flags and every integer stat.  Graphs are loaded with elba_set_overlaps with suffixes the
reduction does not remove at fuzz 0 (every suffix in [5, 9]: a two-edge walk is at least 10), and each load asserts nnz(S) == 2 x pairs."""
import ctypes as C
import functools

import numpy as np
import pytest

import bridge_util as br
import bubble_util as bu
import contig_util as cu
import elba_amd
import rounds_util as ru
import tip_util as tu
import weak_util as wu
from elba_amd import capi
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

CASES = br.hand_cases()
SEEDS = tuple(range(600, 624))
SG_TILE, SCAN_TILE = ru.SG_TILE, ru.SCAN_TILE                   # read from sg_rounds.hpp and prims.hip


def params_of(seed):
    return (2, 3) if seed % 4 == 0 else (1, 2)                  # as test_bridges_cpu.py: seeds 620 and 622 have a bridge


def _same_S(g, rows, cols, vals):
    assert g["n"] == len(rows) and (g["rows"] == rows).all() and (g["cols"] == cols).all()
    assert g["vals"].tobytes() == np.asarray(vals).tobytes()


def _load(e, M, rows, cols, vals, cutoff=0.0, fuzz=0, kept=True):
    e.set_overlaps(M, rows, cols, vals)
    s = e.transitive_reduction(cutoff, fuzz)
    if kept:
        assert s["nnz"] == 2 * len(rows)                        # the reduction keeps the graph as built
    return s


def _cut(e, M, mx, F):
    """cut_bridges on the engine's S equals the restatement on the S exported before the call.  Returns (stats, restatement's result)."""
    g = e.export_string_graph()
    f0 = e.export_read_flags(M)
    want = br.cut_bridges(M, g["rows"], g["cols"], g["vals"], mx, F)
    st = e.cut_bridges(mx, F)
    for k in br.STATS:
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
    M, rows, cols, vals = br.case_overlaps(case, np.random.default_rng(3), extra_reads=2)      # two isolated reads behind the graph
    _load(eng, M, rows, cols, vals)
    st, want = _cut(eng, M, case["mx"], case["F"])
    flags = eng.export_read_flags(M)
    assert set(np.flatnonzero(flags == 16).tolist()) == case["removed"] and flags.sum() == 16 * len(case["removed"])
    assert (st["chains"], st["long_flanks"], st["bridges"], st["reads_removed"]) == (case["chains"], case["long_flanks"], case["bridges"], len(case["removed"]))
    after = np.bincount(eng.export_string_graph()["cols"], minlength=M)
    for v, d in case["deg_after"].items():
        assert after[v] == d
    st2, _ = _cut(eng, M, case["mx"], case["F"])                # the pass is its own fixed point
    assert st2["reads_removed"] == 0 and st2["bridges"] == 0 and st2["nnz_after"] == st["nnz_after"]


@pytest.mark.parametrize("seed", SEEDS)
def test_random_graphs_with_both_images(eng, seed):
    M, rows, cols, vals, _, _ = ru.random_graph(seed)
    _load(eng, M, rows, cols, vals)
    mx, F = params_of(seed)
    st, _ = _cut(eng, M, mx, F)
    assert st["bridges"] == (1 if seed in (620, 622) else 0)
    st2, _ = _cut(eng, M, mx, F)
    assert st2["reads_removed"] == 0
    _load(eng, M, rows, cols, vals)                             # chains are the arms of one round of pop_bubbles, on a fresh load
    assert eng.pop_bubbles(mx, 1)["arms"] == st["chains"]


@pytest.mark.parametrize("seed", SEEDS)
def test_random_graphs_with_one_image_entries(eng, seed):
    """weak_util.random_S's pairs of which the reduction keeps one image: the contract there is what the statements give on the columns as
    they are, and the restatement says what that is.  The guarantees are not claimed, so a second call is compared, not expected to be idle."""
    rng = np.random.default_rng(seed)
    M = int(rng.integers(2, 120 if seed % 3 == 1 else 2500))
    (rows, cols, vals), _ = wu.random_S(rng, M, p_one_image=0.08)
    vals["suffix"] = rng.integers(5, 10, len(vals)); vals["suffixT"] = rng.integers(5, 10, len(vals))
    _load(eng, M, rows, cols, vals, kept=False)
    _same_S(eng.export_string_graph(), *wu.S_of(rows, cols, vals))      # the reduction keeps the graph as built, one-image pairs included
    mx, F = params_of(seed)
    _cut(eng, M, mx, F)
    _cut(eng, M, mx, F)


@functools.lru_cache(maxsize=None)
def _planted(seed, n_paths, length, n, t, gap):
    rng = np.random.default_rng(seed)
    M, rows, cols, vals = br.long_paths(rng, n_paths, length)
    return br.plant_bridges(rng, M, rows, cols, vals, n, t, gap=gap)


@pytest.mark.parametrize("nnz", [23 * SG_TILE - 1, 23 * SG_TILE, 23 * SG_TILE + 1, 3 * SCAN_TILE - 1, 3 * SCAN_TILE, 3 * SCAN_TILE + 1])
def test_planted_bridges_with_nnz_at_the_block_sizes_of_scan_and_compaction(eng, nnz):
    """About 3000 reads: five paths with 100 planted one-read bridges, and one more path whose length sets nnz(S) on, one below and one above
    a multiple of SG_TILE (k_sg_scatter's tile and the flat kernels' workgroup) that is none of the scan's tile, and of SCAN_TILE.  An odd
    nnz comes from one pair whose directionT is -1: the reduction keeps one image of it."""
    assert SG_TILE == 256 and SCAN_TILE == 2048 and (23 * SG_TILE) % SCAN_TILE != 0
    odd = nnz % 2
    M, rows, cols, vals, planted, pairs = _planted(31, 5, 500, 100, 1, 8)
    pairs_now = len(rows)
    extra = (nnz + odd) // 2 - pairs_now - odd                  # pairs of the last path
    assert extra >= 1
    M2 = M + extra + 1 + 2 * odd
    edges = {(int(r), int(c)): v for r, c, v in zip(rows, cols, vals)}
    rng = np.random.default_rng(nnz)
    for i in range(extra):
        o = cu.edge(rng, 20, 20); o["suffix"] = 7; o["suffixT"] = 6
        edges[(M + i, M + i + 1)] = o
    if odd:
        edges[(M2 - 2, M2 - 1)] = cu.edge(rng, 20, 20, directionT=-1)
    r2, c2, v2 = cu.upper(edges)
    s = _load(eng, M2, r2, c2, v2, kept=False)
    assert s["nnz"] == nnz
    st, _ = _cut(eng, M2, 1, 3)
    assert st["bridges"] == 100 and st["reads_removed"] == 100 and st["nnz_after"] == nnz - 400 and st["anchors"] == 200 and st["long_flanks"] == 400
    assert set(np.flatnonzero(eng.export_read_flags(M2) == 16).tolist()) == set(planted.tolist())


def test_40000_reads_with_2000_planted_bridges(eng):
    M, rows, cols, vals, planted, pairs = _planted(32, 20, 2000, 2000, 2, 8)
    assert M == 44000
    _load(eng, M, rows, cols, vals)
    st, _ = _cut(eng, M, 2, 8)
    assert st["bridges"] == 2000 and st["reads_removed"] == 4000 and st["entries_removed"] == 12000 and st["chains"] == 2000 and st["long_flanks"] == 8000
    assert (eng.export_read_flags(M)[planted] == 16).all()
    st2, _ = _cut(eng, M, 2, 8)
    assert st2["reads_removed"] == 0 and st2["anchors"] == 0


@pytest.mark.parametrize("F,cut", [(2000, 4), (2001, 0)])
def test_flank_walks_of_2000_steps(eng, F, cut):
    """Four bridges between anchors that lie exactly 2000 reads from each other and from the ends of their paths."""
    M, rows, cols, vals, planted, pairs = _planted(33, 4, 3 * 2001 + 1, 4, 1, 2000)
    _load(eng, M, rows, cols, vals)
    st, _ = _cut(eng, M, 1, F)
    assert st["bridges"] == cut and st["chains"] == 4 and st["long_flanks"] == 4 * cut and st["anchors"] == 8


def test_the_other_three_calls_go_on_from_the_cut_S_and_it_from_theirs(eng):
    """An H whose flank carries a tip, beside a bubble and a weak overlap: cut_bridges finds nothing until the tip is clipped; then each of
    the four calls is held against its restatement on the S the one before left, in both orders."""
    def graph():
        g = wu.WeakGraph()
        a, b, ch, fl = br._h(g, 1, (3, 3, 3, 3))
        tip = g.arm(fl[0][1], 1)
        bu._bubble(g, [1, 2])
        wu._y(g, 2, (100, 30), (1, 1), tail=5)
        return g, ch, tip

    g, ch, tip = graph()
    M, rows, cols, vals = g.overlaps(np.random.default_rng(6))
    for first in ("bridges", "others"):
        _load(eng, M, rows, cols, vals)
        if first == "bridges":
            st, _ = _cut(eng, M, 1, 3)
            assert st["bridges"] == 0 and st["chains"] == 3     # the bar of the H, the read between a and the tip's anchor, the bubble's arm of one read
        S = eng.export_string_graph()
        want = tu.clip_tips(M, S["rows"], S["cols"], S["vals"], 1, 64)
        ts = eng.clip_tips(1, 64)
        assert all(ts[k] == want[4][k] for k in tu.STATS) and ts["reads_removed"] == 1
        S = eng.export_string_graph()
        want = bu.pop_bubbles(M, S["rows"], S["cols"], S["vals"], 3, 64)
        bs = eng.pop_bubbles(3, 64)
        assert all(bs[k] == want[4][k] for k in bu.STATS) and bs["reads_removed"] == 1
        S = eng.export_string_graph()
        want = wu.cut_weak(M, S["rows"], S["cols"], S["vals"], wu.Q07)
        ws = eng.cut_weak_overlaps(0.7)
        assert all(ws[k] == want[3][k] for k in wu.STATS) and ws["entries_removed"] == 2
        _same_S(eng.export_string_graph(), want[0], want[1], want[2])
        st, _ = _cut(eng, M, 1, 3)
        assert st["bridges"] == 1 and st["reads_removed"] == 1
        f = eng.export_read_flags(M)
        assert f[ch[0]] == 16 and f[tip[0]] == 4 and f.sum() == 16 + 4 + 8
        S = eng.export_string_graph()                           # and the three go on from the cut S
        want = tu.clip_tips(M, S["rows"], S["cols"], S["vals"], 3, 64)
        ts = eng.clip_tips(3, 64)
        assert all(ts[k] == want[4][k] for k in tu.STATS)
        _same_S(eng.export_string_graph(), want[0], want[1], want[2])
        S = eng.export_string_graph()
        want = bu.pop_bubbles(M, S["rows"], S["cols"], S["vals"], 3, 64)
        bs = eng.pop_bubbles(3, 64)
        assert all(bs[k] == want[4][k] for k in bu.STATS)
        _same_S(eng.export_string_graph(), want[0], want[1], want[2])
        S = eng.export_string_graph()
        want = wu.cut_weak(M, S["rows"], S["cols"], S["vals"], wu.Q07)
        ws = eng.cut_weak_overlaps(0.7)
        assert all(ws[k] == want[3][k] for k in wu.STATS)
        _same_S(eng.export_string_graph(), want[0], want[1], want[2])


def test_errors_leave_S_flags_and_contigs_untouched():
    e = elba_amd.Engine(17, 2, 8)
    L = e.L
    cfg = capi.BridgeCfg(1, 2, (C.c_int32 * 2)(0, 0))
    st = capi.BridgeStats()
    assert L.elba_cut_bridges(e.h, C.byref(cfg), C.byref(st)) == 5                    # no S
    rng = np.random.default_rng(2)
    M, rows, cols, vals = br.case_overlaps(CASES["h_bar_of_1_cut_mx1_F2"], rng)
    packed, off, lens = cu.random_packed(rng, M, 20, 40)
    e.set_reads(packed, off, lens)
    e.set_overlaps(M, rows, cols, vals)
    assert L.elba_cut_bridges(e.h, C.byref(cfg), C.byref(st)) == 5                    # an edge list is not an S
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

    assert L.elba_cut_bridges(e.h, None, C.byref(st)) == 1
    unchanged()
    for mx, F, res in ((0, 2, (0, 0)), (-1, 2, (0, 0)), (65535, 65535, (0, 0)), (65535, 65536, (0, 0)), (65536, 65537, (0, 0)), (2, 2, (0, 0)), (3, 2, (0, 0)), (1, 1, (0, 0)),
                       (1, 0, (0, 0)), (1, 65536, (0, 0)), (65534, 65536, (0, 0)), (1, 2, (1, 0)), (1, 2, (0, 7)), (1, 2, (0, -1))):
        bad = capi.BridgeCfg(mx, F, (C.c_int32 * 2)(*res))
        assert L.elba_cut_bridges(e.h, C.byref(bad), C.byref(st)) == 1, (mx, F, res)
        unchanged()
    assert L.elba_cut_bridges(e.h, C.byref(capi.BridgeCfg(65534, 65535, (C.c_int32 * 2)(0, 0))), C.byref(st)) == 0 and st.reads_removed == 0       # the largest cfg is accepted
    e.generate_contigs()
    assert L.elba_cut_bridges(e.h, C.byref(cfg), None) == 0                            # stats are optional
    assert e.export_string_graph()["n"] == g["n"] - 4           # the one bridge read, two pairs
    with pytest.raises(elba_amd.ElbaError) as err:              # contigs made before are invalid after ELBA_OK
        e.export_contigs()
    assert err.value.status == 5
    e.close()


def test_empty_graph_and_context_without_reads(eng):
    z = np.zeros(0, dtype=po.OVERLAP_DTYPE)
    for M in (5, 0):
        _load(eng, M, np.zeros(0, np.int64), np.zeros(0, np.int64), z)
        st, _ = _cut(eng, M, 1, 2)
        assert st["nnz_after"] == 0 and st["reads_removed"] == 0 and st["nreads"] == M and st["anchors"] == 0 and st["chains"] == 0
        assert eng.export_string_graph()["n"] == 0


def test_one_context_over_graphs_of_changing_size():
    e = elba_amd.Engine(17, 2, 8)
    z = np.zeros(0, dtype=po.OVERLAP_DTYPE)
    big = _planted(32, 20, 2000, 2000, 2, 8)[:4]
    small = br.case_overlaps(CASES["cycle_with_one_chord_chain_mx2_F3"], np.random.default_rng(1))
    for (M, rows, cols, vals), mx, F, n in ((big, 2, 8, 2000), (small, 2, 3, 1), ((7, np.zeros(0, np.int64), np.zeros(0, np.int64), z), 1, 2, 0), (big, 3, 4, 2000)):
        _load(e, M, rows, cols, vals)
        st, _ = _cut(e, M, mx, F)
        assert st["bridges"] == n
    st, _ = _cut(e, big[0], 3, 4)
    assert st["reads_removed"] == 0 and st["nnz_after"] == st["nnz_before"]
    e.close()


def test_what_it_is_for_an_H_is_two_contigs_not_four():
    """The H with reads on the context: before the cut four contigs and two branches; after it two contigs whose chains are the two whole
    paths, byte for byte what contig_util makes of the cut S, and with singletons asked for the bridge read does not come back."""
    g = tu.Graph()
    a, b, ch, fl = br._h(g, 1, (4, 5, 6, 7))
    rng = np.random.default_rng(4)
    M, rows, cols, vals = g.overlaps(rng)
    packed, off, lens = cu.random_packed(rng, M, 20, 40)
    seqs = cu.seqs_of(packed, off, lens)
    e = elba_amd.Engine(17, 2, 8)
    e.set_reads(packed, off, lens)
    _load(e, M, rows, cols, vals)
    st0 = e.generate_contigs()
    assert st0["contigs"] == 4 and st0["branches"] == 2
    st, want = _cut(e, M, 1, 4)
    assert st["bridges"] == 1 and st["reads_removed"] == 1
    with pytest.raises(elba_amd.ElbaError) as err:              # the contigs of the uncut graph are gone
        e.export_contigs()
    assert err.value.status == 5
    contigs, chains, _, cst = cu.generate_contigs(M, want[0], want[1], want[2], seqs)
    for single in (False, True):
        st1 = e.generate_contigs(singletons=single)
        got = e.export_contigs()
        assert st1["contigs"] == 2 and st1["branches"] == 0 and got["n"] == 2 and list(got["seqs"]) == list(contigs)
        assert got["chain_read"].tolist() == [v for chain in chains for v, _, _ in chain]
        assert got["chain_prefix"].tolist() == [p for chain in chains for _, p, _ in chain] and got["chain_strand"].tolist() == [s for chain in chains for _, _, s in chain]
    # the two whole paths: a with its flanks and their dead ends, b with its
    sets = [set(got["chain_read"][int(got["chain_off"][i]):int(got["chain_off"][i + 1])].tolist()) for i in range(2)]
    whole = [{a} | set(fl[0]) | set(fl[1]) | {fl[0][-1] + 1, fl[1][-1] + 1}, {b} | set(fl[2]) | set(fl[3]) | {fl[2][-1] + 1, fl[3][-1] + 1}]
    assert sets == whole and [len(c) for c in chains] == [len(w) for w in whole]
    e.close()


def test_cycle_with_a_chord_chain_becomes_one_circular_contig():
    case = CASES["cycle_with_one_chord_chain_mx2_F3"]
    rng = np.random.default_rng(4)
    M, rows, cols, vals = br.case_overlaps(case, rng)
    packed, off, lens = cu.random_packed(rng, M, 20, 40)
    e = elba_amd.Engine(17, 2, 8)
    e.set_reads(packed, off, lens)
    _load(e, M, rows, cols, vals)
    st0 = e.generate_contigs(circular=True)
    assert st0["cycles"] == 0 and st0["branches"] == 2 and (e.export_contigs()["kinds"] == 1).sum() == 0
    st, _ = _cut(e, M, 2, 3)
    assert st["bridges"] == 1 and st["reads_removed"] == 2
    st1 = e.generate_contigs(circular=True)
    got = e.export_contigs()
    assert st1["cycles"] == 1 and got["n"] == 1 and got["kinds"].tolist() == [1] and st1["contig_reads"] == len(case["cycle"]) == 9
    assert set(got["chain_read"].tolist()) == set(case["cycle"])
    e.close()


@pytest.mark.parametrize("seed", ru.SIMPLIFY_WEAK_SEEDS)
def test_simplify_graph_with_bridges_against_the_restatements(eng, seed):
    M, rows, cols, vals, mx_tip, mx_arm = ru.random_scored(seed)
    bridges = params_of(seed)
    for ratio in (None, 0.7):
        _load(eng, M, rows, cols, vals)
        S = eng.export_string_graph()
        want = br.simplify(M, S["rows"], S["cols"], S["vals"], mx_tip, mx_arm, bridges, q16=None if ratio is None else wu.Q07)
        got = eng.simplify_graph(mx_tip, mx_arm, min_overlap_ratio=ratio, bridges=bridges)
        assert len(got) == len(want[4])
        for p, wp in zip(got, want[4]):
            assert len(p) == len(wp) == (3 if ratio is None else 4)
            assert all(p[0][k] == wp[0][k] for k in tu.STATS) and all(p[1][k] == wp[1][k] for k in bu.STATS) and all(p[-1][k] == wp[-1][k] for k in br.STATS)
            assert ratio is None or all(p[2][k] == wp[2][k] for k in wu.STATS)
        _same_S(eng.export_string_graph(), want[0], want[1], want[2])
        assert (eng.export_read_flags(M) == want[3]).all()


def test_simplify_graph_ends_with_cut_bridges_and_without_bridges_does_what_it_did(eng):
    g = tu.Graph()
    a, b, ch, fl = br._h(g, 1, (3, 3, 3, 3))
    tip = g.arm(fl[0][1], 1)
    M, rows, cols, vals = g.overlaps(np.random.default_rng(7))
    _load(eng, M, rows, cols, vals)
    got = eng.simplify_graph(1, 3, bridges=(1, 3))
    assert len(got) == 2 and all(len(p) == 3 for p in got) and got[0][0]["reads_removed"] == 1 and got[0][2]["bridges"] == 1 and got[1][2]["reads_removed"] == 0
    f = eng.export_read_flags(M)
    assert f[tip[0]] == 4 and f[ch[0]] == 16 and f.sum() == 20
    _load(eng, M, rows, cols, vals)
    assert len(eng.simplify_graph(1, 3, passes=1, bridges=(1, 3))) == 1                        # `passes` bounds it
    for args, q16 in (((1, 3), None), ((1, 3, 16, None, None), None), ((1, 3, 16, 0.7), wu.Q07)):
        _load(eng, M, rows, cols, vals)
        S = eng.export_string_graph()
        want = bu.simplify(M, S["rows"], S["cols"], S["vals"], 1, 3) if q16 is None else wu.simplify(M, S["rows"], S["cols"], S["vals"], 1, 3, q16)
        got = eng.simplify_graph(*args)
        assert len(got) == len(want[4]) and all(len(p) == len(wp) == (2 if q16 is None else 3) for p, wp in zip(got, want[4]))
        for p, wp in zip(got, want[4]):
            assert all(p[0][k] == wp[0][k] for k in tu.STATS) and all(p[1][k] == wp[1][k] for k in bu.STATS)
        _same_S(eng.export_string_graph(), want[0], want[1], want[2])
        assert (eng.export_read_flags(M) == want[3]).all() and eng.export_read_flags(M)[ch[0]] == 0      # the bridge is still there
