"""-m gpu: elba_resolve_stars (elba_amd/csrc/stars.hip) against the literal restatement of its rule in star_util.py: every entry of the
resolved S in order, every byte of every value, the read flags and every integer stat.  Graphs are loaded with elba_set_overlaps; the pairs
of R are derived in Python from the loaded overlaps and the flags of the ORACLE's reduction (star_util.r_pairs), never from the device."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import bridge_util as br
import bubble_util as bu
import contig_util as cu
import elba_amd
import rounds_util as ru
import star_util as su
import tip_util as tu
import util
import weak_util as wu
from elba_amd import capi
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

CASES = su.hand_cases()
SEEDS = tuple(range(700, 724))
SG_TILE, SCAN_TILE, SG_BATCH = ru.SG_TILE, ru.SCAN_TILE, ru.SG_BATCH       # read from sg_rounds.hpp and prims.hip


def _same_S(g, rows, cols, vals):
    assert g["n"] == len(rows) and (g["rows"] == rows).all() and (g["cols"] == cols).all()
    assert g["vals"].tobytes() == np.asarray(vals).tobytes()


def _load(e, M, rows, cols, vals, cutoff=0.0, fuzz=0):
    """Loads and reduces; returns the pairs of R, from the oracle's flags."""
    e.set_overlaps(M, rows, cols, vals)
    e.transitive_reduction(cutoff, fuzz)
    return su.r_pairs(M, rows, cols, vals, cutoff, fuzz)


def _resolve(e, M, R, rounds):
    """resolve_stars on the engine's S equals the restatement on the S exported before the call.  Returns (stats, restatement's result)."""
    g = e.export_string_graph()
    f0 = e.export_read_flags(M)
    want = su.resolve_stars(M, g["rows"], g["cols"], g["vals"], R, rounds)
    st = e.resolve_stars(rounds)
    for k in su.STATS:
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
def test_the_rule_one_clause_per_case_and_a_second_call(eng, name):
    case = CASES[name]
    M, rows, cols, vals = su.case_overlaps(case, np.random.default_rng(3), extra_reads=2)      # two isolated reads behind the graph
    for rounds in (1, 64):
        R = _load(eng, M, rows, cols, vals)
        st, want = _resolve(eng, M, R, rounds)
        if rounds == 64:
            flags = eng.export_read_flags(M)
            assert set(np.flatnonzero(flags == 32).tolist()) == case["removed"] and flags.sum() == 32 * len(case["removed"])
            assert st["centres"] == case["centres"] and (st["pairs0"], st["pairs1"], st["pairs2"], st["pairs3"]) == case["by_e"]
            assert st["rounds_run"] == case["moves"] + 1 and st["reads_removed"] == len(case["removed"])
            after = np.bincount(eng.export_string_graph()["cols"], minlength=M)
            for v, d in case["deg_after"].items():
                assert after[v] == d
        st2, _ = _resolve(eng, M, R, 64)                         # a second call goes on from there, and after it a third finds a fixed point
        assert st2["reads_removed"] == len(case["removed"]) - st["reads_removed"]
        st3, _ = _resolve(eng, M, R, 1)
        assert st3["reads_removed"] == 0 and st3["rounds_run"] == 1 and st3["nnz_after"] == st2["nnz_after"]


@pytest.mark.parametrize("K", [2, 4, 5, 9])
def test_chains_of_stars_one_round_short_then_a_second_call_finishes(eng, K):
    assert SG_BATCH == 4
    case = CASES["chain_of_%d_stars_needs_%d_rounds" % (K, K)]
    cs, ws = case["chain"]
    M, rows, cols, vals = su.case_overlaps(case, np.random.default_rng(K))
    R = _load(eng, M, rows, cols, vals)
    st, _ = _resolve(eng, M, R, K - 1)
    assert st["reads_removed"] == K - 1 and st["rounds_run"] == K - 1 and np.flatnonzero(eng.export_read_flags(M)).tolist() == sorted(ws[:K - 1])
    st, _ = _resolve(eng, M, R, 64)
    assert st["reads_removed"] == 1 and st["rounds_run"] == 2 and np.flatnonzero(eng.export_read_flags(M)).tolist() == sorted(ws)
    R = _load(eng, M, rows, cols, vals)
    st, _ = _resolve(eng, M, R, K)                              # exactly as many rounds as remove something: the round that finds nothing is not run
    assert st["reads_removed"] == K and st["rounds_run"] == K and st["centres"] == K
    R = _load(eng, M, rows, cols, vals)
    st, _ = _resolve(eng, M, R, 64)
    assert st["reads_removed"] == K and st["rounds_run"] == K + 1


@pytest.mark.parametrize("length", su.LOOKUP_LENGTHS)
def test_the_lookup_at_the_edges_of_the_searched_row(eng, length):
    """The searched row of R has `length` entries and the other read's length + 7; the sought column is first, last, absent below the
    first, absent above the last, absent between two present ones; the searched read is the smaller or the larger of the two.  (A row of
    length 1 cannot be searched, and one of length 2 cannot hold the key: star_util.lookup_case says why.)"""
    for place in su.LOOKUP_PLACES:
        for short in (0, 1):
            if place in ("first", "last") and length < 3:
                continue
            M, rows, cols, vals, info = su.lookup_case(length, place, short)
            R = _load(eng, M, rows, cols, vals)
            st, _ = _resolve(eng, M, R, 1)
            assert st["centres"] == 1 and st["pairs1"] == int(info["present"]) and st["pairs0"] == 1 - int(info["present"]), (length, place, short, st)
            assert np.flatnonzero(eng.export_read_flags(M)).tolist() == ([info["odd"]] if info["present"] else [])


@pytest.mark.parametrize("seed", SEEDS)
def test_random_graphs_with_both_images(eng, seed):
    M, rows, cols, vals = su.random_stars(seed)
    for rounds in (1, 64):
        R = _load(eng, M, rows, cols, vals)
        _resolve(eng, M, R, rounds)
        st2, _ = _resolve(eng, M, R, 64)
        st3, _ = _resolve(eng, M, R, 64)
        assert st3["reads_removed"] == 0


@pytest.mark.parametrize("seed", SEEDS[:12])
def test_random_graphs_with_one_image_entries(eng, seed):
    """A twelfth of the pairs has directionT -1 and the reduction keeps one image of it: the contract there is what the statements give on
    the columns as they are, and the restatement says what that is."""
    M, rows, cols, vals = su.random_stars(seed, p_one_image=0.08)
    R = _load(eng, M, rows, cols, vals)
    g = eng.export_string_graph()
    assert set(zip(g["rows"].tolist(), g["cols"].tolist())) != set(zip(g["cols"].tolist(), g["rows"].tolist()))
    _resolve(eng, M, R, 64)
    _resolve(eng, M, R, 64)


@functools.lru_cache(maxsize=None)
def _planted(seed, n_paths, length, n, gap=4):
    rng = np.random.default_rng(seed)
    M, rows, cols, vals = su.long_paths(rng, n_paths, length)
    return su.plant_stars(rng, M, rows, cols, vals, n, gap=gap)


@pytest.mark.parametrize("nnz", [23 * SG_TILE - 1, 23 * SG_TILE, 23 * SG_TILE + 1, 3 * SCAN_TILE - 1, 3 * SCAN_TILE, 3 * SCAN_TILE + 1])
def test_planted_stars_with_nnz_at_the_block_sizes_of_scan_and_compaction(eng, nnz):
    """About 3000 reads: five paths with 100 planted stars, and one more path whose length sets nnz(S) on, one below and one above a multiple
    of SG_TILE (k_sg_scatter's tile and the flat kernels' workgroup) that is none of the scan's tile, and of SCAN_TILE.  An odd nnz comes
    from one pair whose directionT is -1: the reduction keeps one image of it.  M is no multiple of 256."""
    assert SG_TILE == 256 and SCAN_TILE == 2048 and (23 * SG_TILE) % SCAN_TILE != 0
    odd = nnz % 2
    M, rows, cols, vals, centres, w = _planted(31, 5, 500, 100)
    in_S = int((vals["direction"] != -1).sum())
    extra = (nnz + odd) // 2 - in_S - odd                       # pairs of the last path
    assert extra >= 1
    M2 = M + extra + 1 + 2 * odd
    assert M2 % 256 != 0
    edges = {(int(r), int(c)): v for r, c, v in zip(rows, cols, vals)}
    rng = np.random.default_rng(nnz)
    for i in range(extra):
        o = cu.edge(rng, 20, 20); o["suffix"] = 7; o["suffixT"] = 6
        edges[(M + i, M + i + 1)] = o
    if odd:
        edges[(M2 - 2, M2 - 1)] = cu.edge(rng, 20, 20, directionT=-1)
    r2, c2, v2 = cu.upper(edges)
    R = _load(eng, M2, r2, c2, v2)
    assert eng.export_string_graph()["n"] == nnz
    st, _ = _resolve(eng, M2, R, 64)
    assert st["pairs1"] == 100 and st["centres"] == 100 and st["reads_removed"] == 100 and st["nnz_after"] == nnz - 400 and st["rounds_run"] == 2
    assert set(np.flatnonzero(eng.export_read_flags(M2) == 32).tolist()) == set(w.tolist())


def test_40000_reads_with_2000_planted_stars(eng):
    M, rows, cols, vals, centres, w = _planted(32, 20, 1800, 2000)
    assert M == 40000
    R = _load(eng, M, rows, cols, vals)
    st, _ = _resolve(eng, M, R, 64)
    assert st["pairs1"] == 2000 and st["reads_removed"] == 2000 and st["entries_removed"] == 8000 and st["centres"] == 2000 and st["rounds_run"] == 2
    assert (eng.export_read_flags(M)[w] == 32).all()
    st2, _ = _resolve(eng, M, R, 64)
    assert st2["reads_removed"] == 0 and st2["centres"] == 0


def test_the_pair_comes_from_the_reduction_itself(eng):
    """layout_stars: the pair of the two path neighbours is a transitive entry that the device's own reduction removes from S and keeps in R."""
    for seed, M0, every in ((0, 5, None), (3, 400, range(5, 395, 10))):
        M, rows, cols, vals, centres, w = su.layout_stars(seed, M=M0, every=every)
        R = _load(eng, M, rows, cols, vals, 0.65, 1000)
        want_S, want_flags, _ = po.string_graph(M, rows, cols, vals, 0.65, 1000)
        _same_S(eng.export_string_graph(), want_S["rows"], want_S["cols"], want_S["vals"])
        assert (eng.export_read_flags(M) == want_flags).all()
        st, _ = _resolve(eng, M, R, 64)
        assert st["pairs1"] >= (1 if every is None else 30) and st["reads_removed"] == st["pairs1"]
        assert set(np.flatnonzero(eng.export_read_flags(M) & 32).tolist()) <= set(w.tolist())


def test_one_context_over_graphs_of_changing_size():
    """A graph whose reduction keeps no pair after a large one, and the reverse: with no kept pair tr_ptr is not written, and the pointers
    of the earlier, larger graph must not be read.  The small graph between them has the same reads under other pairs."""
    e = elba_amd.Engine(17, 2, 8)
    big = _planted(32, 20, 1800, 2000)[:4]
    small = su.case_overlaps(CASES["e1_pair_01_odd_arm_in_slot_2"], np.random.default_rng(1))
    # every pair failed: R is empty, S is empty
    none = (big[0], big[1], big[2], big[3].copy())
    none[3]["passed"] = 0
    for (M, rows, cols, vals), n in ((big, 2000), (small, 1), (none, 0), (small, 1), (big, 2000), (none, 0)):
        R = _load(e, M, rows, cols, vals)
        assert (len(R) == 0) == (n == 0)
        st, _ = _resolve(e, M, R, 64)
        assert st["pairs1"] == n and (st["nnz_before"] == 0) == (n == 0)
    e.close()


def test_the_same_S_under_an_R_that_lost_the_pairs():
    """S has no entry when R has none, so a call never looks anything up behind a reduction that kept no pair.  The nearest thing with an S
    to look at: the same reads and the same S, reduced again from overlaps without the six R-only pairs.  With the R of the reduction
    before, every star would still be e = 1."""
    e = elba_amd.Engine(17, 2, 8)
    M, rows, cols, vals, centres, w = _planted(33, 2, 60, 6)
    R = _load(e, M, rows, cols, vals)
    st, _ = _resolve(e, M, R, 64)
    assert st["pairs1"] == 6
    ronly = vals["direction"] == -1
    R = _load(e, M, rows[~ronly], cols[~ronly], vals[~ronly])   # the same S, an R without the six pairs
    st, _ = _resolve(e, M, R, 64)
    assert st["centres"] == 6 and st["pairs0"] == 6 and st["reads_removed"] == 0
    e.close()


def test_after_release_workspace_the_result_is_the_same():
    e = elba_amd.Engine(17, 2, 8)
    M, rows, cols, vals, centres, w = _planted(31, 5, 500, 100)
    R = _load(e, M, rows, cols, vals)
    e.release_workspace()
    st, _ = _resolve(e, M, R, 64)
    assert st["pairs1"] == 100 and st["reads_removed"] == 100
    e.release_workspace()
    st, _ = _resolve(e, M, R, 64)
    assert st["reads_removed"] == 0
    e.close()


def test_without_S_the_call_is_refused():
    e = elba_amd.Engine(17, 2, 8)
    L = e.L
    cfg = capi.StarCfg(1, (C.c_int32 * 3)(0, 0, 0))
    st = capi.StarStats()
    assert L.elba_resolve_stars(e.h, C.byref(cfg), C.byref(st)) == 5                  # no S
    M, rows, cols, vals = su.case_overlaps(CASES["e1_pair_01_odd_arm_in_slot_2"], np.random.default_rng(2))
    e.set_overlaps(M, rows, cols, vals)
    assert L.elba_resolve_stars(e.h, C.byref(cfg), C.byref(st)) == 5                  # an edge list is not an S
    _load(e, M, rows, cols, vals)
    e.set_overlaps(M, rows, cols, vals)                         # a new edge list after the reduction: the S is gone
    assert L.elba_resolve_stars(e.h, C.byref(cfg), C.byref(st)) == 5
    e.close()


def test_prune_reads_after_the_reduction_leaves_no_S():
    m = util.golden_meta()["small_err"][0]
    packed, off, lens = po.pack_reads(util.read_fasta(os.path.join(util.GOLDEN, "small_err.fa")))
    e = elba_amd.Engine(m["k"], m["lower"], m["upper"])
    e.set_reads(packed, off, lens)
    e.count_kmers(); e.create_kmer_matrix(); e.create_seed_matrix()
    e.align_seeds()
    e.transitive_reduction(0.65, 1000)
    assert e.resolve_stars(1)["nreads"] == len(lens)
    e.read_pileup()
    e.prune_reads(1)
    cfg = capi.StarCfg(1, (C.c_int32 * 3)(0, 0, 0))
    assert e.L.elba_resolve_stars(e.h, C.byref(cfg), None) == 5
    e.close()


def test_errors_leave_S_flags_and_contigs_untouched():
    e = elba_amd.Engine(17, 2, 8)
    L = e.L
    st = capi.StarStats()
    rng = np.random.default_rng(2)
    M, rows, cols, vals = su.case_overlaps(CASES["e1_pair_01_odd_arm_in_slot_2"], rng)
    packed, off, lens = cu.random_packed(rng, M, 20, 40)
    e.set_reads(packed, off, lens)
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

    assert L.elba_resolve_stars(e.h, None, C.byref(st)) == 1
    unchanged()
    for rounds, res in ((0, (0, 0, 0)), (-1, (0, 0, 0)), (65, (0, 0, 0)), (1 << 20, (0, 0, 0)), (1, (1, 0, 0)), (1, (0, 7, 0)), (1, (0, 0, -1)), (64, (0, 0, 1))):
        bad = capi.StarCfg(rounds, (C.c_int32 * 3)(*res))
        assert L.elba_resolve_stars(e.h, C.byref(bad), C.byref(st)) == 1, (rounds, res)
        unchanged()
    cfg = capi.StarCfg(64, (C.c_int32 * 3)(0, 0, 0))
    assert L.elba_resolve_stars(e.h, C.byref(cfg), None) == 0                          # stats are optional; 64 rounds are accepted
    assert e.export_string_graph()["n"] == g["n"] - 4           # the odd arm, two pairs
    with pytest.raises(elba_amd.ElbaError) as err:              # contigs made before are invalid after ELBA_OK
        e.export_contigs()
    assert err.value.status == 5
    e.close()


def test_empty_graph_and_context_without_reads(eng):
    z = np.zeros(0, dtype=po.OVERLAP_DTYPE)
    for M in (5, 0):
        R = _load(eng, M, np.zeros(0, np.int64), np.zeros(0, np.int64), z)
        for rounds in (1, 64):
            st, _ = _resolve(eng, M, R, rounds)
            assert st["nnz_after"] == 0 and st["reads_removed"] == 0 and st["nreads"] == M and st["centres"] == 0 and st["rounds_run"] == 1
        assert eng.export_string_graph()["n"] == 0


def test_the_five_cleaning_calls_in_two_orders(eng):
    """A star hidden behind a tip, beside an H, a bubble and a branching read end: each of the five calls is held against its restatement on
    the S the one before left, with resolve_stars first and with resolve_stars last."""
    g = su.StarGraph()
    u, arms = su._star(g, tails=(4, 4, 4), pairs=[(0, 1)])
    tip = g.arm(arms[0][0], 1)
    a, b, ch, fl = br._h(g, 1, (3, 3, 3, 3))
    bu._bubble(g, [1, 2])
    M, rows, cols, vals = g.overlaps(np.random.default_rng(6))
    vals["score"] = np.random.default_rng(7).integers(20, 100, len(vals))
    for first in ("stars", "others"):
        R = _load(eng, M, rows, cols, vals)
        if first == "stars":
            st, _ = _resolve(eng, M, R, 64)
            # the tip hides the star; the two anchors of the H and the two ends of the bubble are centres without a pair in R
            assert st["pairs1"] == 0 and st["centres"] == st["pairs0"] == 4 and st["reads_removed"] == 0
        S = eng.export_string_graph()
        want = tu.clip_tips(M, S["rows"], S["cols"], S["vals"], 1, 64)
        ts = eng.clip_tips(1, 64)
        assert all(ts[k] == want[4][k] for k in tu.STATS) and ts["reads_removed"] == 1
        if first == "stars":
            st, _ = _resolve(eng, M, R, 64)
            assert st["pairs1"] == 1 and st["reads_removed"] == 1
        S = eng.export_string_graph()
        want = bu.pop_bubbles(M, S["rows"], S["cols"], S["vals"], 3, 64)
        bs = eng.pop_bubbles(3, 64)
        assert all(bs[k] == want[4][k] for k in bu.STATS) and bs["reads_removed"] == 1
        _same_S(eng.export_string_graph(), want[0], want[1], want[2])
        S = eng.export_string_graph()
        want = wu.cut_weak(M, S["rows"], S["cols"], S["vals"], wu.Q07)
        ws = eng.cut_weak_overlaps(0.7)
        assert all(ws[k] == want[3][k] for k in wu.STATS)
        _same_S(eng.export_string_graph(), want[0], want[1], want[2])
        S = eng.export_string_graph()
        want = br.cut_bridges(M, S["rows"], S["cols"], S["vals"], 1, 3)
        cs = eng.cut_bridges(1, 3)
        assert all(cs[k] == want[4][k] for k in br.STATS)
        _same_S(eng.export_string_graph(), want[0], want[1], want[2])
        st, _ = _resolve(eng, M, R, 64)                         # resolve_stars goes on from the S of the other four, whatever they left
        f = eng.export_read_flags(M)
        assert f[tip[0]] == 4 and (f & 32).sum() // 32 == (f == 32).sum()
        S = eng.export_string_graph()                           # and clip_tips goes on from the resolved S
        want = tu.clip_tips(M, S["rows"], S["cols"], S["vals"], 3, 64)
        ts = eng.clip_tips(3, 64)
        assert all(ts[k] == want[4][k] for k in tu.STATS)
        _same_S(eng.export_string_graph(), want[0], want[1], want[2])


@pytest.mark.parametrize("seed", SEEDS[:8])
def test_simplify_graph_with_stars_against_the_restated_loop(eng, seed):
    M, rows, cols, vals = su.random_stars(seed)
    vals["score"] = np.random.default_rng(seed + 7).integers(-3, 12, len(vals))
    for ratio, bridges, stars in ((None, None, True), (0.7, (1, 2), 2), (None, (1, 2), 64)):
        R = _load(eng, M, rows, cols, vals)
        S = eng.export_string_graph()
        want = su.simplify(M, S["rows"], S["cols"], S["vals"], R, 2, 3, stars=64 if stars is True else stars, q16=None if ratio is None else wu.Q07, bridges=bridges)
        got = eng.simplify_graph(2, 3, min_overlap_ratio=ratio, bridges=bridges, stars=stars)
        assert len(got) == len(want[4])
        for p, wp in zip(got, want[4]):
            assert len(p) == len(wp) == 3 + (ratio is not None) + (bridges is not None)
            assert all(p[0][k] == wp[0][k] for k in tu.STATS) and all(p[1][k] == wp[1][k] for k in bu.STATS) and all(p[-1][k] == wp[-1][k] for k in su.STATS)
            assert bridges is None or all(p[-2][k] == wp[-2][k] for k in br.STATS)
            assert ratio is None or all(p[2][k] == wp[2][k] for k in wu.STATS)
        _same_S(eng.export_string_graph(), want[0], want[1], want[2])
        assert (eng.export_read_flags(M) == want[3]).all()


def test_simplify_graph_without_stars_does_what_it_did(eng):
    g = su.StarGraph()
    u, arms = su._star(g, tails=(4, 4, 4), pairs=[(0, 1)])
    tip = g.arm(arms[0][0], 1)
    M, rows, cols, vals = g.overlaps(np.random.default_rng(7))
    _load(eng, M, rows, cols, vals)
    got = eng.simplify_graph(1, 3, stars=True)
    assert len(got) == 2 and all(len(p) == 3 for p in got) and got[0][0]["reads_removed"] == 1 and got[0][2]["pairs1"] == 1 and got[1][2]["reads_removed"] == 0
    f = eng.export_read_flags(M)
    assert f[tip[0]] == 4 and f[arms[2][0]] == 32 and f.sum() == 36
    _load(eng, M, rows, cols, vals)
    assert len(eng.simplify_graph(1, 3, passes=1, stars=1)) == 1                               # `passes` bounds it
    for args, kw in (((1, 3), {}), ((1, 3, 16, None, None), {}), ((1, 3), dict(stars=None)), ((1, 3), dict(stars=False))):
        _load(eng, M, rows, cols, vals)
        S = eng.export_string_graph()
        want = bu.simplify(M, S["rows"], S["cols"], S["vals"], 1, 3)
        got = eng.simplify_graph(*args, **kw)
        assert len(got) == len(want[4]) and all(len(p) == len(wp) == 2 for p, wp in zip(got, want[4]))
        for p, wp in zip(got, want[4]):
            assert all(p[0][k] == wp[0][k] for k in tu.STATS) and all(p[1][k] == wp[1][k] for k in bu.STATS)
        _same_S(eng.export_string_graph(), want[0], want[1], want[2])
        assert (eng.export_read_flags(M) == want[3]).all() and eng.export_read_flags(M)[arms[2][0]] == 0      # the star is still there


def test_what_it_is_for_a_star_is_one_contig_not_three():
    """The star with reads on the context: before the call three contigs and a branch; after it the whole path as one contig, byte for byte
    what contig_util makes of the resolved S, beside the stray read's own tail; with singletons asked for the odd arm does not come back."""
    g = su.StarGraph()
    u, arms = su._star(g, tails=(4, 5, 3), pairs=[(0, 1)])
    rng = np.random.default_rng(4)
    M, rows, cols, vals = g.overlaps(rng)
    packed, off, lens = cu.random_packed(rng, M, 20, 40)
    seqs = cu.seqs_of(packed, off, lens)
    e = elba_amd.Engine(17, 2, 8)
    e.set_reads(packed, off, lens)
    R = _load(e, M, rows, cols, vals)
    st0 = e.generate_contigs()
    assert st0["contigs"] == 3 and st0["branches"] == 1
    st, want = _resolve(e, M, R, 1)
    assert st["pairs1"] == 1 and st["reads_removed"] == 1
    with pytest.raises(elba_amd.ElbaError) as err:              # the contigs of the unresolved graph are gone
        e.export_contigs()
    assert err.value.status == 5
    contigs, chains, _, cst = cu.generate_contigs(M, want[0], want[1], want[2], seqs)
    w = arms[2][0]
    for single in (False, True):
        st1 = e.generate_contigs(singletons=single)
        got = e.export_contigs()
        assert st1["branches"] == 0 and got["n"] == 2 and st1["contigs"] == 2 and list(got["seqs"]) == list(contigs)
        assert got["chain_read"].tolist() == [v for chain in chains for v, _, _ in chain]
        assert got["chain_prefix"].tolist() == [p for chain in chains for _, p, _ in chain] and got["chain_strand"].tolist() == [s for chain in chains for _, _, s in chain]
        assert w not in got["chain_read"].tolist()
    sets = [set(got["chain_read"][int(got["chain_off"][i]):int(got["chain_off"][i + 1])].tolist()) for i in range(2)]
    assert sets == [{u} | set(arms[0]) | set(arms[1]), set(arms[2][1:])]      # the whole path through u, and what lay behind the stray read
    e.close()
