"""-m gpu: elba_clip_tips (elba_amd/csrc/tips.hip) against the restatement of its rule in tip_util.py: every entry of the clipped S in
order, every field, the read flags and the stats, exactly.  Graphs are loaded with elba_set_overlaps with suffixes the reduction does
not remove at fuzz 0 (every suffix in [5, 9]: a two-edge walk is at least 10), which each test asserts from the exported S first."""
import ctypes as C
import functools

import numpy as np
import pytest

import contig_util as cu
import elba_amd
import rounds_util as ru
import string_graph_util as sg
import tip_util as tu
from elba_amd import capi
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

CASES = tu.hand_cases()


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


def _clip(e, M, mx, rounds=1):
    """clip_tips on the engine's S equals the restatement on the S exported before the call.  Returns (stats, restatement's result)."""
    g = e.export_string_graph()
    f0 = e.export_read_flags(M)
    want = tu.clip_tips(M, g["rows"], g["cols"], g["vals"], mx, rounds)
    st = e.clip_tips(mx, rounds)
    for k in tu.STATS:
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
    st, want = _clip(eng, M, case["max"], case["rounds"])
    flags = eng.export_read_flags(M)
    assert set(np.flatnonzero(flags == 4).tolist()) == case["removed"] and st["rounds_run"] == case["rounds_run"]
    assert st["spared_anchors"] == len(case["spared"]) and st["reads_removed"] == len(case["removed"])
    after = np.bincount(eng.export_string_graph()["cols"], minlength=M)
    for v, d in case["deg_after"].items():
        assert after[v] == d


def test_cycle_with_one_tip_becomes_a_circular_contig():
    case = CASES["cycle_with_one_tip"]
    rng = np.random.default_rng(4)
    M, rows, cols, vals = tu.case_overlaps(case, rng)
    packed, off, lens = cu.random_packed(rng, M, 20, 40)
    e = elba_amd.Engine(17, 2, 8)
    e.set_reads(packed, off, lens)
    _load(e, M, rows, cols, vals)
    st0 = e.generate_contigs(circular=True)
    assert st0["cycles"] == 0 and (e.export_contigs()["kinds"] == 1).sum() == 0
    _clip(e, M, case["max"], case["rounds"])
    with pytest.raises(elba_amd.ElbaError) as err:              # the contigs of the unclipped graph are gone
        e.export_contigs()
    assert err.value.status == 5
    st1 = e.generate_contigs(circular=True)
    got = e.export_contigs()
    assert st1["cycles"] == 1 and got["n"] == 1 and got["kinds"].tolist() == [1] and st1["contig_reads"] == 5
    e.close()


def test_isolated_and_flagged_reads_beside_tips(eng):
    """A contained read and a bad read hang on the tip's dead end in the input; the prunes take them, the dead end stays one."""
    g, b, arms = tu._y([1, 5, 6])
    d = arms[0][0]
    rng = np.random.default_rng(5)
    M, rows, cols, vals = g.overlaps(rng, M=g.n + 3)
    iso, w, z = g.n, g.n + 1, g.n + 2
    extra = {}
    extra[(d, w)] = cu.edge(rng, 20, 20); extra[(d, w)]["containedT"] = 1
    extra[(d, z)] = cu.edge(rng, 20, 20); extra[(d, z)]["passed"] = 0
    edges = {(int(r), int(c)): v for r, c, v in zip(rows, cols, vals)}
    edges.update(extra)
    r2, c2, v2 = cu.upper(edges)
    s = _load(eng, M, r2, c2, v2, cutoff=0.5, kept=False)
    assert s["nnz"] == 2 * len(rows) and s["bad_reads"] == 1 and s["contained_reads"] == 1
    f0 = eng.export_read_flags(M)
    assert f0[z] == 1 and f0[w] == 2 and f0[iso] == 0 and f0[d] == 0
    st, _ = _clip(eng, M, 1)
    f = eng.export_read_flags(M)
    assert f[d] == 4 and f[z] == 1 and f[w] == 2 and f[iso] == 0 and st["reads_removed"] == 1


def _hub(n_tips, tip_len=1):
    """A read on a 4-cycle with n_tips chains of tip_len reads: n_tips dead ends, all tips, degree n_tips + 2."""
    g = tu.Graph()
    cyc = g.chain(g.new(4), closed=True)
    for _ in range(n_tips):
        g.arm(cyc[0], tip_len)
    return g, cyc[0]


@pytest.mark.parametrize("n", [255, 256, 257])
def test_dead_ends_all_tips(eng, n):
    g, b = _hub(n)
    M, rows, cols, vals = g.overlaps(np.random.default_rng(n))
    _load(eng, M, rows, cols, vals)
    st, _ = _clip(eng, M, 1, 2)
    assert st["dead_ends"] == n and st["tips"] == n and st["reads_removed"] == n and st["rounds_run"] == 2 and st["nnz_after"] == 8


@pytest.mark.parametrize("n", [255, 256, 257])
def test_dead_ends_none_a_tip(eng, n):
    """n lollipops: a 4-cycle with a tail of two reads, one more than max_tip_reads."""
    g = tu.Graph()
    for _ in range(n):
        cyc = g.chain(g.new(4), closed=True)
        g.arm(cyc[1], 2)
    M, rows, cols, vals = g.overlaps(np.random.default_rng(n), perm=np.random.default_rng(n + 1).permutation(g.n))
    _load(eng, M, rows, cols, vals)
    st, _ = _clip(eng, M, 1, 2)
    assert st["dead_ends"] == n and st["tips"] == 0 and st["reads_removed"] == 0 and st["rounds_run"] == 1 and st["nnz_after"] == st["nnz_before"]


@pytest.mark.parametrize("M", [1, 64, 65, 65537])
def test_read_counts_at_wavefront_and_block_edges(eng, M):
    z = np.zeros(0, dtype=po.OVERLAP_DTYPE)
    if M == 1:
        _load(eng, 1, np.zeros(0, np.int64), np.zeros(0, np.int64), z)
        st, _ = _clip(eng, 1, 3, 2)
        assert st["nnz_before"] == 0 and st["rounds_run"] == 1
        return
    g, b, arms = tu._y([1, 5, 6])
    d = arms[0][0]
    rest = [v for v in range(g.n) if v not in (b, d)]
    perm = np.zeros(g.n, dtype=np.int64)
    perm[b], perm[d] = 0, M - 1
    perm[rest] = np.arange(M - 1 - len(rest), M - 1)            # the graph's other reads next to the last one, isolated reads between
    Mx, rows, cols, vals = g.overlaps(np.random.default_rng(M), perm=perm, M=M)
    _load(eng, M, rows, cols, vals)
    st, _ = _clip(eng, M, 1)
    assert eng.export_read_flags(M)[M - 1] == 4 and st["reads_removed"] == 1


@pytest.mark.parametrize("mx,gone", [(999, 0), (1000, 1000), (65535, 1000)])
def test_a_tip_of_1000_reads(eng, mx, gone):
    g, b = _hub(1, 1000)
    M, rows, cols, vals = g.overlaps(np.random.default_rng(11), perm=np.random.default_rng(12).permutation(g.n))
    _load(eng, M, rows, cols, vals)
    st, _ = _clip(eng, M, mx)
    assert st["reads_removed"] == gone and st["tips"] == (1 if gone else 0) and st["dead_ends"] == 1


@pytest.mark.parametrize("nnz", [SG_TILE - 2, SG_TILE - 1, SG_TILE, SG_TILE + 1, SG_TILE + 2, SCAN_TILE - 2, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, SCAN_TILE + 2,
                                 2 * SCAN_TILE - 2, 2 * SCAN_TILE - 1, 2 * SCAN_TILE, 2 * SCAN_TILE + 1, 2 * SCAN_TILE + 2])
def test_nnz_at_the_block_sizes_of_scan_and_compaction(eng, nnz):
    """nnz(S) round SG_TILE (= SG_THREADS: k_sg_scatter's tile, the flat kernels' workgroup) and the scan's SCAN_TILE.  The scan and
    k_tip_keep run over nnz + 1 elements, so nnz = tile - 1 gives them exactly a tile.  An odd nnz comes from one pair whose directionT is -1:
    the reduction keeps one image of it, a column of one entry whose row has an empty column (a dead end that reaches no anchor)."""
    assert SG_TILE == 256 and SG_THREADS == 256 and SCAN_TILE == 2048
    odd = nnz % 2
    g, b, arms = tu._y([1, 2, (nnz - odd) // 2 - 3])
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
    st, _ = _clip(eng, M, 2, 3)
    assert st["reads_removed"] == 3 and st["nnz_after"] == nnz - 6 and st["rounds_run"] == 2 and st["dead_ends"] == 3 + odd


@functools.lru_cache(maxsize=None)
def _layout_with_tips(seed, M, ntips):
    rng = np.random.default_rng(seed)
    rows, cols, vals = sg.layout_overlaps(rng, M, 8)
    deg, flags = sg.kept_degrees(M, rows, cols, vals, 0.65)
    anchors = np.sort(rng.choice(np.flatnonzero((flags == 0) & (deg > 0)), ntips, replace=False))
    lengths = rng.integers(1, 4, ntips)
    M2, r2, c2, v2, planted = tu.plant_tips(rng, M, rows, cols, vals, anchors, lengths)
    return M2, r2, c2, v2, planted, anchors


def test_empty_graph_and_context_without_reads(eng):
    z = np.zeros(0, dtype=po.OVERLAP_DTYPE)
    for M in (5, 0):
        _load(eng, M, np.zeros(0, np.int64), np.zeros(0, np.int64), z)
        st, _ = _clip(eng, M, 3, 4)
        assert st["nnz_after"] == 0 and st["reads_removed"] == 0 and st["rounds_run"] == 1 and st["nreads"] == M
        assert eng.export_string_graph()["n"] == 0


def test_one_context_over_graphs_of_changing_size():
    e = elba_amd.Engine(17, 2, 8)
    z = np.zeros(0, dtype=po.OVERLAP_DTYPE)
    big = _layout_with_tips(1, 40000, 500)
    small = tu.case_overlaps(CASES["two_tips_one_long_arm"], np.random.default_rng(1))
    for M, rows, cols, vals, kept, fuzz in ((big[0], big[1], big[2], big[3], False, 1000), small + (True, 0), (7, np.zeros(0, np.int64), np.zeros(0, np.int64), z, True, 0),
                                            (big[0], big[1], big[2], big[3], False, 1000)):
        _load(e, M, rows, cols, vals, cutoff=0.65 if not kept else 0.0, fuzz=fuzz, kept=kept)
        st, _ = _clip(e, M, 3, 2)
        if M == big[0]:
            assert st["reads_removed"] >= len(big[4]) // 2
    # a second call on the clipped graph clips from there: after rounds to the end, nothing is left to remove
    _clip(e, big[0], 3, 64)
    st, _ = _clip(e, big[0], 3, 64)
    assert st["reads_removed"] == 0 and st["rounds_run"] == 1 and st["nnz_after"] == st["nnz_before"]
    e.close()


def test_errors_leave_S_untouched():
    e = elba_amd.Engine(17, 2, 8)
    L = e.L
    cfg = capi.TipCfg(3, 1, (C.c_int32 * 2)(0, 0))
    st = capi.TipStats()
    assert L.elba_clip_tips(e.h, C.byref(cfg), C.byref(st)) == 5                      # no S
    M, rows, cols, vals = tu.case_overlaps(CASES["two_tips_one_long_arm"], np.random.default_rng(2))
    e.set_overlaps(M, rows, cols, vals)
    assert L.elba_clip_tips(e.h, C.byref(cfg), C.byref(st)) == 5                      # an edge list is not an S
    _load(e, M, rows, cols, vals)
    g = e.export_string_graph()
    f = e.export_read_flags(M)

    def unchanged():
        _same_S(e.export_string_graph(), g["rows"], g["cols"], g["vals"])
        assert (e.export_read_flags(M) == f).all()

    assert L.elba_clip_tips(e.h, None, C.byref(st)) == 1
    unchanged()
    for mx, rounds, res in ((0, 1, (0, 0)), (65536, 1, (0, 0)), (3, 0, (0, 0)), (3, 65, (0, 0)), (3, 1, (1, 0)), (3, 1, (0, 7)), (-1, 1, (0, 0))):
        bad = capi.TipCfg(mx, rounds, (C.c_int32 * 2)(*res))
        assert L.elba_clip_tips(e.h, C.byref(bad), C.byref(st)) == 1, (mx, rounds, res)
        unchanged()
    assert L.elba_clip_tips(e.h, C.byref(cfg), None) == 0                              # stats are optional
    assert e.export_string_graph()["n"] == g["n"] - 6
    e.close()


def test_what_it_is_for_planted_tips_do_not_break_contigs():
    """A clean layout path of 3000 reads; tips of 1 to 3 reads planted at interior reads.  Unclipped, the contigs break at every planted
    anchor; after clip_tips(3, 2) they are, byte for byte, those of the graph without the tips."""
    M, L = 3000, 400
    rows, cols, vals = sg.layout_overlaps(np.random.default_rng(21), M, 8, L=L, p_fail=0.0, p_nodir=1e-9, p_contained=0.0, jitter=0)
    rng = np.random.default_rng(22)
    anchors = np.arange(50, M - 50, 97)
    lengths = 1 + np.arange(len(anchors)) % 3
    M2, r2, c2, v2, planted = tu.plant_tips(rng, M, rows, cols, vals, anchors, lengths)
    packed, off, lens = cu.random_packed(rng, M2, L, L)
    nb = int(off[M - 1]) + (L + 3) // 4
    base_packed = np.concatenate([packed[:nb], np.zeros(16, np.uint8)])

    e0 = elba_amd.Engine(17, 2, 8)
    e0.set_reads(base_packed, off[:M], lens[:M])
    _load(e0, M, rows, cols, vals, cutoff=0.65, fuzz=1000, kept=False)
    g0 = e0.export_string_graph()
    assert g0["n"] == 2 * (M - 1) and np.bincount(g0["cols"], minlength=M).max() == 2          # one clean path
    st0 = e0.generate_contigs()
    base = e0.export_contigs()
    assert st0["contigs"] == 1 and st0["contig_reads"] == M
    e0.generate_contigs(singletons=True)
    base_single = e0.export_contigs()
    e0.close()

    e = elba_amd.Engine(17, 2, 8)
    e.set_reads(packed, off, lens)
    _load(e, M2, r2, c2, v2, cutoff=0.65, fuzz=1000, kept=False)
    assert e.export_string_graph()["n"] == g0["n"] + 2 * len(planted)
    st = e.generate_contigs()
    assert st["branches"] == len(anchors) and st["contigs"] >= len(anchors) + 1               # broken at every planted anchor
    ts, _ = _clip(e, M2, 3, 2)
    assert ts["tips"] == len(anchors) and ts["reads_removed"] == len(planted) and ts["rounds_run"] == 2
    flags = e.export_read_flags(M2)
    assert (flags[planted] == 4).all() and flags.sum() == 4 * len(planted)
    _same_S(e.export_string_graph(), g0["rows"], g0["cols"], g0["vals"])
    for single, want in ((False, base), (True, base_single)):
        e.generate_contigs(singletons=single)
        got = e.export_contigs()
        assert got["n"] == want["n"] == 1 and got["seqs"] == want["seqs"]                      # the clipped reads are not emitted as singletons
        for k in ("chain_read", "chain_prefix", "chain_strand", "kinds"):
            assert (got[k] == want[k]).all(), k
    e.close()


def test_size_300000_reads_with_planted_tips():
    """The layout graph of the string graph's scale tests with 3000 planted tips (and the tips its own failed pairs leave) against the
    restatement; prints the times DESIGN.md quotes."""
    M2, rows, cols, vals, planted, anchors = _layout_with_tips(2, 300000, 3000)
    e = elba_amd.Engine(17, 2, 8)
    s = _load(e, M2, rows, cols, vals, cutoff=0.65, fuzz=1000, kept=False)
    st, want = _clip(e, M2, 3, 2)
    n = st["nnz_before"]
    gbs = (n * 52 + st["nnz_after"] * 52) / (st["ms_compact"] * 1e-3) / 1e9 if st["ms_compact"] > 0 else 0.0
    print("tips300k: nnz %d -> %d, reads_removed %d, tips %d, ms_total %.3f ms_compact %.3f (first round: %.1f GB/s of 52-byte entries read + written), "
          "transitive_reduction ms_total %.3f" % (n, st["nnz_after"], st["reads_removed"], st["tips"], st["ms_total"], st["ms_compact"], gbs, s["ms_total"]))
    assert st["reads_removed"] >= len(planted) // 2 and st["rounds_run"] == 2
    flags = e.export_read_flags(M2)
    kept_anchor = (flags[anchors] == 0) & (np.bincount(want[1], minlength=M2)[anchors] > 0)
    assert kept_anchor.sum() > len(anchors) // 2
    e.close()
