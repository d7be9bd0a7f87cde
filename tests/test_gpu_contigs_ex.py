"""-m gpu: circular and single-read contigs on the GPU (elba_generate_contigs_ex, contig.hip) against the restatement in contig_ex_util.py,
fed with the GPU's own exported S and read flags: every byte of every contig, the chains, the kinds, the read map, the counts.  The graphs
are triangle-free (or planted with weights that make no entry transitive), so S keeps every edge; each test asserts that from the export."""
import ctypes as C

import numpy as np
import pytest

import contig_ex_util as cx
import contig_util as cu
import elba_amd
import hostcpp_util as hu
from elba_amd import capi, formats
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

STATS = ("nreads", "branches", "components", "used_components", "contigs", "cycles", "contig_reads", "bases", "longest")
FLAGS = [0, cx.CIRCULAR, cx.SINGLETONS, cx.CIRCULAR | cx.SINGLETONS]


def _gen(e, flags):
    return e.generate_contigs(circular=bool(flags & cx.CIRCULAR), singletons=bool(flags & cx.SINGLETONS))


def _engine_with(packed, off, lens, rows, cols, vals, fuzz=1000, cutoff=0.0, keeps_all=True):
    e = elba_amd.Engine(17, 2, 8)
    e.set_reads(packed, off, lens)
    e.set_overlaps(len(lens), rows, cols, vals)
    e.transitive_reduction(cutoff, fuzz)
    g = e.export_string_graph()
    if keeps_all:                                                # S is the input, both triangles: its upper triangle, row-major, is the input
        up = np.nonzero(g["rows"] < g["cols"])[0]
        up = up[np.lexsort((g["cols"][up], g["rows"][up]))]
        assert g["n"] == 2 * len(rows) and (g["rows"][up] == rows).all() and (g["cols"][up] == cols).all()
        for f in ("direction", "directionT", "suffix", "suffixT"):
            assert (g["vals"][f][up] == vals[f]).all(), f
    return e, g


def _check(e, g, st, seqs, flags):
    """The GPU's contigs, chains, kinds, read map and counts equal the restatement's on the GPU's exported S and read flags."""
    M = len(seqs)
    rf = e.export_read_flags(M)
    contigs, chains, kinds, read_contig, xst = cx.generate_contigs_ex(M, g["rows"], g["cols"], g["vals"], seqs, flags, rf)
    for k in STATS:
        assert st[k] == xst[k], (k, st, xst)
    got = e.export_contigs()
    assert got["n"] == len(contigs) and got["seqs"] == contigs
    assert got["kinds"].dtype == np.uint8 and got["kinds"].tolist() == kinds
    co = got["chain_off"]
    assert co.tolist() == np.concatenate([[0], np.cumsum([len(c) for c in chains])]).tolist()
    flat = [el for ch in chains for el in ch]
    assert got["chain_read"].tolist() == [r for r, _, _ in flat]
    assert got["chain_prefix"].tolist() == [p for _, p, _ in flat]
    assert got["chain_strand"].tolist() == [s for _, _, s in flat]
    assert (e.export_read_contigs(M) == np.array(read_contig, dtype=np.int64)).all()
    assert e.get_stat("contig_circular") == kinds.count(cx.CIRCLE) and e.get_stat("contig_singletons") == kinds.count(cx.SINGLE)
    assert e.get_stat("contig_count") == len(contigs)
    assert st["ms_total"] > 0 and st["ms_rank"] >= 0
    return contigs, chains, kinds


@pytest.mark.parametrize("M", [60, 3000])
def test_random_string_graphs_under_every_flag_combination(M):
    rng = np.random.default_rng({60: 8061, 3000: 11000}[M])     # seeds whose graphs hold paths, cycles and lonely reads
    seqs = cu.random_reads(rng, M, 1, 120)
    packed, off, lens = cu.pack(seqs)
    rows, cols, vals = cu.random_string_graph(rng, M, lens, n_paths=M // 6, p_extra=0.1)
    e, g = _engine_with(packed, off, lens, rows, cols, vals)
    st0 = e.generate_contigs()                                   # today's call
    today = e.export_contigs()
    want = cu.generate_contigs(M, g["rows"], g["cols"], g["vals"], seqs)
    assert today["seqs"] == want[0] and all(st0[k] == want[3][k] for k in STATS) and st0["cycles"] > 0
    seen = {}
    for flags in FLAGS:
        st = _gen(e, flags)
        contigs, chains, kinds = _check(e, g, st, seqs, flags)
        seen[flags] = set(kinds)
        if flags == 0:                                           # byte for byte what elba_generate_contigs gives
            got = e.export_contigs()
            assert all(st[k] == st0[k] for k in STATS)
            for k in today:
                assert np.array_equal(got[k], today[k]), k
            assert (got["kinds"] == 0).all()
    assert seen == {0: {cx.PATH}, 1: {cx.PATH, cx.CIRCLE}, 2: {cx.PATH, cx.SINGLE}, 3: {cx.PATH, cx.CIRCLE, cx.SINGLE}}
    e.close()


def _edges(rng, x, y, lens):
    """Valid entries for the pairs {x[a], y[a]} of a triangle-free graph, built with numpy (the large graphs): (rows, cols, vals) ascending
    in (row, col), any direction pair, 0 <= suffixT <= len(row read), 0 <= suffix <= len(col read)."""
    x = np.asarray(x, dtype=np.int64); y = np.asarray(y, dtype=np.int64)
    r, c = np.minimum(x, y), np.maximum(x, y)
    order = np.lexsort((c, r))
    r, c = r[order], c[order]
    v = np.zeros(len(r), dtype=po.OVERLAP_DTYPE)
    v["passed"] = 1
    v["direction"] = rng.integers(0, 4, len(r)); v["directionT"] = rng.integers(0, 4, len(r))
    v["suffixT"] = rng.integers(0, np.asarray(lens)[r].astype(np.int64) + 1); v["suffix"] = rng.integers(0, np.asarray(lens)[c].astype(np.int64) + 1)
    return r, c, v


def _rings(rng, M, parts, ids=None):
    """Cycles / paths of the given sizes over ids (default: a random permutation of 0 .. M-1), in that order; the rest stays isolated."""
    ids = rng.permutation(M) if ids is None else np.asarray(ids)
    xs, ys, at = [], [], 0
    for size, cyc in parts:
        seg = ids[at:at + size]; at += size
        xs.append(seg[:-1]); ys.append(seg[1:])
        if cyc:
            xs.append(seg[-1:]); ys.append(seg[:1])
    assert at <= M
    return np.concatenate(xs), np.concatenate(ys)


def _run_rings(rng, M, parts, ids=None, flags=cx.CIRCULAR, lo=4, hi=24):
    packed, off, lens = cu.random_packed(rng, M, lo, hi)
    seqs = cu.seqs_of(packed, off, lens)
    rows, cols, vals = _edges(rng, *_rings(rng, M, parts, ids), lens)
    e, g = _engine_with(packed, off, lens, rows, cols, vals)
    st = _gen(e, flags)
    contigs, chains, kinds = _check(e, g, st, seqs, flags)
    assert st["cycles"] == sum(1 for size, cyc in parts if cyc) == kinds.count(cx.CIRCLE)
    e.close()
    return st, chains, kinds


@pytest.mark.parametrize("size", [4, 5, 64, 65])
def test_cycles_within_and_across_a_wavefront(size):
    """The smallest cycle (4 reads in a triangle-free graph), 5, a full wavefront of reads and one more; three of each, next to a path."""
    rng = np.random.default_rng(size)
    st, chains, kinds = _run_rings(rng, 3 * size + 9, [(size, True), (size, True), (7, False), (size, True)], flags=cx.CIRCULAR | cx.SINGLETONS)
    assert sorted(len(c) for c, k in zip(chains, kinds) if k == cx.CIRCLE) == [size] * 3 and kinds.count(cx.SINGLE) == 2


@pytest.mark.parametrize("M", [4096, 4097])
def test_one_cycle_of_all_reads_at_the_boundary_of_the_round_count(M):
    """2^12 reads take 12 jump rounds, 2^12 + 1 take 13; the cycle's arcs chain over M - 1 steps either way."""
    st, chains, kinds = _run_rings(np.random.default_rng(M), M, [(M, True)])
    assert kinds == [cx.CIRCLE] and len(chains[0]) == M and chains[0][0][0] == 0


def test_one_cycle_of_2_to_the_17_reads():
    M = 1 << 17
    st, chains, kinds = _run_rings(np.random.default_rng(17), M, [(M, True)], lo=4, hi=8)
    assert kinds == [cx.CIRCLE] and st["contig_reads"] == M


def test_a_thousand_small_cycles_next_to_paths_and_branches():
    rng = np.random.default_rng(1000)
    parts = [(int(s), True) for s in rng.integers(4, 10, 1000)] + [(int(s), False) for s in rng.integers(2, 12, 200)]
    used = sum(s for s, _ in parts)
    M = used + 300
    ids = rng.permutation(M)
    packed, off, lens = cu.random_packed(rng, M, 4, 24)
    seqs = cu.seqs_of(packed, off, lens)
    x, y = _rings(rng, M, parts, ids)
    # hubs: each of 60 spare reads joined to three reads of three different parts' interiors: the hub is a branch, and so may its neighbours become
    hubs = ids[used:used + 60]
    starts = np.concatenate([[0], np.cumsum([s for s, _ in parts])])[:-1]
    tgt = rng.choice(len(parts), size=(60, 3), replace=False)
    x = np.concatenate([x, np.repeat(hubs, 3)]); y = np.concatenate([y, ids[starts[tgt.reshape(-1)] + 1]])
    rows, cols, vals = _edges(rng, x, y, lens)
    e, g = _engine_with(packed, off, lens, rows, cols, vals)
    for flags in (cx.CIRCULAR, cx.CIRCULAR | cx.SINGLETONS):
        st = _gen(e, flags)
        contigs, chains, kinds = _check(e, g, st, seqs, flags)
        assert st["branches"] >= 60 and 800 <= kinds.count(cx.CIRCLE) == st["cycles"] < 1000 and kinds.count(cx.PATH) > 200
    e.close()


@pytest.mark.parametrize("case", ["s_is_read_0", "s_in_the_last_reads_cycle", "smaller_neighbour_first_in_the_walk_of_ascending_ids", "descending_ids"])
def test_where_the_start_and_its_neighbours_sit(case):
    """The start read s at read 0; the cycle of read M - 1; and the two ways round: ids ascending along the ring (the smaller neighbour of s
    is its successor in the ring) and descending (it is its predecessor).  In S's columns rows ascend, so the smaller neighbour of s is
    always the first of its two entries (slot 0 on the device); the second-slot case cannot be built through elba_set_overlaps and the
    kernel compares the ids instead of relying on that order.  The export is checked for the order here."""
    rng = np.random.default_rng(3)
    M = 41
    if case == "s_is_read_0":
        ids = np.concatenate([[0, 17, 3, 29, 8], np.setdiff1d(np.arange(M), [0, 17, 3, 29, 8])])
        parts = [(5, True), (6, False), (9, True)]
    elif case == "s_in_the_last_reads_cycle":
        ids = np.concatenate([[40, 36, 38, 37, 39], np.arange(36)])
        parts = [(5, True), (10, False), (8, True)]
    elif case == "descending_ids":
        ids = np.arange(M)[::-1]
        parts = [(7, True), (4, True), (11, True)]
    else:
        ids = np.arange(M)
        parts = [(7, True), (4, True), (11, True)]
    packed, off, lens = cu.random_packed(rng, M, 4, 24)
    seqs = cu.seqs_of(packed, off, lens)
    rows, cols, vals = _edges(rng, *_rings(rng, M, parts, ids), lens)
    e, g = _engine_with(packed, off, lens, rows, cols, vals)
    st = _gen(e, cx.CIRCULAR)
    contigs, chains, kinds = _check(e, g, st, seqs, cx.CIRCULAR)
    circ = [ch for ch, k in zip(chains, kinds) if k == cx.CIRCLE]
    assert len(circ) == sum(1 for _, c in parts if c)
    for ch in circ:
        s, nxt, last = ch[0][0], ch[1][0], ch[-1][0]
        col = g["rows"][g["cols"] == s]
        assert col.tolist() == [nxt, last] and nxt < last           # column s of S: the smaller neighbour first
    if case == "s_is_read_0":
        assert circ[0][0][0] == 0 and [r for r, _, _ in circ[0]] == [0, 8, 29, 3, 17]
    if case == "s_in_the_last_reads_cycle":
        assert [r for r, _, _ in circ[-1]] == [36, 38, 37, 39, 40]
    e.close()


def test_a_cycle_through_a_branch_read_is_todays_path():
    """A ring one of whose reads has a third neighbour: branch removal opens it, and the contig is the one elba_generate_contigs gives."""
    rng = np.random.default_rng(21)
    M = 30
    packed, off, lens = cu.random_packed(rng, M, 4, 24)
    seqs = cu.seqs_of(packed, off, lens)
    ids = rng.permutation(M)
    x, y = _rings(rng, M, [(9, True), (6, True)], ids)
    x = np.concatenate([x, ids[[3]]]); y = np.concatenate([y, ids[[20]]])      # ids[3] on the first ring gets a third neighbour
    rows, cols, vals = _edges(rng, x, y, lens)
    e, g = _engine_with(packed, off, lens, rows, cols, vals)
    e.generate_contigs()
    today = e.export_contigs()
    assert today["n"] == 1 and len(today["chain_read"]) == 8
    st = _gen(e, cx.CIRCULAR)
    contigs, chains, kinds = _check(e, g, st, seqs, cx.CIRCULAR)
    assert sorted(kinds) == [cx.PATH, cx.CIRCLE] and st["branches"] == 1 and st["cycles"] == 1
    assert contigs[kinds.index(cx.PATH)] == today["seqs"][0]
    e.close()


def _genome_engine(rng, parts):
    seqs, edges, info = cx.genome_graph(rng, parts)
    packed, off, lens = cu.pack(seqs)
    rows, cols, vals = cu.upper(edges)
    e, g = _engine_with(packed, off, lens, rows, cols, vals, fuzz=0)
    return e, g, seqs, info


@pytest.mark.parametrize("n", [4, 5, 50, "two_circles_and_a_line"])
def test_circular_genomes_come_back_as_rotations(n):
    """The fixtures of test_contigs_ex_cpu.py through the device: the circular contig has the genome's length exactly and is a rotation of
    it or of its reverse complement, whatever the ids; the linear genome comes back whole."""
    rng = np.random.default_rng(100 * n if isinstance(n, int) else 900)
    parts = [(int(rng.integers(2000, 5001)), n, True)] if isinstance(n, int) else [(3100, 17, True), (2048, 4, True), (4500, 23, False)]
    e, g, seqs, info = _genome_engine(rng, parts)
    st = _gen(e, cx.CIRCULAR | cx.SINGLETONS)
    _check(e, g, st, seqs, cx.CIRCULAR | cx.SINGLETONS)
    got = e.export_contigs()
    rc = e.export_read_contigs(len(seqs))
    assert got["n"] == len(parts)
    for genome, ids, circ in info:
        k = int(rc[ids[0]])
        assert (rc[ids] == k).all() and got["kinds"][k] == (cx.CIRCLE if circ else cx.PATH)
        assert len(got["seqs"][k]) == len(genome)
        assert cx.is_rotation(got["seqs"][k], genome) if circ else got["seqs"][k] in (genome, cu.revcomp(genome))
    e.close()


def test_singletons_isolated_branch_flagged_and_empty_reads():
    rng = np.random.default_rng(31)
    M = 400
    packed, off, lens = cu.random_packed(rng, M, 4, 24)
    ids = rng.permutation(M)
    empty = ids[[285, 286, 287, 300]]                            # three isolated reads and one branch read without bases (their bytes stay unused)
    lens[empty] = 0
    seqs = cu.seqs_of(packed, off, lens)
    parts = [(int(s), bool(c) and s >= 4) for s, c in zip(rng.integers(2, 9, 40), rng.integers(0, 2, 40))]
    assert sum(s for s, _ in parts) <= 280
    x, y = _rings(rng, M, parts, ids)
    hubs = ids[300:320]                                          # branch reads: four neighbours each among the spare reads
    x = np.concatenate([x, np.repeat(hubs, 4)]); y = np.concatenate([y, ids[320:400]])
    rows, cols, vals = _edges(rng, x, y, lens)
    # containment marks on some edges flag one of their reads; PruneFull then takes all of its entries out of S
    marked = rng.choice(len(rows), 25, replace=False)
    vals["containedT"][marked[:15]] = 1; vals["containedQ"][marked[15:]] = 1
    e, g = _engine_with(packed, off, lens, rows, cols, vals, keeps_all=False)
    rf = e.export_read_flags(M)
    gone = (rf[rows] != 0) | (rf[cols] != 0)
    assert 0 < (rf != 0).sum() and gone.any() and g["n"] == 2 * int((~gone).sum())       # S keeps exactly the edges between unflagged reads
    for flags in (cx.SINGLETONS, cx.CIRCULAR | cx.SINGLETONS):
        st = _gen(e, flags)
        contigs, chains, kinds = _check(e, g, st, seqs, flags)
        single = [ch[0][0] for ch, k in zip(chains, kinds) if k == cx.SINGLE]
        deg = np.bincount(g["cols"], minlength=M)
        assert any(deg[v] > 2 for v in single) and any(deg[v] == 0 for v in single) and st["branches"] > 0
        assert not (rf[single] != 0).any() and not (lens[single] == 0).any()
        assert not set(single) & set(empty.tolist()) and (rf[empty] == 0).any()
    e.close()


def test_singletons_without_edges_and_without_reads():
    rng = np.random.default_rng(32)
    packed, off, lens = cu.random_packed(rng, 70, 1, 40)
    seqs = cu.seqs_of(packed, off, lens)
    none = (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, po.OVERLAP_DTYPE))
    e, g = _engine_with(packed, off, lens, *none)
    st = _gen(e, cx.CIRCULAR | cx.SINGLETONS)
    contigs, chains, kinds = _check(e, g, st, seqs, cx.CIRCULAR | cx.SINGLETONS)
    assert contigs == seqs and kinds == [cx.SINGLE] * 70 and st["components"] == 70 and st["used_components"] == 0
    assert _gen(e, cx.CIRCULAR)["contigs"] == 0
    e.close()
    e = elba_amd.Engine(17, 2, 8)                                # M = 0
    e.set_reads(np.zeros(16, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint32))
    e.set_overlaps(0, *none)
    e.transitive_reduction(0.0, 1000)
    for flags in FLAGS:
        st = _gen(e, flags)
        assert st["contigs"] == 0 and st["nreads"] == 0
        got = e.export_contigs()
        assert got["n"] == 0 and got["seqs"] == [] and len(got["kinds"]) == 0
    e.close()


def _cfg_call(e, cfg):
    st = capi.ContigStats()
    return e.L.elba_generate_contigs_ex(e.h, C.byref(cfg) if cfg is not None else None, C.byref(st))


def test_errors_and_invalidation():
    rng = np.random.default_rng(5)
    e, g, seqs, info = _genome_engine(rng, [(2000, 7, True), (1500, 5, False)])
    M = len(seqs)
    with pytest.raises(elba_amd.ElbaError) as x:                 # kinds before any contigs
        e.export_contig_kinds(0)
    assert x.value.status == 5
    st = _gen(e, cx.CIRCULAR)
    contigs, chains, kinds = _check(e, g, st, seqs, cx.CIRCULAR)
    for n in (0, 1, 3):                                          # kinds with a wrong count
        with pytest.raises(elba_amd.ElbaError) as x:
            e.export_contig_kinds(n)
        assert x.value.status == 1
    assert e.export_contig_kinds(2).tolist() == kinds
    # rejected arguments leave no contigs
    for cfg in (capi.ContigCfg(4), capi.ContigCfg(-1), capi.ContigCfg(1, (0, 0, 1)), capi.ContigCfg(0, (1, 0, 0)), None):
        _gen(e, cx.CIRCULAR)
        assert _cfg_call(e, cfg) == 1
        with pytest.raises(elba_amd.ElbaError) as x:
            e.export_contigs()
        assert x.value.status == 5
        assert e.get_stat("contig_circular") == 0 and e.get_stat("contig_singletons") == 0
    # a new S invalidates
    _gen(e, 3)
    e.transitive_reduction(0.0, 0)
    for call in (lambda: e.export_contig_kinds(2), e.export_contigs, lambda: e.export_read_contigs(M)):
        with pytest.raises(elba_amd.ElbaError) as x:
            call()
        assert x.value.status == 5
    # a new read set invalidates
    _gen(e, 3)
    assert e.export_contig_kinds(2).tolist() == kinds
    e.set_reads(*cu.pack(seqs))
    with pytest.raises(elba_amd.ElbaError) as x:
        e.export_contig_kinds(2)
    assert x.value.status == 5
    # a bad prefix on the closing edge only: names (last read, s), leaves no contigs; unchecked where the cycle is not walked
    circle = chains[kinds.index(cx.CIRCLE)]
    last, s = circle[-1][0], circle[0][0]
    rows, cols, vals = (a.copy() for a in cu.upper({(int(r), int(c)): v for r, c, v in zip(g["rows"], g["cols"], g["vals"]) if r < c}))
    a = int(np.nonzero((rows == min(last, s)) & (cols == max(last, s)))[0][0])
    vals["suffixT" if last < s else "suffix"][a] = len(seqs[last]) + 1
    e.set_overlaps(M, rows, cols, vals)
    e.transitive_reduction(0.0, 0)
    g2 = e.export_string_graph()
    assert g2["n"] == 2 * len(rows)
    with pytest.raises(cu.BadPrefix) as xb:
        cx.generate_contigs_ex(M, g2["rows"], g2["cols"], g2["vals"], seqs, cx.CIRCULAR)
    assert xb.value.pair == (last, s)
    for flags in (cx.CIRCULAR, 3):
        with pytest.raises(elba_amd.ElbaError) as x:
            _gen(e, flags)
        assert x.value.status == 1 and "read %d (next read %d)" % (last, s) in str(x.value)
        with pytest.raises(elba_amd.ElbaError):
            e.export_contigs()
    for flags in (0, cx.SINGLETONS):
        _check(e, g2, _gen(e, flags), seqs, flags)
    e.close()


def test_one_context_over_changing_graphs_and_flags():
    rng = np.random.default_rng(40)
    e = elba_amd.Engine(17, 2, 8)
    for M, flags in ((2500, 3), (90, 0), (700, 1), (2500, 2), (33, 3)):
        seqs = cu.random_reads(rng, M, 1, 60)
        packed, off, lens = cu.pack(seqs)
        rows, cols, vals = cu.random_string_graph(rng, M, lens, n_paths=M // 6, p_extra=0.1)
        e.set_reads(packed, off, lens)
        e.set_overlaps(M, rows, cols, vals)
        e.transitive_reduction(0.0, 1000)
        g = e.export_string_graph()
        assert g["n"] == 2 * len(rows)
        _check(e, g, _gen(e, flags), seqs, flags)
        if M == 700:
            e.release_workspace()                                # the results survive, the next call allocates again
            assert e.export_contig_kinds(e.get_stat("contig_count")).max() == cx.CIRCLE
    e.close()


def test_replicated_reads_serve_the_graph():
    import torch
    rng = np.random.default_rng(17)
    seqs = cu.random_reads(rng, 80)
    packed, off, lens = cu.pack(seqs)
    rows, cols, vals = cu.random_string_graph(rng, 80, lens, n_paths=8, p_extra=0.1)
    e = elba_amd.Engine(17, 2, 8)
    e.set_reads(*cu.pack(seqs[:10]))                             # a shard of the reads
    dp = torch.from_numpy(packed.astype(np.uint8)).cuda(); do = torch.from_numpy(off.astype(np.int64)).cuda(); dl = torch.from_numpy(lens.astype(np.int32)).cuda()
    torch.cuda.synchronize()
    L = e.L
    L.elba_dist_set_all_reads.restype = C.c_int
    L.elba_dist_set_all_reads.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64]
    e._check(L.elba_dist_set_all_reads(e.h, dp.data_ptr(), len(packed) - 16, do.data_ptr(), dl.data_ptr(), 80))
    e.set_overlaps(80, rows, cols, vals)
    e.transitive_reduction(0.0, 1000)
    g = e.export_string_graph()
    assert g["n"] == 2 * len(rows)
    contigs, chains, kinds = _check(e, g, _gen(e, 3), seqs, 3)
    assert set(kinds) == {cx.PATH, cx.CIRCLE, cx.SINGLE}
    e.close()


def test_writers_agree_with_and_without_kinds(tmp_path):
    """Tiled reads of a circular genome, of a linear one, and unrelated reads through the whole pipeline: the host mirror
    (GenerateContigs + parallel_write_contigs with kinds) and write_contigs_fasta write the same file; without kinds the headers are today's."""
    rng = np.random.default_rng(50)
    circle, line = cx.random_genome(rng, 24000), cx.random_genome(rng, 12000)
    seqs = [(circle + circle)[i:i + 3000] for i in range(0, 24000, 1000)] + [line[i:i + 3000] for i in range(0, 9001, 1000)]
    seqs = [cu.revcomp(s) if rng.random() < 0.5 else s for s in seqs] + [cx.random_genome(rng, 1500) for _ in range(3)]
    seqs = [seqs[i] for i in rng.permutation(len(seqs))]
    fa = hu.write_fasta(tmp_path / "reads.fa", seqs)
    packed, off, lens = cu.pack(seqs)
    e = elba_amd.Engine(17, 2, 12)
    e.set_reads(packed, off, lens)
    e.count_kmers(); e.create_kmer_matrix(); e.create_seed_matrix()
    e.align_seeds()
    e.transitive_reduction(0.65, 1000)
    g = e.export_string_graph()
    contigs, chains, kinds = _check(e, g, _gen(e, 3), seqs, 3)
    assert kinds.count(cx.CIRCLE) == 1 and kinds.count(cx.SINGLE) >= 3 and cx.PATH in kinds
    assert cx.is_rotation(contigs[kinds.index(cx.CIRCLE)], circle)
    got = e.export_contigs()
    for with_kinds in (1, 0):
        out, ref = tmp_path / ("cpp%d.contigs.fa" % with_kinds), tmp_path / ("py%d.contigs.fa" % with_kinds)
        hu.run_json(hu.binary("test_host_contigs_ex"), [fa, 17, 2, 12, out, 3, with_kinds])
        formats.write_contigs_fasta(str(ref), got["seqs"], kinds=got["kinds"] if with_kinds else None)
        assert out.read_bytes() == ref.read_bytes()
        heads = [ln for ln in ref.read_text().split("\n") if ln.startswith(">")]
        assert heads == [">contig%d%s" % (i, " circular" if with_kinds and k == cx.CIRCLE else "") for i, k in enumerate(kinds)]
    today = tmp_path / "today.contigs.fa"
    formats.write_contigs_fasta(str(today), got["seqs"])
    assert today.read_bytes() == (tmp_path / "py0.contigs.fa").read_bytes()
    e.close()
