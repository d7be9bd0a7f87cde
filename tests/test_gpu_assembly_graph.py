"""-m gpu: the links of the assembly graph on the GPU (elba_export_assembly_links, graph_links.hip) against the two restatements of
gfa_util.py, fed with the GPU's own exported S, contigs and read map: record for record, count for count.  The graphs are triangle-free, so
the transitive reduction at fuzz 0 keeps every edge; each test asserts that from the export."""
import ctypes as C

import numpy as np
import pytest

import contig_util as cu
import elba_amd
import gfa_util as gu
from elba_amd import capi, formats
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

NONE = (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, po.OVERLAP_DTYPE))


def _engine(packed, off, lens, rows, cols, vals, e=None):
    e = elba_amd.Engine(17, 2, 8) if e is None else e
    e.set_reads(packed, off, lens)
    e.set_overlaps(len(lens), rows, cols, vals)
    e.transitive_reduction(0.0, 0)
    g = e.export_string_graph()
    assert g["n"] == 2 * len(rows)                               # S keeps every edge
    return e, g


def _gen(e, flags):
    return e.generate_contigs(circular=bool(flags & 1), singletons=bool(flags & 2))


def _check(e, g, lens):
    """The device's records and counts are those of both restatements on the device's own S and contigs."""
    M = len(lens)
    got = e.export_contigs()
    inp = gu.inputs_of_export(g, got, e.export_read_contigs(M), lens)
    recs, st = e.assembly_links()
    assert recs.dtype == capi.LINK_DTYPE and st["ms_total"] > 0
    for want, wst in (gu.links_walk(inp), gu.links_tables(inp)):
        assert {k: st[k] for k in gu.STATS} == wst, (st, wst)
        assert gu.same_records(recs, want), (recs[:8], want[:8])
    for k in gu.STATS:
        assert e.get_stat("graph_" + k) == st[k]
    return recs, st, got


def _edges(rng, x, y, lens):
    """Entries with any direction pair and valid prefixes for the pairs {x[a], y[a]}: (rows, cols, vals) ascending in (row, col)."""
    x = np.asarray(x, dtype=np.int64); y = np.asarray(y, dtype=np.int64)
    r, c = np.minimum(x, y), np.maximum(x, y)
    order = np.lexsort((c, r))
    r, c = r[order], c[order]
    assert len(set(zip(r.tolist(), c.tolist()))) == len(r) and (r < c).all()
    v = np.zeros(len(r), dtype=po.OVERLAP_DTYPE)
    v["passed"] = 1
    v["direction"] = rng.integers(0, 4, len(r)); v["directionT"] = rng.integers(0, 4, len(r))
    v["suffixT"] = rng.integers(0, np.asarray(lens)[r].astype(np.int64) + 1); v["suffix"] = rng.integers(0, np.asarray(lens)[c].astype(np.int64) + 1)
    return r, c, v


def test_no_reads_no_entries_no_branch_and_only_closures():
    e = elba_amd.Engine(17, 2, 8)                                # M = 0
    e.set_reads(np.zeros(16, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint32))
    e.set_overlaps(0, *NONE)
    e.transitive_reduction(0.0, 0)
    _gen(e, 3)
    recs, st = e.assembly_links()
    assert len(recs) == 0 and {k: st[k] for k in gu.STATS} == dict.fromkeys(gu.STATS, 0)
    e.close()
    rng = np.random.default_rng(1)
    packed, off, lens = cu.random_packed(rng, 70, 4, 24)
    e, g = _engine(packed, off, lens, *NONE)                     # S empty: 70 one-read segments, no record
    _gen(e, 3)
    recs, st, _ = _check(e, g, lens)
    assert len(recs) == 0 and st["segments"] == 70 and st["candidates"] == 0
    ids = rng.permutation(70)
    x = np.concatenate([ids[0:19], ids[20:39]]); y = np.concatenate([ids[1:20], ids[21:40]])
    e, g = _engine(packed, off, lens, *_edges(rng, x, y, lens), e=e)         # two paths: no branch at all
    _gen(e, 3)
    recs, st, _ = _check(e, g, lens)
    assert len(recs) == 0 and st["candidates"] == 0 and st["segments"] == 32
    x = np.concatenate([ids[0:20], ids[20:30], ids[30:70]]); y = np.concatenate([np.roll(ids[0:20], -1), np.roll(ids[20:30], -1), np.roll(ids[30:70], -1)])
    e, g = _engine(packed, off, lens, *_edges(rng, x, y, lens), e=e)         # three rings: only closures
    _gen(e, 1)
    recs, st, got = _check(e, g, lens)
    assert st["closures"] == 3 == len(recs) and st["candidates"] == 0 and (recs["flags"] == 1).all() and (recs["overlap"] == 0).all()
    assert recs["from_read"].tolist() == sorted([int(ids[0:20].min()), int(ids[20:30].min()), int(ids[30:70].min())])
    e.close()


@pytest.mark.parametrize("deg", [3, 63, 64, 65, 257])
def test_branch_columns_around_the_wavefront_width(deg):
    """A hub of `deg` neighbours in the middle of the ids, so that kept ends lie on both sides of the diagonal: half of the neighbours are
    lone reads, half are ends of two-read paths; a second hub of 70 shares some of them.  Up to 64 entries a lane walks the column, beyond
    that the wavefront does."""
    rng = np.random.default_rng(deg)
    M = 3 * deg + 200
    packed, off, lens = cu.random_packed(rng, M, 4, 24)
    ids = rng.permutation(M)
    hub, hub2 = M // 2, M // 2 + 1
    ids = np.concatenate([[hub, hub2], ids[(ids != hub) & (ids != hub2)]])
    lo, hi = 2 + int(np.argmax(ids[2:] < hub)), 3 + int(np.argmax(ids[3:] > hub2))
    ids[[2, lo]] = ids[[lo, 2]]; ids[[3, hi]] = ids[[hi, 3]]    # a neighbour on either side of the hub whatever its degree
    nb = ids[2:2 + deg]
    tails = ids[2 + deg:2 + deg + deg // 2]                      # the first deg // 2 neighbours are ends of two-read paths
    nb2 = np.concatenate([nb[:min(deg, 5)], ids[2 + 2 * deg:2 + 2 * deg + 65]])
    x = np.concatenate([np.full(deg, hub), nb[:deg // 2], np.full(len(nb2), hub2)])
    y = np.concatenate([nb, tails, nb2])
    e, g = _engine(packed, off, lens, *_edges(rng, x, y, lens))
    degs = np.bincount(g["cols"], minlength=M)
    assert degs[hub] == deg and degs[hub2] == len(nb2) and (nb < hub).any() and (nb > hub).any()
    for flags in (3, 2):
        _gen(e, flags)
        recs, st, _ = _check(e, g, lens)
        # (the path ends that the second hub holds too have degree 3: their path edge is a candidate as well)
        assert st["candidates"] == deg + len(nb2) + min(5, deg // 2) and st["unplaced"] == 0 and st["links"] > deg // 2
        assert ((recs["from_read"] == hub) | (recs["to_read"] == hub)).sum() > deg // 2
    _gen(e, 0)                                                   # the hubs and the lone reads are in no contig
    recs, st, _ = _check(e, g, lens)
    assert st["unplaced"] == st["candidates"] and len(recs) == 0
    e.close()


@pytest.mark.parametrize("M", [255, 256, 257])
def test_random_graphs_around_a_block_edge_under_every_flag_combination(M):
    rng = np.random.default_rng(M)
    seqs = cu.random_reads(rng, M, 1, 60)
    packed, off, lens = cu.pack(seqs)
    rows, cols, vals = cu.random_string_graph(rng, M, lens, n_paths=M // 6, p_extra=0.25)
    e, g = _engine(packed, off, lens, rows, cols, vals)
    seen = dict.fromkeys(gu.STATS, 0)
    for flags in range(4):
        _gen(e, flags)
        recs, st, _ = _check(e, g, lens)
        assert (st["unplaced"] == 0) == bool(flags & 2)
        for k in gu.STATS:
            seen[k] += st[k]
    assert all(seen[k] > 0 for k in ("candidates", "links", "twisted", "unplaced", "asymmetric"))
    e.close()


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_totals_on_and_beside_one_span_of_the_scan(delta):
    """Stars of lone reads emit every edge, so the total is the number of edges: the scan's span (prims.hip: SCAN_THREADS x SCAN_ITEMS, read
    from elba_get_stat) and one either side; more reads than one span as well."""
    e = elba_amd.Engine(17, 2, 8)
    span = e.get_stat("text_scan_span")
    assert span == 2048
    total = span + delta
    rng = np.random.default_rng(total)
    nstars = total // 3 - 1
    sizes = [3] * nstars + [total - 3 * nstars]
    M = sum(sizes) + len(sizes) + 5
    assert M > span and sizes[-1] >= 3
    ids = rng.permutation(M)
    x, y, at = [], [], 0
    for s in sizes:
        x.append(np.full(s, ids[at])); y.append(ids[at + 1:at + 1 + s]); at += s + 1
    packed, off, lens = cu.random_packed(rng, M, 4, 24)
    e, g = _engine(packed, off, lens, *_edges(rng, np.concatenate(x), np.concatenate(y), lens), e=e)
    _gen(e, 3)
    recs, st, _ = _check(e, g, lens)
    assert len(recs) == total == st["links"] == st["candidates"] and st["twisted"] == 0
    e.close()


@pytest.mark.parametrize("seed,glen,n,skips", [(21, 4000, 12, (3,)), (22, 9000, 40, (5, 7, 9, 20, 37)), (23, 60000, 300, tuple(range(2, 290, 6)))])
def test_ground_truth_graphs_satisfy_the_sequence_property_on_the_device(seed, glen, n, skips, tmp_path):
    """The generator's triangle-free form (the true edge (i + 1, i + 2) left out at every skip: with it the skip edge is transitive by
    construction and the reduction, which is the only way an S gets onto a context, removes it).  On the device's own contigs and links:
    every link's oriented from-segment ends with the bases its oriented to-segment begins with, nothing is twisted, clamped,
    asymmetric or unplaced, and the GFA is one connected graph."""
    rng = np.random.default_rng(seed)
    genome, seqs, edges, ids, rc = gu.truth_graph(rng, glen, n, skips, drop_middle=True)
    packed, off, lens = cu.pack(seqs)
    e, g = _engine(packed, off, lens, *cu.upper(edges))
    _gen(e, 3)
    recs, st, got = _check(e, g, lens)
    assert st["twisted"] == st["clamped"] == st["asymmetric"] == st["unplaced"] == st["closures"] == 0 and st["links"] >= len(skips)
    assert all(c in genome or cu.revcomp(c) in genome for c in got["seqs"])
    assert gu.sequence_property_failures(got["seqs"], recs) == []
    path = tmp_path / "truth.gfa"
    formats.write_gfa(str(path), got["seqs"], got["kinds"], recs, chains=got["chain_off"])
    version, segs, links = gu.parse_gfa(str(path))
    assert gu.gfa_components(segs, links) == 1 and len(segs) == got["n"] and len(links) == len(recs)
    e.close()


@pytest.mark.parametrize("name", sorted(gu.hand_cases()))
def test_hand_cases_on_the_device(name):
    case = gu.hand_cases()[name]
    (rows, cols, vals), seqs = gu.case_graph(case)
    packed, off, lens = cu.pack(seqs)
    e, g = _engine(packed, off, lens, *cu.upper(case["edges"]))
    _gen(e, case["flags"])
    recs, st, _ = _check(e, g, lens)
    case["claims"](recs, st, e.export_read_contigs(case["M"]).tolist())
    e.close()


def test_after_simplify_graph_and_after_clip_tips():
    rng = np.random.default_rng(77)
    M = 1200
    seqs = cu.random_reads(rng, M, 1, 60)
    packed, off, lens = cu.pack(seqs)
    rows, cols, vals = cu.random_string_graph(rng, M, lens, n_paths=M // 8, p_extra=0.2)
    e, g = _engine(packed, off, lens, rows, cols, vals)
    _gen(e, 3)
    before, st0, _ = _check(e, g, lens)
    e.simplify_graph(3, 3, bridges=(1, 3), stars=True)
    g2 = e.export_string_graph()
    rf = e.export_read_flags(M)
    assert 0 < g2["n"] < g["n"] and (rf != 0).any()
    with pytest.raises(elba_amd.ElbaError) as x:                 # the cleaning calls drop the contigs
        e.assembly_links()
    assert x.value.status == 5
    _gen(e, 3)
    recs, st, _ = _check(e, g2, lens)
    assert st["unplaced"] == 0 and 0 < st["candidates"] <= st0["candidates"]
    rc = e.export_read_contigs(M)
    assert (rc[rf != 0] == -1).all() and not np.isin(np.nonzero(rf != 0)[0], np.concatenate([recs["from_read"], recs["to_read"]])).any()
    e.close()


def test_one_context_over_graphs_of_changing_size_and_a_released_workspace():
    rng = np.random.default_rng(40)
    e = elba_amd.Engine(17, 2, 8)
    for M, flags in ((2500, 3), (90, 2), (700, 1), (2500, 2), (33, 3)):
        seqs = cu.random_reads(rng, M, 1, 60)
        packed, off, lens = cu.pack(seqs)
        rows, cols, vals = cu.random_string_graph(rng, M, lens, n_paths=M // 6, p_extra=0.2)
        e, g = _engine(packed, off, lens, rows, cols, vals, e=e)
        assert e.get_stat("graph_links") == 0 and e.get_stat("graph_segments") == 0      # nothing valid yet
        _gen(e, flags)
        assert e.get_stat("graph_segments") == 0                 # no call on these contigs yet
        recs, st, _ = _check(e, g, lens)
        if M == 700:
            e.release_workspace()
            again, st2 = e.assembly_links()
            assert gu.same_records(recs, again) and {k: st2[k] for k in gu.STATS} == {k: st[k] for k in gu.STATS}
    with pytest.raises(elba_amd.ElbaError):
        e.get_stat("graph_nothing")
    e.close()


def test_replicated_reads_serve_the_lengths():
    import torch
    rng = np.random.default_rng(17)
    seqs = cu.random_reads(rng, 80)
    packed, off, lens = cu.pack(seqs)
    rows, cols, vals = cu.random_string_graph(rng, 80, lens, n_paths=8, p_extra=0.3)
    e = elba_amd.Engine(17, 2, 8)
    e.set_reads(*cu.pack(seqs[:10]))                             # a shard of the reads
    dp = torch.from_numpy(packed.astype(np.uint8)).cuda(); do = torch.from_numpy(off.astype(np.int64)).cuda(); dl = torch.from_numpy(lens.astype(np.int32)).cuda()
    torch.cuda.synchronize()
    L = e.L
    L.elba_dist_set_all_reads.restype = C.c_int
    L.elba_dist_set_all_reads.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64]
    e._check(L.elba_dist_set_all_reads(e.h, dp.data_ptr(), len(packed) - 16, do.data_ptr(), dl.data_ptr(), 80))
    e.set_overlaps(80, rows, cols, vals)
    e.transitive_reduction(0.0, 0)
    g = e.export_string_graph()
    assert g["n"] == 2 * len(rows)
    _gen(e, 3)
    recs, st, _ = _check(e, g, lens)
    assert st["links"] > 0
    e.close()


def test_state_errors_and_an_untouched_context():
    rng = np.random.default_rng(5)
    M = 400
    seqs = cu.random_reads(rng, M, 1, 60)
    packed, off, lens = cu.pack(seqs)
    rows, cols, vals = cu.random_string_graph(rng, M, lens, n_paths=M // 6, p_extra=0.2)
    e = elba_amd.Engine(17, 2, 8)
    e.set_reads(packed, off, lens)

    def refused():
        with pytest.raises(elba_amd.ElbaError) as x:
            e.assembly_links()
        assert x.value.status == 5
        assert e.get_stat("graph_links") == 0
    refused()                                                    # no S
    e.set_overlaps(M, rows, cols, vals)
    refused()
    e.transitive_reduction(0.0, 0)
    refused()                                                    # S, no contigs
    g = e.export_string_graph()
    _gen(e, 3)
    # the call changes nothing: S, the flags, the contigs, the read map and the validity of all of them
    before = (e.export_string_graph(), e.export_contigs(), e.export_read_contigs(M), e.export_read_flags(M))
    recs, st, _ = _check(e, g, lens)
    again, st2 = e.assembly_links()                              # and gives the same answer twice
    assert gu.same_records(recs, again)
    after = (e.export_string_graph(), e.export_contigs(), e.export_read_contigs(M), e.export_read_flags(M))
    for k in ("rows", "cols"):
        assert (before[0][k] == after[0][k]).all()
    assert before[0]["vals"].tobytes() == after[0]["vals"].tobytes() and before[1]["seqs"] == after[1]["seqs"]
    for k in ("seq_off", "chain_off", "chain_read", "chain_prefix", "chain_strand", "kinds"):
        assert np.array_equal(before[1][k], after[1][k]), k
    assert (before[2] == after[2]).all() and (before[3] == after[3]).all()
    assert e.L.elba_export_assembly_links(e.h, None, None) == 1  # a null output
    out = capi.Links()
    assert e.L.elba_export_assembly_links(e.h, C.byref(out), None) == 0 and out.n == len(recs)      # stats may be null
    e.L.elba_free_links(C.byref(out))
    assert out.n == 0 and not out.links
    e.L.elba_free_links(C.byref(out)); e.L.elba_free_links(None)
    e.clip_tips(2, 1)                                            # drops the contigs
    refused()
    _gen(e, 3)
    _check(e, e.export_string_graph(), lens)
    e.set_reads(*cu.pack(seqs[:20]))                             # the reads the contig stage needed are gone (and the contigs with them)
    refused()
    e.close()
