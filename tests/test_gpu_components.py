"""-m gpu: elba_graph_components and elba_partition_components (elba_amd/csrc/components.hip) against the restatement in comp_util.py.
The expected labels come from the literal union-find over what the device itself exports — export_string_graph for S, the loaded or
exported pairs for the overlaps — so the reduction is not under test.  Graphs are loaded with elba_set_overlaps with suffixes the
reduction does not remove at cutoff 0 and fuzz 0 (every suffix in [5, 9]: a two-edge walk is at least 10), which _load asserts."""
import ctypes as C

import numpy as np
import pytest

import comp_util as ku
import contig_util as cu
import elba_amd
import gfa_util as gu
import placement_util as pu
import string_graph_util as sg
from elba_amd import capi, formats
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

CASES = ku.hand_cases()
INVALID, STATE, UNSUPPORTED = 1, 5, 6
PASS_CAP = 512
STATS = ("nreads", "edges", "components", "used_components", "isolated", "largest_reads", "largest_bases")


@pytest.fixture(scope="module")
def eng():
    e = elba_amd.Engine(17, 2, 8)
    yield e
    e.close()


def _load(e, M, u, v, rng, passed=None, reduce=True):
    """The edge list as pairs on the engine; with reduce also its S, which keeps every passed pair.  Returns (rows, cols, vals)."""
    rows, cols = ku.sorted_pairs(u, v)
    vals = ku.overlap_records(rng, len(rows), po.OVERLAP_DTYPE, passed)
    e.set_overlaps(M, rows, cols, vals)
    if reduce:
        s = e.transitive_reduction(0.0, 0)
        assert s["nnz"] == 2 * int((vals["passed"] != 0).sum())
    return rows, cols, vals


def _same(cc, st, want, M):
    assert ku.same_tables(cc, want) is None, ku.same_tables(cc, want)
    ws = ku.stats(want)
    assert {k: st[k] for k in STATS} == ws, (st, ws)
    assert st["nreads"] == M and st["ms_total"] >= st["ms_label"] >= 0 and 0 < st["passes"] <= PASS_CAP
    return cc, st


def _string(e, M, lens=None, base=0):
    """graph_components of S equals the restatement on the S the device exports."""
    g = e.export_string_graph()
    u, v = ku.edges_of_string_graph(g)
    want = ku.tables(M, u - base, v - base, lens=lens, base=base)
    cc, st = e.graph_components("string", bases=lens is not None)
    return _same(cc, st, want, M)


def _overlaps(e, M, rows, cols, vals, lens=None, base=0):
    u, v = ku.edges_of_overlaps(rows, cols, vals)
    want = ku.tables(M, u - base, v - base, lens=lens, base=base)
    cc, st = e.graph_components("overlaps", bases=lens is not None)
    return _same(cc, st, want, M)


def _zero_reads(M, length):
    """M reads of `length` bases each, every byte zero: (packed, byte_off, lens)."""
    nb = (length + 3) // 4
    return np.zeros(M * nb + 16, dtype=np.uint8), (np.arange(M, dtype=np.uint64) * np.uint64(nb)), np.full(M, length, dtype=np.uint32)


# ---- hand cases and state --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_the_rule_one_clause_per_case(eng, name):
    case = CASES[name]
    M, u, v = ku.case_edges(case)
    rows, cols, vals = _load(eng, M, u, v, np.random.default_rng(3))
    cc, st = _string(eng, M)
    ku.check_case(case, cc)
    cc2, _ = _overlaps(eng, M, rows, cols, vals)
    ku.check_case(case, cc2)
    assert eng.get_stat("cc_components") == len(case["edges"]) == st["components"]
    if name == "no_edge":
        assert st["components"] == M and st["isolated"] == M and st["edges"] == 0
    if name == "ring4":
        assert (cc["reads"][0], cc["edges"][0], cc["branches"][0], cc["ends"][0]) == (4, 4, 0, 0)


@pytest.mark.parametrize("M", [6, 300])
def test_a_pair_of_which_s_holds_one_image_is_one_edge(eng, M):
    """The reduction drops an image without a direction alone: on a path whose pairs lack direction, directionT or neither in turn, S holds
    one entry of some pairs — above or below the diagonal — and both of others.  Every such pair is still one edge with two ends."""
    rng = np.random.default_rng(M)
    _, u, v = ku.path(M, "random", rng)
    rows, cols = ku.sorted_pairs(u, v)
    vals = ku.overlap_records(rng, len(rows), po.OVERLAP_DTYPE)
    which = np.arange(len(rows)) % 3
    vals["direction"][which == 1] = -1
    vals["directionT"][which == 2] = -1
    eng.set_overlaps(M, rows, cols, vals)
    eng.transitive_reduction(0.0, 0)
    g = eng.export_string_graph()
    pairs = set(zip(np.minimum(g["rows"], g["cols"]).tolist(), np.maximum(g["rows"], g["cols"]).tolist()))
    below, above = int((g["rows"] > g["cols"]).sum()), int((g["rows"] < g["cols"]).sum())
    assert len(pairs) == M - 1 and g["n"] < 2 * (M - 1) and below < M - 1 and above < M - 1      # one image of some pairs, on either side
    cc, st = _string(eng, M)
    assert cc["reads"].tolist() == [M] and cc["edges"].tolist() == [M - 1] and cc["ends"].tolist() == [2] and cc["branches"].tolist() == [0]
    part, pw = eng.partition_components(2, nreads=M)
    assert pw.tolist() == [M, 0] and (part == 0).all()


def test_every_error_status_and_the_state_conditions():
    e = elba_amd.Engine(17, 2, 8)
    rng = np.random.default_rng(1)
    with pytest.raises(elba_amd.ElbaError) as err:               # nothing loaded: no S, no pairs
        e.graph_components("string")
    assert err.value.status == STATE
    with pytest.raises(elba_amd.ElbaError) as err:
        e.graph_components("overlaps")
    assert err.value.status == STATE
    M, u, v = ku.path(9)
    rows, cols, vals = _load(e, M, u, v, rng, reduce=False)
    _overlaps(e, M, rows, cols, vals)                            # the pairs are enough for their graph
    with pytest.raises(elba_amd.ElbaError) as err:
        e.graph_components("string")
    assert err.value.status == STATE and "string graph" in str(err.value)
    with pytest.raises(elba_amd.ElbaError) as err:
        e.partition_components(2, nreads=M)
    assert err.value.status == STATE
    e.transitive_reduction(0.0, 0)
    _string(e, M)
    for kw in (dict(graph=2), dict(graph=-1), dict(flags=2), dict(flags=-1), dict(reserved=(1, 0)), dict(reserved=(0, 1))):
        with pytest.raises(elba_amd.ElbaError) as err:
            e.graph_components(**kw)
        assert err.value.status == INVALID, kw
    o, s = capi.Components(), capi.CcStats()
    o.nreads, o.reads = 7, 8                                     # (stale values: the call zeroes them)
    assert e.L.elba_graph_components(e.h, None, C.byref(o), C.byref(s)) == INVALID
    assert o.nreads == 0 and o.n == 0 and not (o.comp_of_read or o.first_read or o.reads or o.bases or o.edges or o.branches or o.ends)
    assert e.L.elba_graph_components(e.h, C.byref(capi.CcCfg(0, 0)), None, None) == INVALID
    for graph in ("string", "overlaps"):                         # bases without the reads
        with pytest.raises(elba_amd.ElbaError) as err:
            e.graph_components(graph, bases=True)
        assert err.value.status == STATE and "lengths" in str(err.value)
        with pytest.raises(elba_amd.ElbaError) as err:
            e.partition_components(2, graph=graph, weight="bases", nreads=M)
        assert err.value.status == STATE
    packed, off, lens = cu.random_packed(rng, M + 1)             # ... and with reads that are not the graph's
    e.set_reads(packed, off, lens)
    rows, cols, vals = _load(e, M, u, v, rng)
    with pytest.raises(elba_amd.ElbaError) as err:
        e.graph_components("string", bases=True)
    assert err.value.status == STATE
    for kw in (dict(nparts=0), dict(nparts=-3), dict(nparts=2, weight=2), dict(nparts=2, min_reads=-1), dict(nparts=2, reserved=(0, 0, 0, 1)), dict(nparts=2, graph=5),
               dict(nparts=2, nreads=M + 1), dict(nparts=2, nreads=M - 1)):
        kw.setdefault("nreads", M)
        with pytest.raises(elba_amd.ElbaError) as err:
            e.partition_components(**kw)
        assert err.value.status == INVALID, kw
    part = np.zeros(M, dtype=np.int32)
    assert e.L.elba_partition_components(e.h, None, part.ctypes.data, M, part.ctypes.data) == INVALID
    assert e.L.elba_partition_components(e.h, C.byref(capi.PartCfg(0, 2, 0, 2)), part.ctypes.data, M, None) == INVALID
    _string(e, M)                                                # none of that left anything behind
    e.close()


def test_the_counters_follow_the_graph_they_belong_to():
    e = elba_amd.Engine(17, 2, 8)
    rng = np.random.default_rng(2)
    M, u, v = ku.isolated_pairs(5)
    _load(e, M, u, v, rng)
    assert e.get_stat("cc_components") == 0 == e.get_stat("cc_passes")           # before the first call
    cc, st = _string(e, M)
    assert (e.get_stat("cc_components"), e.get_stat("cc_used_components"), e.get_stat("cc_largest_reads"), e.get_stat("cc_passes")) == (10, 5, 2, st["passes"])
    part, pw = e.partition_components(2, nreads=M)               # the partition labels too
    assert e.get_stat("cc_components") == 10 and pw.tolist() == [6, 4]
    e.set_overlaps(M, *ku.sorted_pairs(u, v), ku.overlap_records(rng, 5, po.OVERLAP_DTYPE))       # new pairs drop S
    assert e.get_stat("cc_components") == 0 == e.get_stat("cc_largest_reads")
    e.graph_components("overlaps")
    assert e.get_stat("cc_components") == 10
    with pytest.raises(elba_amd.ElbaError) as err:
        e.get_stat("cc_nothing")
    assert err.value.status == INVALID
    e.close()


def test_an_export_changes_nothing_and_survives_release_workspace():
    t = pu.truth_set(np.random.default_rng(5), 1500, 20, False, 30, 12)
    packed, off, lens = cu.pack(t["seqs"])
    M = len(lens)
    e = elba_amd.Engine(17, 2, 8)
    e.set_reads(packed, off, lens)
    e.set_overlaps(M, *t["pairs"])
    e.read_pileup(mode=0, margin=0, min_depth=1, min_run=1, trim_len=0)
    e.transitive_reduction(0.0, 0)
    e.generate_contigs(circular=True, singletons=True)

    def snapshot():
        c = e.export_contigs()
        links, ls = e.assembly_links()
        pl, ps = e.place_reads()
        p = e.export_pileup()
        g = e.export_string_graph()
        return [c["seqs"], c["chain_read"].tobytes(), c["kinds"].tobytes(), links.tobytes(), pl["reads"].tobytes(), pl["seg_depth"].tobytes(), pl["credited_bases"].tobytes(),
                p["seg_off"].tobytes(), p["seg_depth"].tobytes(), p["trim_beg"].tobytes(), g["rows"].tobytes(), g["vals"].tobytes(), e.export_read_flags(M).tobytes(),
                e.get_stat("contig_count"), e.get_stat("graph_links"), e.get_stat("place_chain")]
    before = snapshot()
    cc, st = _string(e, M, lens=lens)
    co, sto = _overlaps(e, M, *t["pairs"], lens=lens)
    part, pw = e.partition_components(3, weight="bases", nreads=M)
    assert snapshot() == before
    # contained reads (flag 2) are lone in S and inside their container's component among the overlaps: one genome, one component
    contained = np.flatnonzero(t["read_flags"] & 2)
    assert len(contained) == 30 and (cc["reads"][cc["comp_of_read"][contained]] == 1).all()
    assert sto["components"] == 1 and co["reads"].tolist() == [M] and co["bases"].tolist() == [int(lens.astype(np.int64).sum())]
    e.release_workspace()
    cc2, st2 = _string(e, M, lens=lens)
    assert ku.same_tables(cc2, cc) is None and {k: st2[k] for k in STATS} == {k: st[k] for k in STATS}
    part2, pw2 = e.partition_components(3, weight="bases", nreads=M)
    assert (part2 == part).all() and (pw2 == pw).all()
    assert snapshot() == before
    e.close()


# ---- passes ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ku.NUMBERINGS)
def test_a_path_of_131073_reads_takes_logarithmic_passes(eng, kind):
    M, u, v = ku.path((1 << 17) + 1, kind, np.random.default_rng(17))
    rows, cols, vals = _load(eng, M, u, v, np.random.default_rng(4))
    for call in (lambda: _string(eng, M), lambda: _overlaps(eng, M, rows, cols, vals)):
        cc, st = call()
        assert st["components"] == 1 and cc["first_read"].tolist() == [0] and cc["edges"].tolist() == [M - 1] and cc["ends"].tolist() == [2]
        assert cc["branches"].tolist() == [0] and st["passes"] <= PASS_CAP and eng.get_stat("cc_passes") == st["passes"]
        assert (cc["comp_of_read"] == 0).all()


@pytest.mark.parametrize("shape", ["binary_tree", "caterpillar"])
def test_a_deep_tree_and_an_alternating_caterpillar_under_the_same_cap(eng, shape):
    M, u, v = ku.binary_tree(16) if shape == "binary_tree" else ku.caterpillar(1 << 16, "alternating")
    rows, cols, vals = _load(eng, M, u, v, np.random.default_rng(5))
    for cc, st in (_string(eng, M), _overlaps(eng, M, rows, cols, vals)):
        assert st["components"] == 1 and st["passes"] <= PASS_CAP and cc["edges"].tolist() == [M - 1]
        assert cc["ends"].tolist() == [1 << 16] and cc["branches"].tolist() == [(1 << 16) - 2]


# ---- one hot word ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hub_first", [True, False])
def test_a_star_of_70000_leaves(eng, hub_first):
    M, u, v = ku.star(70000, hub_first)
    rows, cols, vals = _load(eng, M, u, v, np.random.default_rng(6))
    for cc, st in (_string(eng, M), _overlaps(eng, M, rows, cols, vals)):
        assert cc["reads"].tolist() == [M] and cc["branches"].tolist() == [1] and cc["ends"].tolist() == [70000] and cc["edges"].tolist() == [70000]


def test_a_component_of_100000_reads_beside_30000_lone_reads(eng):
    rng = np.random.default_rng(7)
    M = 130000
    member = np.sort(rng.permutation(M)[:100000])                # the lone reads lie anywhere among them: mixed wavefronts
    _, u, v = ku.path(100000, "random", rng)
    packed, off, lens = cu.random_packed(rng, M, 20, 60)
    eng.set_reads(packed, off, lens)                             # (new reads drop the pairs: the reads come first)
    rows, cols, vals = _load(eng, M, member[u], member[v], rng)
    for cc, st in (_string(eng, M, lens=lens), _overlaps(eng, M, rows, cols, vals, lens=lens)):
        assert st["components"] == 30001 and st["isolated"] == 30000 and st["used_components"] == 1 and st["largest_reads"] == 100000
        assert st["largest_bases"] == int(lens[member].astype(np.int64).sum()) and int(cc["bases"].sum()) == int(lens.astype(np.int64).sum())


def test_bases_past_two_to_the_32(eng):
    M, L = 66000, 65536
    eng.set_reads(*_zero_reads(M, L))
    _, u, v = ku.path(M, "alternating")
    rows, cols, vals = _load(eng, M, u, v, np.random.default_rng(8), reduce=False)
    cc, st = eng.graph_components("overlaps", bases=True)
    assert M * L > 1 << 32 and cc["bases"].tolist() == [M * L] and st["largest_bases"] == M * L and cc["reads"].tolist() == [M]
    part, pw = eng.partition_components(2, graph="overlaps", weight="bases", nreads=M)
    assert pw.tolist() == [M * L, 0] and (part == 0).all()
    cc, st = eng.graph_components("overlaps")                    # without the flag: all zero
    assert cc["bases"].tolist() == [0] and st["largest_bases"] == 0


# ---- many components -------------------------------------------------------------------------------------------------------------------
def test_65537_pairs_interleaved_with_lone_reads(eng):
    M, u, v = ku.isolated_pairs(65537)
    rows, cols, vals = _load(eng, M, u, v, np.random.default_rng(9))
    for cc, st in (_string(eng, M), _overlaps(eng, M, rows, cols, vals)):
        assert st["components"] == 2 * 65537 and st["used_components"] == 65537 == st["isolated"] and st["largest_reads"] == 2
        assert (np.diff(cc["first_read"]) > 0).all() and cc["first_read"][-1] == M - 2 and int(cc["comp_of_read"].max()) == 2 * 65537 - 1 > 1 << 16
        assert (cc["comp_of_read"][0::3] == cc["comp_of_read"][2::3]).all() and (cc["comp_of_read"][1::3] == cc["comp_of_read"][0::3] + 1).all()


# ---- edges of lanes and tiles ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [255, 256, 257])
@pytest.mark.parametrize("nedges", [1, 256, 257])
def test_reads_and_edges_around_one_workgroup(eng, M, nedges):
    rng = np.random.default_rng(1000 * M + nedges)
    _, u, v = ku.random_graph(rng, M, nedges)
    if nedges == 1:
        u, v = np.array([M - 2]), np.array([M - 1])              # the last two reads
    assert len(u) == nedges
    rows, cols, vals = _load(eng, M, u, v, rng)
    _string(eng, M)
    _overlaps(eng, M, rows, cols, vals)


@pytest.mark.parametrize("nnz", [65535, 65536, 65537])
def test_an_edge_list_around_two_to_the_16(eng, nnz):
    rng = np.random.default_rng(nnz)
    M, u, v = ku.random_graph(rng, 70001, nnz)
    assert len(u) == nnz
    passed = (rng.random(nnz) < 0.9).astype(np.uint8)
    rows, cols, vals = _load(eng, M, u, v, rng, passed=passed)
    _string(eng, M)
    _overlaps(eng, M, rows, cols, vals)


def test_the_last_edge_of_the_list_joins_two_components_of_30000_reads(eng):
    M, u, v = ku.two_giants(30000)
    rng = np.random.default_rng(10)
    rows, cols, vals = _load(eng, M, u, v, rng)
    assert (int(rows[-1]), int(cols[-1])) == (M - 2, M - 1)
    g = eng.export_string_graph()
    half = np.flatnonzero(g["rows"] > g["cols"])
    assert (int(g["cols"][half[-1]]), int(g["rows"][half[-1]])) == (M - 2, M - 1)
    for cc, st in (_string(eng, M), _overlaps(eng, M, rows, cols, vals)):
        assert cc["reads"].tolist() == [M] and cc["ends"].tolist() == [2]
    passed = np.ones(len(rows), dtype=np.uint8)
    passed[-1] = 0                                               # the same list with that pair failed: the only bridge does not join them
    rows, cols, vals = _load(eng, M, u, v, rng, passed=passed)
    for cc, st in (_string(eng, M), _overlaps(eng, M, rows, cols, vals)):
        assert cc["reads"].tolist() == [30000, 30000] and cc["first_read"].tolist() == [0, 29999] and st["edges"] == M - 2


# ---- the overlaps graph ----------------------------------------------------------------------------------------------------------------
def test_own_alignments_a_loaded_list_and_the_id_base():
    packed, off, lens, info = elba_amd.synth_reads(77, 30000, 14, 2500, 400, error_rate=0.01)
    M = len(lens)
    e = elba_amd.Engine(17, 2, 30)
    seen = {}
    for base in (0, 1000, 1 << 32):
        e.set_reads(packed, off, lens, first_global_id=base)
        e.count_kmers(); e.create_kmer_matrix(); e.create_seed_matrix()
        e.align_seeds()
        if base == 1 << 32:
            e.transitive_reduction(0.65, 1000)
            for graph in ("overlaps", "string"):
                with pytest.raises(elba_amd.ElbaError) as err:
                    e.graph_components(graph)
                assert err.value.status == UNSUPPORTED and "32 bit" in str(err.value)
            with pytest.raises(elba_amd.ElbaError) as err:
                e.partition_components(2, nreads=M)
            assert err.value.status == UNSUPPORTED
            break
        ov = e.export_overlaps()
        assert int(ov["rows"].min()) >= base and int((ov["vals"]["passed"] != 0).sum()) > M
        co, sto = _overlaps(e, M, ov["rows"], ov["cols"], ov["vals"], lens=lens, base=base)
        assert int(co["first_read"][0]) == base and sto["largest_reads"] > M // 2
        e.transitive_reduction(0.65, 1000)
        flags = e.export_read_flags(M)
        cs, sts = _string(e, M, lens=lens, base=base)
        dropped = np.flatnonzero(flags & 3)                      # bad and contained reads: lone in S, with their partners among the overlaps
        assert len(dropped) > 0 and (cs["reads"][cs["comp_of_read"][dropped]] == 1).all()
        u, v = ku.edges_of_overlaps(ov["rows"] - base, ov["cols"] - base, ov["vals"])
        with_edge = np.isin(dropped, np.concatenate([u, v]))
        assert with_edge.any() and (co["reads"][co["comp_of_read"][dropped[with_edge]]] >= 2).all()
        seen[base] = (co, cs)
    for a, b in zip(seen[0], seen[1000]):                        # the base moves first_read and nothing else
        assert (a["comp_of_read"] == b["comp_of_read"]).all() and (a["first_read"] + 1000 == b["first_read"]).all() and (a["bases"] == b["bases"]).all()
    order = np.lexsort((ov["cols"], ov["rows"]))                 # (the last export: base 1000)
    lr, lc, lv = ov["rows"][order] - 1000, ov["cols"][order] - 1000, ov["vals"][order]
    f = elba_amd.Engine(17, 2, 30)                               # the same pairs as a loaded list on another context
    f.set_reads(packed, off, lens)
    f.set_overlaps(M, lr, lc, lv)
    cl, stl = _overlaps(f, M, lr, lc, lv, lens=lens)
    assert ku.same_tables(cl, seen[0][0]) is None
    f.close()
    e.close()


# ---- random graphs ---------------------------------------------------------------------------------------------------------------------
def test_two_hundred_random_graphs_around_the_connectivity_threshold(eng):
    rng = np.random.default_rng(12)
    for it in range(200):
        M = int(rng.integers(1, 3001))
        ne = int(M * (0.3, 0.5, 0.6, 1.0)[it % 4]) if it % 9 else int(rng.integers(0, 4))
        M, u, v = ku.random_graph(rng, M, ne)
        passed = (rng.random(len(u)) < 0.8).astype(np.uint8)
        rows, cols, vals = _load(eng, M, u, v, rng, passed=passed)
        _string(eng, M)
        _overlaps(eng, M, rows, cols, vals)


def _mapped(perm, a, b):
    """b is a with read v renamed perm[v]: the same sets of reads, the same counts per set."""
    first = np.array([perm[np.flatnonzero(a["comp_of_read"] == c)].min() for c in range(len(a["reads"]))]) if len(a["reads"]) < 2000 else None
    image = b["comp_of_read"][perm[a["first_read"]]]
    assert len(np.unique(image)) == len(a["reads"]) == len(b["reads"])
    assert (b["comp_of_read"][perm] == image[a["comp_of_read"]]).all()
    for k in ("reads", "edges", "branches", "ends", "bases"):
        assert (b[k][image] == a[k]).all(), k
    if first is not None:
        assert (b["first_read"][image] == first).all()


def test_a_layout_of_20000_reads_with_hubs_three_calls_and_a_relabelling():
    M = 20000
    rows, cols, vals = sg.layout_with_hub_degrees(31, M, 3, ((5000, 90), (15000, 300)), L=2000)
    e = elba_amd.Engine(17, 2, 8)
    e.set_overlaps(M, rows, cols, vals)
    e.transitive_reduction(0.65, 1000)
    runs = [(_string(e, M), _overlaps(e, M, rows, cols, vals), e.partition_components(5, nreads=M), e.partition_components(5, graph="overlaps", nreads=M)) for _ in range(3)]
    (cs, sts), (co, sto), (ps, ws), (pov, wo) = runs[0]
    assert sts["components"] > sto["components"] > 1 and sts["largest_reads"] > 100
    for (cs2, _), (co2, _), (ps2, ws2), (pov2, wo2) in runs[1:]:       # three calls are bit-identical
        assert all(cs2[k].tobytes() == cs[k].tobytes() and co2[k].tobytes() == co[k].tobytes() for k in cs)
        assert ps2.tobytes() == ps.tobytes() and ws2.tobytes() == ws.tobytes() and pov2.tobytes() == pov.tobytes() and wo2.tobytes() == wo.tobytes()
    assert (ps == ku.partition_of_reads(cs, 5)[0]).all() and (ws == ku.partition_of_reads(cs, 5)[1]).all()
    assert (pov == ku.partition_of_reads(co, 5)[0]).all() and (wo == ku.partition_of_reads(co, 5)[1]).all()
    perm = np.random.default_rng(32).permutation(M)
    prows, pcols, pvals = sg.relabel(perm, rows, cols, vals)
    e.set_overlaps(M, prows, pcols, pvals)
    e.transitive_reduction(0.65, 1000)
    (pcs, _), (pco, _) = _string(e, M), _overlaps(e, M, prows, pcols, pvals)
    _mapped(perm, cs, pcs)
    _mapped(perm, co, pco)
    e.close()


# ---- S on the move ---------------------------------------------------------------------------------------------------------------------
def test_components_after_the_cleaning_calls_move_s():
    rng = np.random.default_rng(14)
    M = 6000
    rows, cols, vals = sg.layout_overlaps(rng, M, 8)
    e = elba_amd.Engine(17, 2, 8)
    e.set_overlaps(M, rows, cols, vals)
    e.transitive_reduction(0.65, 1000)
    seen = [_string(e, M)[1]["components"]]
    moved = 0
    for call in (lambda: e.clip_tips(4, 1), lambda: e.pop_bubbles(8, 1), lambda: e.cut_bridges(3, 4), lambda: e.clip_tips(6, 3)):
        n0 = e.export_string_graph()["n"]
        call()
        moved += e.export_string_graph()["n"] != n0
        seen.append(_string(e, M)[1]["components"])             # S is in its other buffer after an odd number of moves
        _overlaps(e, M, rows, cols, vals)                        # the pairs did not move
    assert moved >= 1 and seen[-1] > seen[0]                     # removed reads are lone components now
    e.close()


def test_one_context_over_50000_then_10_then_50000_reads():
    e = elba_amd.Engine(17, 2, 8)
    rng = np.random.default_rng(15)
    for M, ne in ((50000, 30000), (10, 6), (50000, 24000)):
        M, u, v = ku.random_graph(rng, M, ne)
        rows, cols, vals = _load(e, M, u, v, rng)
        _string(e, M)
        _overlaps(e, M, rows, cols, vals)
    e.close()


# ---- against the other stages ------------------------------------------------------------------------------------------------------------
def test_chains_links_and_the_gfa_agree_with_the_components(tmp_path):
    rng = np.random.default_rng(9)
    genome, seqs, edges, ids, rc = gu.truth_graph(rng, 9000, 40, (5, 7, 9, 20, 37), drop_middle=True)
    lone = cu.random_reads(rng, 3, 30, 40)                       # three reads without an edge: single-read contigs, components of their own
    seqs = seqs + lone
    M = len(seqs)
    rows, cols, vals = cu.upper(edges)
    e = elba_amd.Engine(17, 2, 8)
    e.set_reads(*cu.pack(seqs))
    e.set_overlaps(M, rows, cols, vals)
    e.transitive_reduction(0.0, 0)
    e.generate_contigs(circular=True, singletons=True)
    recs, st = e.assembly_links()
    assert st["twisted"] == 0 and st["unplaced"] == 0 and st["links"] > 0
    c = e.export_contigs()
    cc, cst = _string(e, M)
    comp = cc["comp_of_read"]
    for k in range(c["n"]):                                      # every chain's reads share one component
        assert len(set(comp[c["chain_read"][c["chain_off"][k]:c["chain_off"][k + 1]]].tolist())) == 1
    of_contig = formats.contig_components(comp, c["chain_off"], c["chain_read"])
    assert (of_contig[recs["from"]] == of_contig[recs["to"]]).all()             # both contigs of every link share one
    out, fa = tmp_path / "a.gfa", tmp_path / "a.fa"
    formats.write_gfa(str(out), c["seqs"], c["kinds"], recs, chains=c["chain_off"], component=of_contig)
    version, segs, links = gu.parse_gfa(str(out))
    assert gu.gfa_components(segs, links) == len(set(of_contig.tolist())) == 4
    assert [tags["cc"] for _, _, tags in segs] == of_contig.tolist()            # the cc:i: tags parse back
    formats.write_contigs_fasta(str(fa), c["seqs"], kinds=c["kinds"], components=of_contig)
    heads = [line for line in fa.read_text().split("\n") if line.startswith(">")]
    assert [int(h.rsplit("component=", 1)[1]) for h in heads] == of_contig.tolist()
    e.close()


# ---- the partition ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nparts", [1, 2, 3, 8, 64])
def test_the_partition_equals_the_restatement(eng, nparts):
    rng = np.random.default_rng(16)
    g = ku.random_graph(rng, 200, 55)                            # a few dozen components of two or more reads, fewer than 64
    sizes = [7, 7, 7, 7, 5, 5, 3, 3, 3, 2, 2, 2, 2, 1, 1]        # ... beside paths of equal sizes, where the tie rule decides
    M, us, vs = g[0], [g[1]], [g[2]]
    for n in sizes:
        if n > 1:
            us.append(np.arange(M, M + n - 1)); vs.append(np.arange(M + 1, M + n))
        M += n
    u, v = np.concatenate(us), np.concatenate(vs)
    packed, off, lens = cu.random_packed(rng, M, 20, 60)
    eng.set_reads(packed, off, lens)                             # (new reads drop the pairs: the reads come first)
    rows, cols, vals = _load(eng, M, u, v, rng)
    cc, st = _string(eng, M, lens=lens)
    assert 20 < st["used_components"] < 64
    for weight in ("reads", "bases"):
        for min_reads in (1, 2, 3):
            part, pw = eng.partition_components(nparts, weight=weight, min_reads=min_reads, nreads=M)
            wpart, wpw = ku.partition_of_reads(cc, nparts, weight, min_reads)
            assert (part == wpart).all() and (pw == wpw).all(), (weight, min_reads)
            assert ((part >= 0) == (cc["reads"][cc["comp_of_read"]] >= min_reads)).all() and part.max() < nparts
            dealt = cc[weight][cc["reads"] >= min_reads]
            assert pw.sum() == dealt.sum() and pw.max() - pw.min() <= dealt.max()
            po_part, po_pw = eng.partition_components(nparts, graph="overlaps", weight=weight, min_reads=min_reads, nreads=M)
            assert (po_part == part).all() and (po_pw == pw).all()              # every pair passed: the same graph
    if nparts == 64:
        assert (eng.partition_components(64, nreads=M)[1] == 0).sum() == 64 - st["used_components"]        # more parts than components: the rest stay empty
    part, _ = eng.partition_components(nparts)                   # the binding finds the read count itself
    assert len(part) == M
