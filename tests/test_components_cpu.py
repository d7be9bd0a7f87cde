"""The component rule (elba_graph_components / elba_partition_components, include/elba_amd.h) on the CPU: the two restatements of
comp_util.py against each other under many edge orders, the hand cases' claims, the builders' own conditions and the rounds the
vectorised form takes on them, the partition against a brute-force re-run of the loop and its guarantee, relabelled graphs, the GFA and
FASTA writers' component columns, and the library's symbols.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

import comp_util as ku
import elba_amd
import gfa_util as gu
import string_graph_util as sg
from elba_amd import capi, formats
from oracle import pyoracle as po

CASES = ku.hand_cases()
PASS_CAP = 512          # what the GPU tests allow a labelling of the 131 073-read path


def _both(M, u, v):
    a = ku.union_find(M, u, v)
    b, rounds = ku.min_label(M, u, v)
    assert (a == b).all()
    assert (a <= np.arange(M)).all() and (a[a] == a).all()            # a label is a smaller read of the component, and a fixed point
    return a, rounds


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_cases_hold_their_claims_in_both_restatements(name):
    case = CASES[name]
    M, u, v = ku.case_edges(case)
    labels, _ = _both(M, u, v)
    ku.check_case(case, ku.tables(M, u, v, labels))
    ku.check_case(case, ku.tables(M, v, u))                          # the orientation of an edge says nothing
    st = ku.stats(ku.tables(M, u, v))
    assert st["nreads"] == M and st["edges"] == len(u) and st["components"] == st["used_components"] + st["isolated"] == len(case["edges"])


def test_there_are_about_thirty_hand_cases_and_they_cover_every_shape():
    shapes = {s for c in CASES.values() for s in c["shapes"]}
    assert len(CASES) >= 30 and shapes == {"lone", "path", "ring", "other"}
    assert any(len(set(c["comp"])) >= 3 for c in CASES.values())


def test_the_two_forms_agree_under_twenty_edge_orders():
    rng = np.random.default_rng(11)
    for M, ne in ((1, 0), (2, 1), (40, 15), (300, 140), (300, 160), (300, 600), (2000, 1000)):
        M, u, v = ku.random_graph(rng, M, ne)
        want = ku.tables(M, u, v)
        for _ in range(20):
            order = rng.permutation(len(u))
            flip = rng.random(len(u)) < 0.5
            uu, vv = np.where(flip, v, u)[order], np.where(flip, u, v)[order]
            labels, _ = _both(M, uu, vv)
            assert ku.same_tables(ku.tables(M, uu, vv, labels), want) is None


def test_the_builders_keep_their_own_conditions():
    rng = np.random.default_rng(2)
    for kind in ku.NUMBERINGS:
        ids = ku.numbering(1001, kind, rng)
        assert sorted(ids.tolist()) == list(range(1001))
        M, u, v = ku.path(1001, kind, rng)
        t = ku.tables(M, u, v)
        assert len(u) == 1000 and t["reads"].tolist() == [1001] and t["ends"].tolist() == [2] and t["branches"].tolist() == [0]
        M, u, v = ku.ring(1001, kind, rng)
        t = ku.tables(M, u, v)
        assert t["edges"].tolist() == [1001] and ku.shape(1001, int(t["branches"][0]), int(t["ends"][0])) == "ring"
    assert ku.numbering(7, "alternating").tolist() == [0, 6, 1, 5, 2, 4, 3]
    for first in (True, False):
        M, u, v = ku.star(70, first)
        t = ku.tables(M, u, v)
        assert M == 71 and t["branches"].tolist() == [1] and t["ends"].tolist() == [70] and set(u.tolist()) == {0 if first else 70}
    M, u, v = ku.binary_tree(5)
    t = ku.tables(M, u, v)
    assert M == 63 and t["edges"].tolist() == [62] and t["ends"].tolist() == [32] and t["branches"].tolist() == [30]
    M, u, v = ku.caterpillar(50)
    t = ku.tables(M, u, v)
    assert M == 100 and t["edges"].tolist() == [99] and t["ends"].tolist() == [50] and t["branches"].tolist() == [48]       # the two end reads of the spine have degree 2
    M, u, v = ku.isolated_pairs(40)
    t = ku.tables(M, u, v)
    assert M == 120 and t["reads"].tolist() == [2, 1] * 40 and t["first_read"].tolist() == [x for k in range(40) for x in (3 * k, 3 * k + 1)]
    M, u, v = ku.two_giants(30)
    r, c = ku.sorted_pairs(u, v)
    assert (int(r[-1]), int(c[-1])) == (58, 59)
    without = ku.tables(M, r[:-1], c[:-1])
    assert without["reads"].tolist() == [30, 30] and ku.tables(M, r, c)["reads"].tolist() == [60]
    assert ku.tables(M, r, c)["ends"].tolist() == [2]


def test_the_vectorised_form_needs_logarithmic_rounds_where_plain_propagation_needs_the_diameter():
    M = (1 << 17) + 1
    rng = np.random.default_rng(3)
    for kind in ku.NUMBERINGS:
        _, u, v = ku.path(M, kind, rng)
        labels, rounds = ku.min_label(M, u, v)
        assert (labels == 0).all() and rounds <= PASS_CAP, (kind, rounds)
    for build in (lambda: ku.binary_tree(16), lambda: ku.caterpillar(1 << 16, "alternating")):
        m, u, v = build()
        labels, rounds = ku.min_label(m, u, v)
        assert (labels == 0).all() and rounds <= PASS_CAP, rounds


def test_a_pair_with_one_image_in_s_is_one_edge():
    """The oracle's reduction keeps one image of a pair that lacks a direction on one side; the edges of S are its pairs, each once."""
    rng = np.random.default_rng(6)
    M, u, v = ku.path(30, "random", rng)
    rows, cols = ku.sorted_pairs(u, v)
    vals = ku.overlap_records(rng, len(rows), po.OVERLAP_DTYPE)
    which = np.arange(len(rows)) % 3
    vals["direction"][which == 1] = -1
    vals["directionT"][which == 2] = -1
    S, flags, st = po.string_graph(M, rows, cols, vals, cutoff=0.0, fuzz=0)
    assert 0 < int((S["rows"] > S["cols"]).sum()) < M - 1 and 0 < int((S["rows"] < S["cols"]).sum()) < M - 1 and len(S["rows"]) < 2 * (M - 1)
    eu, ev = ku.edges_of_string_graph(S)
    assert len(eu) == M - 1 and (eu > ev).all() and sorted(zip(ev.tolist(), eu.tolist())) == list(zip(rows.tolist(), cols.tolist()))
    t = ku.tables(M, eu, ev)
    assert t["reads"].tolist() == [M] and t["ends"].tolist() == [2] and t["branches"].tolist() == [0]
    empty = ku.edges_of_string_graph(dict(rows=np.zeros(0, np.int64), cols=np.zeros(0, np.int64)))
    assert len(empty[0]) == 0 == len(empty[1])


def _brute_partition(reads, weight, nparts, min_reads):
    todo = [c for c in range(len(reads)) if reads[c] >= min_reads]
    sums, poc = np.zeros(nparts, dtype=np.int64), np.full(len(reads), -1)
    while todo:
        c = min(todo, key=lambda x: (-int(weight[x]), x))            # the heaviest left, the smaller component on a tie
        todo.remove(c)
        p = int(np.argmin(sums))                                     # (argmin: the first of the smallest)
        sums[p] += int(weight[c]); poc[c] = p
    return poc, sums


def test_the_partition_is_the_loop_and_keeps_its_guarantee():
    rng = np.random.default_rng(8)
    for it in range(200):
        n = int(rng.integers(0, 50))
        reads = rng.integers(1, 6, n)
        weight = reads.copy() if it % 2 else rng.integers(0, (3, 500, 1 << 40)[it % 3], n)
        nparts, min_reads = int(rng.integers(1, 80 if it % 4 == 0 else 7)), int(rng.integers(1, 3))
        poc, pw = ku.partition(reads, weight, nparts, min_reads)
        bpoc, bpw = _brute_partition(reads, weight, nparts, min_reads)
        assert poc.tolist() == bpoc.tolist() and pw.tolist() == bpw.tolist()
        dealt = weight[reads >= min_reads]
        assert pw.sum() == dealt.sum() and pw.max() - pw.min() <= (dealt.max() if len(dealt) else 0)
        assert ((poc >= 0) == (reads >= min_reads)).all()
    poc, pw = ku.partition([5] * 7, [5] * 7, 3)
    assert poc.tolist() == [0, 1, 2, 0, 1, 2, 0] and pw.tolist() == [15, 10, 10]


def test_a_relabelled_graph_gives_the_mapped_partition():
    rng = np.random.default_rng(21)
    for M, density in ((30, 0.05), (60, 0.03), (120, 0.012)):
        rows, cols, vals = sg.random_overlaps(rng, M, density=density, p_fail=0.3)
        perm = rng.permutation(M)
        prows, pcols, pvals = sg.relabel(perm, rows, cols, vals)
        a = ku.tables(M, *ku.edges_of_overlaps(rows, cols, vals))
        b = ku.tables(M, *ku.edges_of_overlaps(prows, pcols, pvals))
        sets_a = {frozenset(perm[np.flatnonzero(a["comp_of_read"] == c)].tolist()) for c in range(len(a["reads"]))}
        sets_b = {frozenset(np.flatnonzero(b["comp_of_read"] == c).tolist()) for c in range(len(b["reads"]))}
        assert sets_a == sets_b and len(sets_a) < M
        for k in ("reads", "edges", "branches", "ends"):                # the same components with the same counts, numbered anew
            first = b["first_read"][b["comp_of_read"][perm[a["first_read"]]]]
            assert (b[k][b["comp_of_read"][perm[a["first_read"]]]] == a[k]).all(), k
            assert (first == np.array([min(perm[np.flatnonzero(a["comp_of_read"] == c)]) for c in range(len(a["reads"]))])).all()


def _fake_assembly(rng, n, nlinks):
    seqs = ["ACGT" * int(rng.integers(1, 5)) for _ in range(n)]
    recs = np.zeros(nlinks, dtype=capi.LINK_DTYPE)
    recs["from"] = rng.integers(0, n, nlinks); recs["to"] = rng.integers(0, n, nlinks)
    recs["from_rev"] = rng.integers(0, 2, nlinks); recs["to_rev"] = rng.integers(0, 2, nlinks); recs["overlap"] = rng.integers(0, 4, nlinks)
    return seqs, recs


def test_the_gfa_parser_counts_the_components_the_tags_name(tmp_path):
    rng = np.random.default_rng(4)
    for n, nlinks in ((1, 0), (6, 3), (40, 18), (40, 60)):
        seqs, recs = _fake_assembly(rng, n, nlinks)
        t = ku.tables(n, recs["from"].astype(np.int64), recs["to"].astype(np.int64))
        path = tmp_path / ("g%d_%d.gfa" % (n, nlinks))
        formats.write_gfa(str(path), seqs, None, recs, component=t["comp_of_read"])
        version, segs, links = gu.parse_gfa(str(path))
        assert gu.gfa_components(segs, links) == len(t["reads"]) == len({tags["cc"] for _, _, tags in segs})
        assert [tags["cc"] for _, _, tags in segs] == t["comp_of_read"].tolist()
        for a, _, b, _, _ in links:                                     # a link never leaves its component
            assert segs[int(a[6:])][2]["cc"] == segs[int(b[6:])][2]["cc"]


def test_without_the_new_arguments_every_byte_is_as_before(tmp_path):
    seqs, recs = _fake_assembly(np.random.default_rng(6), 5, 4)
    a, b, c = tmp_path / "a.gfa", tmp_path / "b.gfa", tmp_path / "c.gfa"
    formats.write_gfa(str(a), seqs, None, recs, chains=[0, 1, 3, 4, 6, 7], depth=[4, 8, 0, 2, 9])
    formats.write_gfa(str(b), seqs, None, recs, chains=[0, 1, 3, 4, 6, 7], depth=[4, 8, 0, 2, 9], component=None)
    formats.write_gfa(str(c), seqs, None, recs, chains=[0, 1, 3, 4, 6, 7], depth=[4, 8, 0, 2, 9], component=[0, 0, 1, 2, 2])
    assert a.read_bytes() == b.read_bytes()
    want = a.read_bytes().split(b"\n")
    comp = iter([0, 0, 1, 2, 2])
    want = b"\n".join(line + b"\tcc:i:%d" % next(comp) if line.startswith(b"S\t") else line for line in want)
    assert c.read_bytes() == want
    assert a.read_bytes().startswith(b"H\tVN:Z:1.0\nS\tcontig0\t" + seqs[0].encode() + b"\tLN:i:%d\tRC:i:1\tDP:f:" % len(seqs[0]))
    with pytest.raises(ValueError):
        formats.write_gfa(str(c), seqs, None, recs, component=[0, 0])
    fa, fb, fc = tmp_path / "a.fa", tmp_path / "b.fa", tmp_path / "c.fa"
    formats.write_contigs_fasta(str(fa), seqs, first=3, kinds=[0, 1, 2, 0, 1])
    formats.write_contigs_fasta(str(fb), seqs, first=3, kinds=[0, 1, 2, 0, 1], components=None)
    formats.write_contigs_fasta(str(fc), seqs, first=3, kinds=[0, 1, 2, 0, 1], components=[0, 0, 1, 2, 2])
    assert fa.read_bytes() == fb.read_bytes() == b"".join(b">contig%d%s\n%s\n" % (i + 3, b" circular" if k == 1 else b"", s.encode())
                                                          for i, (s, k) in enumerate(zip(seqs, [0, 1, 2, 0, 1])))
    heads = [line for line in fc.read_bytes().split(b"\n") if line.startswith(b">")]
    assert heads == [b">contig3 component=0", b">contig4 circular component=0", b">contig5 component=1", b">contig6 component=2", b">contig7 circular component=2"]
    with pytest.raises(ValueError):
        formats.write_contigs_fasta(str(fc), seqs, components=[1])


def test_a_contigs_component_is_that_of_its_first_chain_read():
    comp = np.array([0, 1, 0, 2, 1, 0], dtype=np.int32)
    got = formats.contig_components(comp, [0, 2, 3, 6], [12, 10, 13, 11, 14, 15], id_base=10)
    assert got.tolist() == [0, 2, 1]


def test_the_library_exports_both_symbols_and_the_abi_version_stays():
    L = ctypes.CDLL(elba_amd.lib_path())
    for name in ("elba_graph_components", "elba_free_components", "elba_partition_components"):
        assert hasattr(L, name) and name in capi.EXPORTED_SYMBOLS
    L.elba_abi_version.restype = ctypes.c_int
    assert L.elba_abi_version() == 3
    assert hasattr(elba_amd.Engine, "graph_components") and hasattr(elba_amd.Engine, "partition_components")
    assert ctypes.sizeof(capi.CcCfg) == 16 and ctypes.sizeof(capi.PartCfg) == 32 and ctypes.sizeof(capi.Components) == 9 * 8 and ctypes.sizeof(capi.CcStats) == 7 * 8 + 4 * 4
    header = open(os.path.join(os.path.dirname(elba_amd.lib_path()), "..", "..", "include", "elba_amd.h")).read()
    for word in ("ELBA_CC_STRING", "ELBA_CC_OVERLAPS", "ELBA_CC_BASES", "elba_cc_cfg", "elba_part_cfg", "ascending smallest read", "std::min_element"):
        assert word in header, word
    L.elba_free_components(None)
    assert po.OVERLAP_DTYPE.itemsize == 36
