"""The assembly-graph rule (elba_export_assembly_links, include/elba_amd.h) on the CPU: the hand cases' claims, the two restatements of
gfa_util.py against each other, the sequence property on ground-truth graphs — which is what pins the orientation rule — and the GFA
writer against the test parser.  No GPU: the contigs are those of contig_ex_util.generate_contigs_ex."""
import ctypes

import numpy as np
import pytest

import contig_ex_util as cx
import contig_util as cu
import elba_amd
import gfa_util as gu
from elba_amd import capi, formats

CASES = gu.hand_cases()


def _both(inp):
    a, sa = gu.links_walk(inp)
    b, sb = gu.links_tables(inp)
    assert sa == sb, (sa, sb)
    assert gu.same_records(a, b), (a, b)
    assert sa["candidates"] == sa["links"] + sa["twisted"] + sa["unplaced"] and len(a) == sa["links"] + sa["closures"]
    keys = list(zip(a["from_read"].tolist(), a["to_read"].tolist()))
    assert keys == sorted(set(keys))
    return a, sa


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_cases_hold_their_claims_in_both_restatements(name):
    case = CASES[name]
    (rows, cols, vals), seqs = gu.case_graph(case)
    inp, contigs = gu.inputs_of_restatement(case["M"], rows, cols, vals, seqs, case["flags"], case["read_flags"])
    recs, st = _both(inp)
    case["claims"](recs, st, inp["read_contig"].tolist())


def test_the_hand_cases_cover_what_they_are_there_for():
    seen = dict.fromkeys(gu.STATS, 0)
    revs = set()
    for case in CASES.values():
        (rows, cols, vals), seqs = gu.case_graph(case)
        recs, st = gu.links_walk(gu.inputs_of_restatement(case["M"], rows, cols, vals, seqs, case["flags"])[0])
        for k in gu.STATS:
            seen[k] = max(seen[k], st[k])
        revs |= set(zip(recs["from_rev"].tolist(), recs["to_rev"].tolist()))
    assert all(seen[k] > 0 for k in gu.STATS) and revs == {(0, 0), (0, 1), (1, 0), (1, 1)}


def test_a_graph_after_clip_tips_with_flagged_reads():
    before, after, flags = gu.clipped_case()
    seqs = [cx.random_genome(np.random.default_rng(3), 100) for _ in range(8)]
    inp0, _ = gu.inputs_of_restatement(8, *before, seqs, 3)
    recs0, st0 = _both(inp0)
    assert st0["links"] == 3 and st0["segments"] == 4            # the branch, the lone read and the two arms
    assert flags.tolist() == [0, 4, 0, 0, 0, 0, 0, 0]
    inp, contigs = gu.inputs_of_restatement(8, *after, seqs, 3, flags)
    recs, st = _both(inp)
    assert st == dict(segments=1, candidates=0, links=0, closures=0, twisted=0, unplaced=0, clamped=0, asymmetric=0) and len(recs) == 0
    assert inp["read_contig"].tolist() == [0, -1, 0, 0, 0, 0, 0, 0]


@pytest.mark.parametrize("seed,M", [(1, 12), (2, 60), (3, 300), (4, 300), (5, 1500)])
def test_the_restatements_agree_on_random_string_graphs(seed, M):
    """Any direction pair and any valid prefix on every edge: twisted, asymmetric and clamped links all occur."""
    rng = np.random.default_rng(seed)
    seqs = cu.random_reads(rng, M, 1, 80)
    lens = [len(s) for s in seqs]
    rows, cols, vals = cu.symmetric({(int(r), int(c)): v for r, c, v in zip(*cu.random_string_graph(rng, M, lens, n_paths=max(1, M // 6), p_extra=0.2))})
    total = dict.fromkeys(gu.STATS, 0)
    for flags in range(4):
        inp, _ = gu.inputs_of_restatement(M, rows, cols, vals, seqs, flags)
        recs, st = _both(inp)
        assert (st["unplaced"] == 0) == (flags & 2 != 0 or st["candidates"] == 0)
        for k in gu.STATS:
            total[k] += st[k]
    if M >= 300:                                                 # (closures and clamps need a cycle / a short contig: the hand cases have them)
        assert all(total[k] > 0 for k in ("candidates", "links", "twisted", "unplaced", "asymmetric")), total


TRUTH = [(11, 4000, 12, (3,), False), (12, 9000, 40, (2, 4, 17, 30), False), (13, 9000, 40, (5, 7, 9, 20, 37), True), (14, 2500, 9, (1, 6), True), (17, 2500, 9, (1, 5), False),
         (15, 30000, 120, tuple(range(4, 110, 9)), False), (16, 30000, 120, tuple(range(4, 110, 6)) + (7, 9), True)]


def _truth_links(genome, seqs, edges, flags=3):
    rows, cols, vals = cu.symmetric(edges)
    inp, contigs = gu.inputs_of_restatement(len(seqs), rows, cols, vals, seqs, flags)
    recs, st = _both(inp)
    return inp, contigs, recs, st


@pytest.mark.parametrize("seed,glen,n,skips,drop", TRUTH)
def test_the_sequence_property_on_ground_truth_graphs(seed, glen, n, skips, drop, tmp_path):
    """Linear genomes at error 0 with true skip edges: every link's oriented from-segment ends with the bases its oriented to-segment
    begins with; nothing is twisted, clamped or asymmetric; every contig is a piece of the genome; the same after relabelling; and the
    GFA is one connected graph."""
    rng = np.random.default_rng(seed)
    genome, seqs, edges, ids, rc = gu.truth_graph(rng, glen, n, skips, drop_middle=drop)
    inp, contigs, recs, st = _truth_links(genome, seqs, edges)
    assert st["twisted"] == st["clamped"] == st["asymmetric"] == st["unplaced"] == st["closures"] == 0
    per_skip = 4 if drop else 5                                  # a lone skip's links: (i-1, i), (i, i+1), (i, i+2), [(i+1, i+2)], (i+2, i+3)
    assert st["links"] >= len(skips) and st["links"] <= per_skip * len(skips) and (recs["overlap"] > 0).all()
    assert all(c in genome or cu.revcomp(c) in genome for c in contigs)
    assert gu.sequence_property_failures(contigs, recs) == []
    # a wrong orientation would be seen: flipping either side of a link breaks the property on it (overlaps of 16 bases and more: a
    # shorter one can match by chance)
    for side in ("from_rev", "to_rev"):
        flipped = recs[recs["overlap"] >= 16].copy()
        flipped[side] ^= 1
        assert len(flipped) > 0 and len(gu.sequence_property_failures(contigs, flipped)) == len(flipped)
    # relabelled: another permutation of the ids and other reads stored reverse-complemented
    rng2 = np.random.default_rng(seed)
    g2, seqs2, edges2, ids2, rc2 = gu.truth_graph(rng2, glen, n, skips, ids=np.random.default_rng(seed + 100).permutation(n),
                                                  rc=np.random.default_rng(seed + 200).integers(0, 2, n).astype(bool), drop_middle=drop)
    assert g2 == genome and not (ids2 == ids).all()
    inp2, contigs2, recs2, st2 = _truth_links(g2, seqs2, edges2)
    assert {k: st2[k] for k in gu.STATS} == {k: st[k] for k in gu.STATS}
    assert gu.sequence_property_failures(contigs2, recs2) == []
    back, back2 = {int(ids[i]): i for i in range(n)}, {int(ids2[i]): i for i in range(n)}      # the same edges of the layout are links
    assert sorted(tuple(sorted((back[int(r["from_read"])], back[int(r["to_read"])]))) for r in recs) == \
        sorted(tuple(sorted((back2[int(r["from_read"])], back2[int(r["to_read"])]))) for r in recs2)
    assert sorted(recs["overlap"].tolist()) == sorted(recs2["overlap"].tolist())
    # the GFA loads as one connected graph
    path = tmp_path / "truth.gfa"
    formats.write_gfa(str(path), contigs, inp["kinds"], recs, chains=inp["chain_off"])
    version, segs, links = gu.parse_gfa(str(path))
    assert version == "1.0" and gu.gfa_components(segs, links) == 1 and len(links) == len(recs)


def test_a_skip_edge_at_the_genomes_end_is_twisted():
    """Reads 0, 1, 2 with the skip 0 <-> 2: only read 2 has a third neighbour, 0 and 1 form a path, and read 0 overlaps 2 on the same end
    as it overlaps 1 — the side that is interior to the contig.  The same at the other end of the genome.  The other links are true."""
    genome, seqs, edges, ids, rc = gu.truth_graph(np.random.default_rng(17), 2500, 9, (0, 6), at_ends=True)
    inp, contigs, recs, st = _truth_links(genome, seqs, edges)
    assert st["twisted"] == 2 and st["links"] == st["candidates"] - 2 > 0 and st["unplaced"] == st["clamped"] == st["asymmetric"] == 0
    assert gu.sequence_property_failures(contigs, recs) == []


def test_write_gfa_round_trips_through_the_parser(tmp_path):
    case = CASES["circle_beside_a_branch_flags_3"]
    (rows, cols, vals), seqs = gu.case_graph(case)
    inp, contigs = gu.inputs_of_restatement(case["M"], rows, cols, vals, seqs, 3)
    recs, st = _both(inp)
    recs = recs.copy()
    recs["from_rev"][1] = 1; recs["to_rev"][2] = 1               # all four sign pairs in the file
    p = tmp_path / "a.gfa"
    formats.write_gfa(str(p), contigs, inp["kinds"], recs, chains=inp["chain_off"])
    version, segs, links = gu.parse_gfa(str(p))
    assert version == "1.0"
    assert [s[0] for s in segs] == ["contig%d" % i for i in range(len(contigs))] and [s[1] for s in segs] == contigs
    assert [s[2] for s in segs] == [dict(LN=len(c), RC=int(b - a)) for c, a, b in zip(contigs, inp["chain_off"][:-1], inp["chain_off"][1:])]
    assert links == [("contig%d" % r["from"], "-" if r["from_rev"] else "+", "contig%d" % r["to"], "-" if r["to_rev"] else "+", int(r["overlap"])) for r in recs]
    assert links[0] == ("contig0", "+", "contig0", "+", 0)       # the closure of the circular contig
    raw = p.read_bytes()
    assert raw.startswith(b"H\tVN:Z:1.0\nS\tcontig0\t") and raw.count(b"\n") == 1 + len(contigs) + len(recs)
    # chains given one per contig, and none
    q = tmp_path / "b.gfa"
    chains = [list(range(int(a), int(b))) for a, b in zip(inp["chain_off"][:-1], inp["chain_off"][1:])]
    formats.write_gfa(str(q), contigs, inp["kinds"], recs, chains=chains)
    assert q.read_bytes() == raw
    formats.write_gfa(str(q), contigs, inp["kinds"], recs)
    assert b"RC:i:" not in q.read_bytes() and gu.parse_gfa(str(q))[2] == links
    formats.write_gfa(str(q), [], [], recs[:0])
    assert q.read_bytes() == b"H\tVN:Z:1.0\n"
    with pytest.raises(ValueError):
        formats.write_gfa(str(q), contigs, inp["kinds"], recs[1:])          # a circular contig without its closure
    with pytest.raises(ValueError):
        formats.write_gfa(str(q), contigs[:2], inp["kinds"][:2], recs)


def test_the_library_exports_the_entry_points_and_the_abi_version_stays():
    L = elba_amd.load_library()
    assert hasattr(L, "elba_export_assembly_links") and hasattr(L, "elba_free_links") and hasattr(elba_amd.Engine, "assembly_links")
    assert L.elba_abi_version() == 3
    assert capi.LINK_DTYPE.itemsize == 24 and capi.LINK_DTYPE == gu.LINK and ctypes.sizeof(capi.GraphStats) == 72
    assert {"elba_export_assembly_links", "elba_free_links"} <= set(capi.EXPORTED_SYMBOLS)
