"""CPU tests of the contig stage's yardsticks: hand-derived answers through the restatement of GenerateContigs (tests/contig_util.py),
the .contigs.fa writer, and the library's new symbols.  The GPU's own contigs are checked in tests/test_gpu_contigs.py."""
import numpy as np
import pytest

import contig_util as cu
import elba_amd
from elba_amd import formats
from oracle import pyoracle as po


def ov(direction, directionT, suffix, suffixT):
    o = np.zeros(1, dtype=po.OVERLAP_DTYPE)[0]
    o["passed"] = 1; o["direction"] = direction; o["directionT"] = directionT; o["suffix"] = suffix; o["suffixT"] = suffixT
    return o


def run(seqs, edges):
    rows, cols, vals = cu.symmetric(edges)
    return cu.generate_contigs(len(seqs), rows, cols, vals, seqs)


def test_forward_three_read_chain():
    seqs = ["ACGTAC", "TACGGA", "GGATTC"]
    contigs, chains, rc, st = run(seqs, {(0, 1): ov(1, 2, 0, 3), (1, 2): ov(1, 2, 0, 2)})
    # S(0,1).suffixT = 3 bases of read 0, S(1,2).suffixT = 2 of read 1, all of read 2; strands (1 >> 1) & 1 = 0 and 1 - (1 & 1) = 0
    assert contigs == ["ACG" + "TA" + "GGATTC"]
    assert chains == [[(0, 3, 0), (1, 2, 0), (2, 6, 0)]]
    assert rc == [0, 0, 0]
    assert st == dict(nreads=3, branches=0, components=1, used_components=1, contigs=1, cycles=0, contig_reads=3, bases=11, longest=11)


def test_reverse_strand_edges():
    seqs = ["AACG", "GGTA"]
    # direction 2: strand (2 >> 1) & 1 = 1 for read 0; the last read gets 1 - (2 & 1) = 1
    contigs, chains, _, _ = run(seqs, {(0, 1): ov(2, 1, 0, 2)})
    assert contigs == ["CG" + "TACC"]
    assert chains == [[(0, 2, 1), (1, 4, 1)]]


def test_two_read_contig_mixed_strands():
    seqs = ["ACCA", "GTTG"]
    contigs, chains, _, st = run(seqs, {(0, 1): ov(3, 0, 1, 1)})     # strand of 0: (3 >> 1) & 1 = 1; of 1: 1 - (3 & 1) = 0
    assert contigs == ["T" + "GTTG"] and chains == [[(0, 1, 1), (1, 4, 0)]]
    assert st["contigs"] == 1 and st["components"] == 1 and st["used_components"] == 1


def test_walk_from_the_higher_id_side_reads_the_transpose():
    # path 1 - 0 - 2: the walk starts at 1 (degree 1, smaller end) and reads S(1,0) = Transpose(S(0,1)): suffixT = S(0,1).suffix,
    # direction = S(0,1).directionT; then S(0,2) as stored
    seqs = ["CCCCCC", "AAAAAA", "GGGGGG"]
    contigs, chains, rc, _ = run(seqs, {(0, 1): ov(1, 1, 4, 2), (0, 2): ov(1, 2, 5, 3)})
    assert chains == [[(1, 4, 0), (0, 3, 0), (2, 6, 0)]]
    assert contigs == ["AAAA" + "CCC" + "GGGGGG"] and rc == [0, 0, 0]


def test_hub_splits_a_path_and_is_dropped():
    seqs = ["AAAA", "CCCC", "GGGG", "TTTT", "ACGT", "TGCA"]
    e = {(0, 1): ov(1, 2, 2, 2), (0, 3): ov(1, 2, 2, 2), (2, 3): ov(1, 2, 2, 2), (3, 4): ov(1, 2, 2, 2), (4, 5): ov(1, 2, 2, 2)}
    contigs, chains, rc, st = run(seqs, e)
    assert contigs == ["AA" + "CCCC", "AC" + "TGCA"]
    assert [[c[0] for c in ch] for ch in chains] == [[0, 1], [4, 5]]
    assert rc == [0, 0, -1, -1, 1, 1]
    # components of S without read 3's edges: {0,1}, {2}, {3}, {4,5}
    assert st["branches"] == 1 and st["components"] == 4 and st["used_components"] == 2 and st["contigs"] == 2 and st["cycles"] == 0


def test_five_cycle_emits_nothing():
    seqs = ["ACGT"] * 5
    e = {(0, 1): ov(1, 2, 1, 1), (1, 2): ov(1, 2, 1, 1), (2, 3): ov(1, 2, 1, 1), (3, 4): ov(1, 2, 1, 1), (0, 4): ov(1, 2, 1, 1)}
    contigs, chains, rc, st = run(seqs, e)
    assert contigs == [] and chains == [] and rc == [-1] * 5
    assert st["cycles"] == 1 and st["components"] == 1 and st["used_components"] == 1 and st["contigs"] == 0


def test_isolated_reads():
    contigs, _, rc, st = run(["ACGT", "CC", "G"], {})
    assert contigs == [] and rc == [-1, -1, -1]
    assert st["components"] == 3 and st["used_components"] == 0 and st["branches"] == 0


def test_lower_id_end_is_the_genome_right_end():
    g = "AAACCCGGGTTTACGT"
    seqs = [g[8:16], g[4:12], g[0:8]]              # read 0 is the rightmost: the walk from 0 runs leftwards, on the reverse strand
    contigs, chains, _, _ = run(seqs, {(0, 1): ov(2, 1, 4, 4), (1, 2): ov(2, 1, 4, 4)})
    assert chains == [[(0, 4, 1), (1, 4, 1), (2, 8, 1)]]
    assert contigs == [cu.revcomp(g)]


def test_bad_prefix_is_an_error():
    with pytest.raises(cu.BadPrefix):
        run(["ACGT", "ACGT"], {(0, 1): ov(1, 2, 0, 5)})
    with pytest.raises(cu.BadPrefix):
        run(["ACGT", "ACGT"], {(0, 1): ov(1, 2, 0, -1)})


def test_random_graphs_are_valid_and_triangle_free():
    rng = np.random.default_rng(3)
    seqs = cu.random_reads(rng, 300)
    rows, cols, vals = cu.random_string_graph(rng, 300, [len(s) for s in seqs])
    adj = [set() for _ in range(300)]
    for i, j in zip(rows.tolist(), cols.tolist()):
        assert i < j
        adj[i].add(j); adj[j].add(i)
    assert all(not (adj[i] & adj[j]) for i, j in zip(rows.tolist(), cols.tolist()))
    assert ((vals["suffixT"] >= 0) & (vals["suffixT"] <= np.array([len(seqs[i]) for i in rows]))).all()
    assert set(vals["direction"].tolist()) == {0, 1, 2, 3}
    S = cu.symmetric({(int(i), int(j)): v for i, j, v in zip(rows, cols, vals)})
    contigs, chains, rc, st = cu.generate_contigs(300, *S, seqs)
    assert st["contigs"] > 0 and st["contig_reads"] == sum(1 for x in rc if x >= 0)


def test_pack_roundtrip():
    rng = np.random.default_rng(1)
    seqs = cu.random_reads(rng, 20, 1, 40)
    assert cu.seqs_of(*cu.pack(seqs)) == seqs


def test_write_contigs_fasta_bytes(tmp_path):
    p = tmp_path / "x.contigs.fa"
    formats.write_contigs_fasta(str(p), ["ACGT", "", "TTGCA"])
    assert p.read_bytes() == b">contig0\nACGT\n>contig1\n\n>contig2\nTTGCA\n"
    formats.write_contigs_fasta(str(p), ["GG"], first=7)
    assert p.read_bytes() == b">contig7\nGG\n"


def test_library_exports_the_contig_symbols():
    L = elba_amd.load_library()
    for n in ("elba_generate_contigs", "elba_export_contigs", "elba_free_contigs", "elba_export_read_contigs"):
        assert hasattr(L, n), n
    assert L.elba_abi_version() == 3
