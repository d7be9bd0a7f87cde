"""The C++ host mirror of the components (graph_components and partition_components in elba_amd/hostcpp/elba_host.hpp) against the
Python binding on two loaded graphs: the same component of every read in both graphs, the same tables, the same parts."""
import numpy as np
import pytest

import comp_util as ku
import contig_util as cu
import elba_amd
import gfa_util as gu
import hostcpp_util as hu
from oracle import pyoracle as po


def _hub_rings_and_lone_reads(rng):
    """A hub of 65 neighbours, thirty of them with a tail, beside two rings and 150 reads without an edge."""
    M = 300
    seqs = cu.random_reads(rng, M, 4, 40)
    lens = [len(s) for s in seqs]
    ids = rng.permutation(M)
    hub, nb, tails = ids[0], ids[1:66], ids[66:96]
    pairs = [(hub, v) for v in nb] + list(zip(nb[:30], tails))
    for ring in (ids[100:140], ids[140:147]):
        pairs += list(zip(ring, np.roll(ring, -1)))
    edges = {(int(min(a, b)), int(max(a, b))): cu.edge(rng, lens[min(a, b)], lens[max(a, b)]) for a, b in pairs}
    return seqs, edges


def _truth(rng):
    genome, seqs, edges, ids, rc = gu.truth_graph(rng, 9000, 40, (5, 7, 9, 20, 37), drop_middle=True)
    return seqs + cu.random_reads(rng, 4, 20, 30), edges


def _write_inputs(tmp_path, seqs, edges):
    fa, ed = tmp_path / "reads.fa", tmp_path / "edges.txt"
    hu.write_fasta(fa, seqs)
    rows, cols, vals = cu.upper(edges)
    with open(ed, "w") as f:
        for r, c, v in zip(rows, cols, vals):
            f.write("%d %d %d %d %d %d\n" % (r, c, v["direction"], v["directionT"], v["suffix"], v["suffixT"]))
    return fa, ed, (rows, cols, vals)


def test_components_mirror_builds_and_fails_loudly_without_gpu(tmp_path):
    seqs, edges = _truth(np.random.default_rng(1))
    fa, ed, _ = _write_inputs(tmp_path, seqs, edges)
    got = hu.runs_or_reports_no_device([hu.binary("test_host_components"), fa, ed, 3, tmp_path / "o.txt"])
    assert got is None or got["reads"] == 44


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["hub_rings_and_lone_reads", "ground_truth"])
def test_components_mirror_equals_the_python_binding(which, tmp_path):
    seqs, edges = (_hub_rings_and_lone_reads if which == "hub_rings_and_lone_reads" else _truth)(np.random.default_rng(9))
    fa, ed, (rows, cols, vals) = _write_inputs(tmp_path, seqs, edges)
    out = tmp_path / "cpp.txt"
    got = hu.run_json(hu.binary("test_host_components"), [fa, ed, 3, out])
    M = len(seqs)
    e = elba_amd.Engine(17, 2, 8)
    packed, off, lens = cu.pack(seqs)
    e.set_reads(packed, off, lens)
    full = np.zeros(len(rows), dtype=po.OVERLAP_DTYPE)          # what the mirror's text carries: the four fields the stages read, passed
    for f in ("direction", "directionT", "suffix", "suffixT"):
        full[f] = vals[f]
    full["passed"] = 1
    e.set_overlaps(M, rows, cols, full)
    e.transitive_reduction(0.0, 0)
    assert e.export_string_graph()["n"] == 2 * len(rows) == got["string_nnz"]
    cs, st = e.graph_components("string", bases=True)
    co, sto = e.graph_components("overlaps")
    part, pw = e.partition_components(3, weight="bases", nreads=M)
    want = ku.tables(M, rows, cols, lens=lens)                  # every pair passed and the reduction kept them: one graph
    assert ku.same_tables(cs, want) is None and ku.same_tables(co, ku.tables(M, rows, cols)) is None
    assert got == dict(reads=M, string_nnz=2 * len(rows), components=st["components"], used_components=st["used_components"], isolated=st["isolated"],
                       largest_reads=st["largest_reads"], largest_bases=st["largest_bases"], edges=st["edges"], overlap_components=sto["components"], overlap_edges=sto["edges"])
    lines = out.read_text().splitlines()
    n = st["components"]
    assert len(lines) == M + n + 1 and st["isolated"] > 0 and st["used_components"] >= (3 if which == "hub_rings_and_lone_reads" else 1)
    per_read = np.array([[int(x) for x in line.split()] for line in lines[:M]])
    assert (per_read[:, 0] == cs["comp_of_read"]).all() and (per_read[:, 1] == co["comp_of_read"]).all() and (per_read[:, 2] == part).all()
    per_comp = np.array([[int(x) for x in line.split()] for line in lines[M:M + n]])
    for i, k in enumerate(ku.TABLES):
        assert (per_comp[:, i] == cs[k]).all(), k
    assert [int(x) for x in lines[-1].split()] == pw.tolist() == ku.partition_of_reads(cs, 3, "bases")[1].tolist()
    e.close()
