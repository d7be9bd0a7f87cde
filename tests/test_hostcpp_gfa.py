"""The C++ host mirror of the assembly graph (assembly_links and write_gfa in elba_amd/hostcpp/elba_host.hpp) against the Python binding
on two loaded graphs: the same records, the same counts, the same GFA bytes."""
import numpy as np
import pytest

import contig_util as cu
import elba_amd
import gfa_util as gu
import hostcpp_util as hu
from elba_amd import formats
from oracle import pyoracle as po


def _hub_and_rings(rng):
    """A hub of 65 neighbours (lone reads and ends of two-read paths, any direction pair) beside two rings: links, twisted edges, closures."""
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
    return seqs, edges


def _write_inputs(tmp_path, seqs, edges):
    fa, ed = tmp_path / "reads.fa", tmp_path / "edges.txt"
    hu.write_fasta(fa, seqs)
    rows, cols, vals = cu.upper(edges)
    with open(ed, "w") as f:
        for r, c, v in zip(rows, cols, vals):
            f.write("%d %d %d %d %d %d\n" % (r, c, v["direction"], v["directionT"], v["suffix"], v["suffixT"]))
    return fa, ed, (rows, cols, vals)


def test_gfa_mirror_builds_and_fails_loudly_without_gpu(tmp_path):
    seqs, edges = _truth(np.random.default_rng(1))
    fa, ed, _ = _write_inputs(tmp_path, seqs, edges)
    got = hu.runs_or_reports_no_device([hu.binary("test_host_gfa"), fa, ed, 3, tmp_path / "o.gfa", tmp_path / "o.links"])
    assert got is None or got["reads"] == 40


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["hub_and_rings", "ground_truth"])
def test_gfa_mirror_equals_the_python_binding(which, tmp_path):
    seqs, edges = (_hub_and_rings if which == "hub_and_rings" else _truth)(np.random.default_rng(9))
    fa, ed, (rows, cols, vals) = _write_inputs(tmp_path, seqs, edges)
    out, lk = tmp_path / "cpp.gfa", tmp_path / "cpp.links"
    got = hu.run_json(hu.binary("test_host_gfa"), [fa, ed, 3, out, lk])
    e = elba_amd.Engine(17, 2, 8)
    e.set_reads(*cu.pack(seqs))
    full = np.zeros(len(rows), dtype=po.OVERLAP_DTYPE)          # what the mirror's text carries: the four fields the stages read, passed
    for f in ("direction", "directionT", "suffix", "suffixT"):
        full[f] = vals[f]
    full["passed"] = 1
    e.set_overlaps(len(seqs), rows, cols, full)
    e.transitive_reduction(0.0, 0)
    assert e.export_string_graph()["n"] == 2 * len(rows) == got["string_nnz"]
    e.generate_contigs(circular=True, singletons=True)
    recs, st = e.assembly_links()
    c = e.export_contigs()
    ref = tmp_path / "py.gfa"
    formats.write_gfa(str(ref), c["seqs"], c["kinds"], recs, chains=c["chain_off"])
    assert out.read_bytes() == ref.read_bytes()
    want = {k: st[k] for k in gu.STATS}
    want.update(reads=len(seqs), string_nnz=2 * len(rows), records=len(recs))
    assert got == want
    cpp = np.loadtxt(str(lk), dtype=np.int64, ndmin=2).reshape(-1, 8)
    assert cpp.tolist() == [[int(r[k]) for k in ("from", "to", "from_read", "to_read", "overlap", "from_rev", "to_rev", "flags")] for r in recs]
    assert st["links"] > 0 and (st["closures"] == 2 and st["twisted"] > 0 if which == "hub_and_rings" else st["twisted"] == 0)
    version, segs, links = gu.parse_gfa(str(out))
    assert version == "1.0" and len(segs) == c["n"] and len(links) == len(recs)
    e.close()
