"""The C++ host mirror of the induced sub-problem (induce_part and load_part in elba_amd/hostcpp/elba_host.hpp) against the Python binding on
a built multi-component input: the same parts, the same outside counts, the same read flags and the same S of every part."""
import numpy as np
import pytest

import contig_util as cu
import elba_amd
import hostcpp_util as hu
import induce_util as iu
from oracle import pyoracle as po

FIELDS = ("begQ", "endQ", "begT", "endT", "rc", "score", "passed", "containedQ", "containedT", "direction", "directionT", "suffix", "suffixT")
BLOCKS = (("layout", 120), ("layout", 80), ("layout", 50), ("layout", 9))


def _inputs(tmp_path, seed):
    g = iu.build_input(seed, BLOCKS, n_failed=40, lone=2)
    seqs = cu.seqs_of(*g["reads"])
    fa, pr = tmp_path / "reads.fa", tmp_path / "pairs.txt"
    hu.write_fasta(fa, seqs)
    vals = np.zeros(len(g["vals"]), dtype=po.OVERLAP_DTYPE)      # what the mirror's text carries
    for f in FIELDS:
        vals[f] = g["vals"][f]
    with open(pr, "w") as f:
        for r, c, v in zip(g["rows"], g["cols"], vals):
            f.write("%d %d %s\n" % (r, c, " ".join(str(int(v[k])) for k in FIELDS)))
    return g, seqs, vals, fa, pr


def test_induce_mirror_builds_and_fails_loudly_without_gpu(tmp_path):
    g, seqs, vals, fa, pr = _inputs(tmp_path, 1)
    got = hu.runs_or_reports_no_device([hu.binary("test_host_induce"), fa, pr, 3, tmp_path / "o.txt"])
    assert got is None or got["reads"] == g["M"] == got["part_reads"]


@pytest.mark.gpu
@pytest.mark.parametrize("nparts", [1, 3])
def test_induce_mirror_equals_the_python_binding(nparts, tmp_path):
    g, seqs, vals, fa, pr = _inputs(tmp_path, 2)
    out = tmp_path / "cpp.txt"
    got = hu.run_json(hu.binary("test_host_induce"), [fa, pr, nparts, out])
    M = g["M"]
    e, second = elba_amd.Engine(17, 2, 8), elba_amd.Engine(17, 2, 8)
    e.set_reads(*cu.pack(seqs))
    e.set_overlaps(M, g["rows"], g["cols"], vals)
    part_of_read, _ = e.partition_components(nparts, graph="overlaps", min_reads=1, nreads=M)
    lines = []
    tot = dict(part_reads=0, part_pairs=0, split_pairs=0, split_passed=0, string_nnz=0, bad_reads=0, bases=0)
    for part in range(nparts):
        ind, st = e.induce_part(part_of_read, part)
        second.load_part(ind)
        s = second.transitive_reduction(0.65, 0)
        flags = second.export_read_flags(ind["reads"])
        S = second.export_string_graph()
        old = ind["old_of_new"]
        lines.append("%d %d %d %d %d %d" % (part, ind["reads"], ind["pairs"], st["split_pairs"], st["split_passed"], S["n"]))
        lines += ["%d %d %d %d" % t for t in zip(old.tolist(), ind["outside_aligned"].tolist(), ind["outside_passed"].tolist(), flags.tolist())]
        lines += ["%d %d %d %d" % t for t in zip(old[S["rows"]].tolist(), old[S["cols"]].tolist(), S["vals"]["suffix"].tolist(), S["vals"]["direction"].tolist())]
        for k, v in (("part_reads", ind["reads"]), ("part_pairs", ind["pairs"]), ("split_pairs", st["split_pairs"]), ("split_passed", st["split_passed"]), ("string_nnz", S["n"]),
                     ("bad_reads", s["bad_reads"]), ("bases", st["bases"])):
            tot[k] += int(v)
    assert got == dict(reads=M, parts=nparts, **tot)
    assert tot["part_reads"] == M and tot["split_passed"] == 0 and (tot["split_pairs"] > 0) == (nparts > 1) and tot["string_nnz"] > 0
    assert out.read_text().splitlines() == lines
    second.close(); e.close()
