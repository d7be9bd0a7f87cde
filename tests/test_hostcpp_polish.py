"""The C++ host mirror of contig polishing (polish_contigs in elba_amd/hostcpp/elba_host.hpp) against the Python binding on ground-truth
layouts with planted errors: the same polished bytes, per-contig counts, per-read records, votes and stats."""
import numpy as np
import pytest

import consensus_util as cs
import contig_util as cu
import elba_amd
import hostcpp_util as hu
import placement_util as pu

FIELDS = ("begQ", "endQ", "begT", "endT", "rc", "score", "passed", "containedQ", "containedT", "direction", "directionT", "suffix", "suffixT")


def _inputs(tmp_path, seed, glen, nchain, circular, ncont, nextra, nerr):
    t = pu.truth_set(np.random.default_rng(seed), glen, nchain, circular, ncont, nextra)
    seqs, _ = cs.mutate_truth(t, np.random.default_rng(seed + 1000), nerr)
    fa, pr = tmp_path / "reads.fa", tmp_path / "pairs.txt"
    hu.write_fasta(fa, seqs)
    rows, cols, vals = t["pairs"]
    with open(pr, "w") as f:
        for r, c, v in zip(rows, cols, vals):
            f.write("%d %d %s\n" % (r, c, " ".join(str(int(v[k])) for k in FIELDS)))
    return t, seqs, fa, pr


def _args(tmp_path, fa, pr, flags, skip, band, max_diff, min_depth):
    out = tmp_path / "cpp.txt"
    return [hu.binary("test_host_polish"), fa, pr, flags, skip, band, repr(max_diff), min_depth, out], out


def test_polish_mirror_builds_and_fails_loudly_without_gpu(tmp_path):
    t, seqs, fa, pr = _inputs(tmp_path, 7, 600, 6, False, 45, 3, 8)
    args, _ = _args(tmp_path, fa, pr, 1, 1, 64, 0.25, 3)
    got = hu.runs_or_reports_no_device(args)
    assert got is None or got["nreads"] == 54


@pytest.mark.gpu
@pytest.mark.parametrize("seed,glen,nchain,circular,ncont,nextra,nerr,band", [(2, 1200, 9, True, 80, 8, 14, 64), (7, 600, 6, False, 45, 3, 8, 128)])
def test_polish_mirror_equals_the_python_binding(seed, glen, nchain, circular, ncont, nextra, nerr, band, tmp_path):
    t, seqs, fa, pr = _inputs(tmp_path, seed, glen, nchain, circular, ncont, nextra, nerr)
    args, outf = _args(tmp_path, fa, pr, 3, 1, band, 0.25, 3)
    got = hu.run_json(args[0], args[1:])
    e = elba_amd.Engine(17, 2, 8)
    e.set_reads(*cu.pack(seqs))
    e.set_overlaps(len(seqs), *t["pairs"])
    e.transitive_reduction(0.0, 0)
    e.generate_contigs(circular=True, singletons=True)
    out, st = e.polish_contigs(1, band, 0.25, 3, votes=True)
    want = {k: st[k] for k in cs.STATS}
    want["contigs"] = len(out["seqs"])
    assert got == want and st["voted"] > nchain
    lines = outf.read_text().split("\n")
    nc, M = len(out["seqs"]), len(seqs)
    for k in range(nc):
        assert lines[k] == "%d %d %d %d %s" % (out["voters"][k], out["substituted"][k], out["deleted"][k], out["inserted"][k], out["seqs"][k])
    assert lines[nc:nc + M] == ["%d %d %d %d" % tuple(int(x) for x in r) for r in out["reads"]]
    at = nc + M
    assert lines[at:at + len(out["col"])] == [" ".join(str(int(x)) for x in row) for row in out["col"]]
    at += len(out["col"])
    assert lines[at:at + len(out["gap"])] == [" ".join(str(int(x)) for x in row) for row in out["gap"]]
    assert lines[at + len(out["gap"]):] == [""]
    e.close()
