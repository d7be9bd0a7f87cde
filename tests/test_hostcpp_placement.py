"""The C++ host mirror of the read placements (place_reads, write_placements_paf and write_gfa's depth in elba_amd/hostcpp/elba_host.hpp)
against the Python binding on ground-truth layouts: the same records, segments, credits and counts, the same PAF and GFA bytes."""
import numpy as np
import pytest

import contig_util as cu
import elba_amd
import hostcpp_util as hu
import placement_util as pu
from elba_amd import formats

FIELDS = ("begQ", "endQ", "begT", "endT", "rc", "score", "passed", "containedQ", "containedT", "direction", "directionT", "suffix", "suffixT")


def _write_inputs(tmp_path, t):
    fa, pr = tmp_path / "reads.fa", tmp_path / "pairs.txt"
    hu.write_fasta(fa, t["seqs"])
    rows, cols, vals = t["pairs"]
    with open(pr, "w") as f:
        for r, c, v in zip(rows, cols, vals):
            f.write("%d %d %s\n" % (r, c, " ".join(str(int(v[k])) for k in FIELDS)))
    return fa, pr


def _args(tmp_path, fa, pr, flags, skip):
    out = [tmp_path / n for n in ("cpp.paf", "cpp.gfa", "cpp.records")]
    return [hu.binary("test_host_place"), fa, pr, flags, skip] + out, out


def test_placement_mirror_builds_and_fails_loudly_without_gpu(tmp_path):
    t = pu.truth_set(np.random.default_rng(1), 900, 12, False, 15, 6)
    args, _ = _args(tmp_path, *_write_inputs(tmp_path, t), 1, 1)
    got = hu.runs_or_reports_no_device(args)
    assert got is None or got["nreads"] == 33


@pytest.mark.gpu
@pytest.mark.parametrize("seed,glen,nchain,circular,ncont,nextra,skip", [(2, 1200, 9, True, 20, 8, 1), (5, 1500, 20, False, 30, 12, 1), (5, 1500, 20, False, 30, 12, 2)])
def test_placement_mirror_equals_the_python_binding(seed, glen, nchain, circular, ncont, nextra, skip, tmp_path):
    t = pu.truth_set(np.random.default_rng(seed), glen, nchain, circular, ncont, nextra)
    fa, pr = _write_inputs(tmp_path, t)
    args, (paf, gfa, rec) = _args(tmp_path, fa, pr, 3, skip)
    got = hu.run_json(args[0], args[1:])
    e = elba_amd.Engine(17, 2, 8)
    e.set_reads(*cu.pack(t["seqs"]))
    e.set_overlaps(len(t["seqs"]), *t["pairs"])
    e.transitive_reduction(0.0, 0)
    e.generate_contigs(circular=True, singletons=True)
    pl, st = e.place_reads(skip)
    c = e.export_contigs()
    links, _ = e.assembly_links()
    want = {k: st[k] for k in pu.STATS}
    want["contigs"] = c["n"]
    assert got == want and st["chain"] == nchain + nextra       # (with SINGLETONS the reads whose pairs have no direction are contigs of their own)
    assert (st["skipped"] > 0) == (skip == 2)
    names = ["r%d" % i for i in range(len(t["seqs"]))]
    ref_paf, ref_gfa = tmp_path / "py.paf", tmp_path / "py.gfa"
    formats.write_placements_paf(str(ref_paf), pl, names, t["lens"], np.diff(c["seq_off"]), c["kinds"])
    formats.write_gfa(str(ref_gfa), c["seqs"], c["kinds"], links, depth=pl["credited_bases"])
    assert paf.read_bytes() == ref_paf.read_bytes() and gfa.read_bytes() == ref_gfa.read_bytes()
    assert b"\tDP:f:" in gfa.read_bytes() and len(pu.parse_paf(str(paf))) == st["chain"] + st["anchored"]
    lines = [[int(x) for x in ln.split()] for ln in rec.read_text().split("\n") if ln]
    M = len(names)
    assert lines[:M] == [[int(r[k]) for k in ("start", "contig", "anchor", "score", "strand", "kind", "flags")] for r in pl["reads"]]
    at = M
    for k in range(c["n"]):
        a, b = int(pl["seg_off"][k]), int(pl["seg_off"][k + 1])
        assert lines[at] == [b - a, int(pl["credited_reads"][k]), int(pl["credited_bases"][k])]
        assert lines[at + 1:at + 1 + b - a] == [[int(s), int(d)] for s, d in zip(pl["seg_start"][a:b], pl["seg_depth"][a:b])]
        at += 1 + b - a
    assert at == len(lines)
    e.close()
