"""The C++ host mirror of the five string-graph cleaning calls (ClipTips, PopBubbles, CutWeakOverlaps, CutBridges, ResolveStars in
elba_amd/hostcpp/elba_host.hpp) against the Python binding, each on one workload: the same stats, the same cleaned S and removed reads
(checksums), the same contigs' counts, and the host's own comparison of the cleaned S with the S before the call."""
import collections
import os

import numpy as np
import pytest

import contig_util as cu
import elba_amd
import hostcpp_util as hu
import util

FA = os.path.join(util.GOLDEN, "small_err.fa")
MIN_RATIO = 0.9

# One row per call.  args: what follows `reads.fa K LOWER UPPER` on the program's command line.  The workload is
# synth_reads(seed, 60000, 12, 3000, 500, error_rate=err, min_len=400) at k = 17, 2 .. 12.  call: the binding's call on an engine that has
# S.  flag: the bit of export_read_flags the call gives the reads it removes (0: it removes none, and the program prints no read_checksum).
# keys: the stats the program prints.  changed(st, removed, flags_kept): what the call did to the graph of this workload.
Row = collections.namedtuple("Row", "name binary args seed err call flag keys changed")
ROWS = [
    # its string graph has a tip of 5 reads
    Row("tips", "test_host_tips", [10, 4], 44, 0.03, lambda e: e.clip_tips(10, 4), 4,
        ("nnz_before", "nnz_after", "dead_ends", "tips", "reads_removed", "entries_removed", "spared_anchors", "rounds_run"),
        lambda st, removed, flags_kept: st["reads_removed"] > 0 and st["tips"] > 0 and st["nnz_after"] < st["nnz_before"] and len(removed) == st["reads_removed"]),
    # its string graph has four bubbles of one-read arms
    Row("bubbles", "test_host_bubbles", [10, 4], 89, 0.03, lambda e: e.pop_bubbles(10, 4), 8,
        ("nnz_before", "nnz_after", "anchors", "arms", "bubbles", "arms_removed", "reads_removed", "entries_removed", "rounds_run"),
        lambda st, removed, flags_kept: st["reads_removed"] > 0 and st["bubbles"] > 0 and st["nnz_after"] < st["nnz_before"] and len(removed) == st["reads_removed"]),
    # its string graph has read ends with two overlaps of unlike scores; the graph changes, the flags do not
    Row("weak", "test_host_weak", [int(round(MIN_RATIO * 65536))], 89, 0.03, lambda e: e.cut_weak_overlaps(MIN_RATIO), 0,
        ("nnz_before", "nnz_after", "branch_sides", "weak_entries", "entries_removed", "sides_emptied"),
        lambda st, removed, flags_kept: st["entries_removed"] > 0 and st["weak_entries"] > 0 and st["nnz_after"] < st["nnz_before"] and flags_kept),
    # Cut at (2, 3).  Its string graph has 218 entries, 8 anchors, 8 chains and 8 long flanks, and no bridge: a scan on the device of seeds
    # 80 .. 99 x error rate {0.03, 0.08} x {no repeats, 4 repeat families of 400 bases on a tenth of the genome} at (1, 3) and (2, 3) found none
    # in any of the 160 graphs (they have some 240 reads each), and this is the one with the most chains and long flanks.  So the mirror is
    # held to the binding on a call that looks at chains and flanks and removes nothing; tests/test_gpu_bridges.py holds the removal.
    Row("bridges", "test_host_bridges", [2, 3], 89, 0.03, lambda e: e.cut_bridges(2, 3), 16,
        ("nnz_before", "nnz_after", "anchors", "chains", "long_flanks", "bridges", "reads_removed", "entries_removed"),
        lambda st, removed, flags_kept: len(removed) == st["reads_removed"] and st["anchors"] > 0 and st["chains"] > 0 and st["long_flanks"] > 0),
    # Up to 64 rounds: the R of a real reduction, transitive pairs and all.  Its string graph has 230 entries and 6 centres, 2 with one pair in
    # R and 4 with two; 2 reads go, in one round.  A scan on the device of seeds 80 .. 99 x error rate {0.03, 0.08} x {no repeats, 4 repeat
    # families of 400 bases on a tenth of the genome} found centres in 26 of the 80 graphs (none at 0.08, whose graphs are nearly empty), a
    # resolved one in 15, never more than 2, and no centre with e = 0 but one: in a layout of this coverage the neighbours of a read mostly
    # overlap each other.
    Row("stars", "test_host_stars", [64], 92, 0.03, lambda e: e.resolve_stars(64), 32,
        ("nnz_before", "nnz_after", "centres", "pairs0", "pairs1", "pairs2", "pairs3", "reads_removed", "entries_removed", "rounds_run"),
        lambda st, removed, flags_kept: len(removed) == st["reads_removed"] == 2 and st["pairs1"] == 2 and st["pairs2"] == 4 and st["centres"] == 6 and st["rounds_run"] == 2),
]
BY_ROW = dict(argvalues=ROWS, ids=[r.name for r in ROWS])


@pytest.mark.parametrize("row", **BY_ROW)
def test_cleaning_mirror_builds_and_fails_loudly_without_gpu(row):
    m = util.golden_meta()["small_err"][0]
    got = hu.runs_or_reports_no_device([hu.binary(row.binary), FA, m["k"], m["lower"], m["upper"]] + row.args)
    assert got is None or got["reads"] == 80


@pytest.mark.gpu
@pytest.mark.parametrize("row", **BY_ROW)
def test_cleaning_mirror_equals_the_python_binding(row, tmp_path):
    packed, off, lens, _ = elba_amd.synth_reads(row.seed, 60000, 12, 3000, 500, error_rate=row.err, min_len=400)
    fa = hu.write_fasta(tmp_path / "reads.fa", cu.seqs_of(packed, off, lens))
    got = hu.run_json(hu.binary(row.binary), [fa, 17, 2, 12] + row.args)
    e = hu.pipeline_engine(packed, off, lens, 17, 2, 12)
    f0 = e.export_read_flags(len(lens))
    st = row.call(e)
    g = e.export_string_graph()
    removed = np.flatnonzero(e.export_read_flags(len(lens)) & row.flag)
    cs = e.generate_contigs()
    want = {k: st[k] for k in row.keys}
    want.update(reads=len(lens), s_checksum=hu.s_checksum(g), host_equal=1, contigs=cs["contigs"], bases=cs["bases"], branches=cs["branches"])
    if row.flag:
        want.update(read_checksum=hu.read_checksum(removed))
    print("host mirror workload:", want)
    assert got == want
    assert row.changed(st, removed, (e.export_read_flags(len(lens)) == f0).all())
    e.close()
