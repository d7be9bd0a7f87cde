"""-m gpu: contig polishing (polish.hip) at its kernels' own boundaries, on the cases of consensus_edge_cases.py: left runs across the
lane groups of the prefix-minimum scan, up runs across and over the 64-row blocks of the walk, both in one read inside batches that start
off a multiple of four, rings shorter than the band, slices clipped on both strands, non-voters among voters, the seams between
contigs, and slots and reads around one block of 256 lanes.  Every comparison is exact equality with the restatements of
consensus_util.py (test_gpu_consensus._check: sequences byte for byte, col, gap, per-read records, all stats, the plain call against the
votes call), and the device's batch count is the one the cases' batch_starts gives; test_consensus_edges_cpu.py holds the cases' claims
on the CPU."""
import pytest

import consensus_edge_cases as ec
import consensus_util as cs
import contig_util as cu
import elba_amd
from test_gpu_consensus import _check

pytestmark = pytest.mark.gpu


def _ids(cases):
    return [c["name"] for c in cases]


def _run(case):
    """The case on a fresh context: the device places the reads where the case says, polishes as the restatements do, holds the case's own
    claims, and gives the same under every setting of polish_trace_bytes the case names."""
    cin = case["cin"]
    seqs = cin["seqs"]
    e = elba_amd.Engine(17, 2, 8)
    e.set_reads(*cu.pack(seqs))
    e.set_overlaps(len(seqs), *case["pairs"])
    e.transitive_reduction(case["cutoff"], 0)
    e.generate_contigs(circular=bool(case["cflags"] & 1), singletons=bool(case["cflags"] & 2))
    got = e.export_contigs()
    assert got["seqs"] == cin["contigs"] and (e.export_read_flags(len(seqs)) == case["read_flags"]).all()
    pl, _ = e.place_reads(case["skip"])
    for f in ("start", "contig", "strand", "kind", "flags"):
        assert (pl["reads"][f] == cin["reads"][f]).all(), f
    args = (case["skip"], cin["band"], cin["max_diff_q16"] / 65536.0, cin["min_depth"])
    out, st, _ = _check(e, seqs, *args[1:], skip=case["skip"], loops=case["loops"], got=got)
    assert ec.check_claims(case, out, st) is None, ec.check_claims(case, out, st)
    assert st["batches"] == 1
    rows = [int(x) for x in out["reads"]["n"]]
    for nbytes in case["trace"]:
        e.set_option("polish_trace_bytes", nbytes)
        again, st2 = e.polish_contigs(*args, votes=True)
        assert cs.first_difference(out, again) is None, (nbytes, cs.first_difference(out, again))
        assert {k: st2[k] for k in cs.STATS} == {k: st[k] for k in cs.STATS} and st2["batches"] > 1
        assert st2["batches"] == len(ec.batch_starts(rows, cin["band"], nbytes))          # the device cut where the cases say it does
        if nbytes == 1:
            assert st2["batches"] == st["voted"] + st["rejected"]          # every voter alone, no batch for a read without rows
    e.set_option("polish_trace_bytes", 0)
    e.close()
    return out, st


@pytest.mark.parametrize("case", ec.left_run_cases(), ids=_ids(ec.left_run_cases()))
def test_left_runs_across_the_lane_groups_of_the_scan(case):
    _run(case)


@pytest.mark.parametrize("case", ec.up_run_cases(), ids=_ids(ec.up_run_cases()))
def test_up_runs_across_and_over_the_blocks_of_the_walk(case):
    _run(case)


@pytest.mark.parametrize("case", ec.both_run_cases(), ids=_ids(ec.both_run_cases()))
def test_both_runs_in_batches_that_start_off_a_multiple_of_four(case):
    """The first setting cuts the batches at reads 0, 1, 3, 4, 6, 7, 9, the second at 0, 1, 4, 7: the long reads 3, 6 and 9 stand first or third
    in a batch whose first read is 3, 6, 9, 1, 4 or 7."""
    out, st = _run(case)
    assert st["voted"] == 10


@pytest.mark.parametrize("case", ec.short_ring_cases(), ids=_ids(ec.short_ring_cases()))
def test_rings_shorter_than_the_band(case):
    _run(case)


@pytest.mark.parametrize("case", ec.clipped_cases(), ids=_ids(ec.clipped_cases()))
def test_clipped_slices_on_both_strands(case):
    _run(case)


@pytest.mark.parametrize("case", ec.non_voter_cases(), ids=_ids(ec.non_voter_cases()))
def test_outside_and_unplaced_reads_among_the_voters(case):
    out, st = _run(case)
    assert st["outside"] >= 2 and int((out["reads"]["status"] == cs.NOT_PLACED).sum()) == 3


@pytest.mark.parametrize("case", ec.seam_cases(), ids=_ids(ec.seam_cases()))
def test_seams_between_contigs(case):
    out, st = _run(case)
    assert len(out["seqs"]) == 6 and out["inserted"].tolist() == [1, 1, 0, 1, 0, 1] and out["deleted"].tolist() == [0, 0, 1, 0, 0, 0]
    assert [int(x) for x in out["seq_off"]] == case["seq_off"]


@pytest.mark.parametrize("case", ec.launch_edge_cases(), ids=_ids(ec.launch_edge_cases()))
def test_slots_and_reads_around_one_block_of_256_lanes(case):
    out, st = _run(case)
    assert st["low_depth_columns"] == len(ec.low_depth_slots(case, out))
