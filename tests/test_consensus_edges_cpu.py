"""CPU: the cases of consensus_edge_cases.py against the two restatements of contig polishing (consensus_util.py) before any of them
reaches the device: the restatements agree on the case, the case's claims hold, its walks have the runs, band cells, rows and seams the
case was built for, and the placements it writes down are those placement_util.place_tables derives from its graph.  Cases marked
loops = False run through polish_tables alone: their reads have 700 to 1 750 rows of 128 or 256 cells, which polish_loops, a dict entry
per cell, does not do in a second (nor the cases of 255 to 257 reads); band 64 has every construction at a size polish_loops does."""
import pytest

import consensus_edge_cases as ec
import consensus_util as cs
import placement_util as pu

CASES = ec.all_cases()
IDS = [c["name"] for c in CASES]


@pytest.fixture(scope="module")
def results():
    memo = {}

    def get(case):
        if case["name"] not in memo:
            walks = {}
            memo[case["name"]] = cs.polish_tables(case["cin"], walks) + (walks,)
        return memo[case["name"]]
    return get


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_claims_and_structure_hold(case, results):
    out, st, walks = results(case)
    assert ec.check_claims(case, out, st) is None, ec.check_claims(case, out, st)
    assert ec.check_structure(case, walks, out) is None, ec.check_structure(case, walks, out)
    assert st["voted"] + st["rejected"] + st["outside"] + int((out["reads"]["status"] == cs.NOT_PLACED).sum()) == len(case["cin"]["seqs"])


@pytest.mark.parametrize("case", [c for c in CASES if c["loops"]], ids=[c["name"] for c in CASES if c["loops"]])
def test_the_two_restatements_agree(case, results):
    a, sa, _ = results(case)
    b, sb = cs.polish_loops(case["cin"])
    assert cs.first_difference(a, b) is None and sa == sb, (cs.first_difference(a, b), sa, sb)


def test_every_band_has_its_large_cases_and_band_64_has_them_under_both_restatements():
    for build in (ec.left_run_cases, ec.up_run_cases, ec.both_run_cases):
        bands = {c["cin"]["band"]: c["loops"] for c in build()}
        assert bands[64] and 256 in bands, build.__name__


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_cases_are_the_ones_the_placement_rule_gives(case):
    inp = pu.inputs_of_chains([len(s) for s in case["cin"]["seqs"]], case["chains"], case["kinds"], *case["pairs"], case["read_flags"], case["skip"])
    pl, _ = pu.place_tables(inp)
    got, want = pl["reads"], case["cin"]["reads"]
    for f in ("start", "contig", "strand", "kind", "flags"):
        assert (got[f] == want[f]).all(), (case["name"], f, got[f], want[f])


@pytest.mark.parametrize("case", ec.left_run_cases(), ids=[c["name"] for c in ec.left_run_cases()])
def test_left_runs_cross_the_lane_groups_they_are_named_for(case, results):
    """Band cell b lies in lane b / C: cells 16 C, 32 C and 48 C are the first of lanes 16, 32 and 48, where the prefix minimum passes from
    one row of 16 lanes to the next (row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and 3)."""
    _, _, walks = results(case)
    Cc = case["cin"]["band"] // 64
    for r in (1, 2):
        (run,) = cs.runs_of(walks[r], 2)
        crossed = ec.lane_groups_crossed(run[4], run[5], Cc)
        if "all-lane-groups" in case["name"]:
            assert run[4] < 16 * Cc and run[5] >= 48 * Cc and crossed == [16, 32, 48]
        elif "only-" in case["name"]:
            assert crossed == [int(case["name"].rsplit("-", 1)[1]) // Cc]
        else:
            assert run[5] == case["cin"]["band"] - 1


@pytest.mark.parametrize("case", ec.up_run_cases()[:3], ids=[c["name"] for c in ec.up_run_cases()[:3]])
def test_up_runs_sit_on_every_seam_and_cast_one_vote(case, results):
    out, _, walks = results(case)
    seams = set()
    for r in range(1, 7):
        (run,) = cs.runs_of(walks[r], 1)
        n = walks[r][0][1]
        seams |= {(which, d) for which in (0, 1) for d in (-1, 0, 1) if (n + d - run[which]) % 64 == 0}
    assert seams >= {(w, d) for w in (0, 1) for d in (-1, 0, 1)}
    assert int(out["gap"].sum()) == 6 and int(out["inserted"][0]) == 1                  # one vote per read, all for the same gap
    if case["cin"]["band"] > 64:
        assert sum(1 for c in case["structure"] if c[0] == "block") >= {128: 5, 256: 6}[case["cin"]["band"]]


def test_no_up_run_is_longer_than_the_band_allows():
    """An up step moves one band cell down, so from cell W - 3 a run has W - 3 rows at the most: a region of W - 2 bases does not come out
    as one run (which is why band 128 has a run of 124 rows and not of 130 or more)."""
    case = ec.over_long_up_run_part(128)
    walks = {}
    out, _ = cs.polish_tables(case["cin"], walks)
    ups = cs.runs_of(walks[1], 1) if 1 in walks else []
    assert int(out["reads"][1]["status"]) in (cs.VOTED, cs.REJECTED) and all(u[1] - u[0] + 1 <= 125 for u in ups)
    assert int(out["reads"][1]["dist"]) > 126 or len(ups) > 1


def test_batches_start_off_a_multiple_of_four(results):
    for case in ec.both_run_cases():
        out, _, _ = results(case)
        rows, W = [int(x) for x in out["reads"]["n"]], case["cin"]["band"]
        assert [ec.batch_starts(rows, W, b) for b in case["trace"]] == [[0, 1, 3, 4, 6, 7, 9], [0, 1, 4, 7]]


def test_short_rings_see_every_column_more_than_once(results):
    for case in ec.short_ring_cases():
        cin = case["cin"]
        out, _, _ = results(case)
        depth, votes = out["col"].sum(axis=1), int(out["gap"][0].sum())
        assert int(depth[0]) >= 2 * votes > int(depth[-1])            # gap 0 emits through column L - 1 only
        L, W = len(cin["contigs"][0]), cin["band"]
        assert L < W and cin["kinds"] == [ec.C] and {int(s) for s in cin["reads"]["strand"]} == {0, 1}
        assert int(cin["reads"]["start"].min()) < 0 and max(len(s) for s in cin["seqs"]) > L
    out, _ = cs.polish_tables(ec.short_ring_case(40, 256)["cin"])
    assert int(out["reads"]["end_j"].min()) <= -118                   # far below column 0: pos % L on negative positions


def test_clipped_slices_start_inside_the_read_on_both_strands():
    for case in ec.clipped_cases():
        rec = case["cin"]["reads"]
        assert {(int(r["strand"]), int(r["start"]) < 0) for r in rec} >= {(0, True), (1, True), (0, False), (1, False)}
        assert all(len(s) % 4 for s, r in zip(case["cin"]["seqs"], rec) if int(r["kind"]) == pu.ANCHORED and len(s) != 114) and len({len(s) % 4 for s in case["cin"]["seqs"]}) >= 3


def test_non_voters_stand_between_voters(results):
    (case,) = ec.non_voter_cases()
    out, st, _ = results(case)
    status = out["reads"]["status"].tolist()
    assert st["outside"] >= 2 and status.count(cs.NOT_PLACED) == 3 and case["read_flags"].tolist().count(1) == 2
    for r, s in enumerate(status):
        if s in (cs.NOT_PLACED, cs.OUTSIDE):
            assert cs.VOTED in status[:r] and cs.VOTED in status[r + 1:]
    rows = [int(x) for x in out["reads"]["n"]]
    assert len(ec.batch_starts(rows, 64, 1)) == st["voted"] and 1 < len(ec.batch_starts(rows, 64, case["trace"][0])) < st["voted"]


def test_launch_edges_lie_on_both_sides_of_lane_255(results):
    for case in ec.launch_edge_cases():
        out, st, _ = results(case)
        if case["name"].startswith("slots-"):
            X = int(case["name"].split("-")[1])
            low = ec.low_depth_slots(case, out)
            assert int(out["col_off"][-1]) + len(case["cin"]["contigs"]) == X and len(low) == st["low_depth_columns"] and max(low) == X - 2
            assert {x // 64 for x in low} >= set(range((X - 2) // 64 + 1))            # a low-depth column in every wavefront of the call
            if X == 320:
                assert {254, 255, 256, 257} <= set(low)
        else:
            M = int(case["name"].split("-")[1])
            status = out["reads"]["status"].tolist()
            assert len(status) == M and status[-3:] == [cs.OUTSIDE] * 3 and status.count(cs.VOTED) == M - 3
    assert [c["name"] for c in ec.launch_edge_cases()] == ["slots-255", "slots-256", "slots-257", "slots-320", "reads-255", "reads-256", "reads-257"]


def test_the_seams_case_has_every_kind_of_neighbour(results):
    (case,) = ec.seam_cases()
    out, _, _ = results(case)
    assert case["kinds"] == [ec.P, ec.C, ec.C, ec.S, ec.S, ec.S] and case["seq_off"] is not None
    assert out["inserted"].tolist() == [1, 1, 0, 1, 0, 1] and out["deleted"].tolist() == [0, 0, 1, 0, 0, 0] and out["voters"].tolist()[4] == 1
    off = [int(x) for x in out["col_off"]]
    assert int(out["gap"][off[0] + 0 + 97].sum()) == 2 and int(out["gap"][off[1] + 1].sum()) == 4            # gap L of the path, gap 0 of the ring behind it
    assert int(out["col"][off[3] - 1][4]) == 3 and int(out["gap"][off[3] + 3].sum()) == 2                   # the deleted last column, gap 0 of the contig behind it
