"""-m gpu: the routes through the host driver of the overlap SpGEMM (csrc/spgemm.hip: plan, tier table, steps, sharded entry points), pinned.  Every case
of tests/overlap_routes.py — reads-built matrices on the reads-path instantiation and with each option that turns it off, sampled cold calls with
mirror slabs, the dense path, 32-byte records, escalation and the HBM tier, a repeated pass, wide rows, row pointers by the scan, empty and one-row
matrices, sharded calls with and without the mirror exchange — must give the digests of B and the statistics recorded in
tests/golden/overlap_routes.json (recorded on the commit before the driver was split), the oracle's B, and complete every non-empty row on some tier
(run_case checks both)."""
import json
import os

import pytest

import overlap_routes as routes
import util

pytestmark = pytest.mark.gpu

with open(os.path.join(util.GOLDEN, "overlap_routes.json")) as _f:
    GOLDEN = json.load(_f)


def _calls(g, name):
    return g[name] if name in routes.ENGINE_CASES else [c for rank in g[name] for c in rank]


def test_the_fixture_holds_every_case_and_the_routes_the_cases_are_for():
    assert sorted(GOLDEN) == sorted(routes.ALL_CASES)
    g = GOLDEN
    # the reads-path instantiation where the matrix allows it, the general kernel under every option that changes one of its switches
    assert [c["overlap_spec"] for c in g["reads15_whole"]] == [1, 1, 1] and [c["overlap_spec"] for c in g["reads_whole"]] == [0, 0, 0]
    for name, (matrix, opts, _, _, spec) in routes.ENGINE_CASES.items():
        if spec is not None:
            assert all(c["overlap_spec"] == spec for c in g[name]), name
    assert all(c["overlap_spec"] == 0 for name in routes.SHARDED_CASES for c in _calls(g, name))
    # a staging area too small — forced by the workspace hint, or a B far beyond nnz(A) — costs a cold call a second pass, the next call none
    repeated = {"repeated_pass": [2, 1], "wide_rows": [2, 1], "escalation_hbm": [2]}
    assert all([c["passes"] for c in _calls(g, name)] == repeated.get(name, [1] * len(_calls(g, name))) for name in routes.ALL_CASES)
    # slabs: the ratio carried over from the cold call, then forced
    slab = [c.get("overlap_slab_q16") for c in g["sampled_slabs"]]
    assert slab[0] is None and slab[2] == 1 and 1 < slab[1] < slab[3]      # (the margin and the capacity of the slab area shape the ratio the call reports)
    # every call of a case gives the same B; the options of one matrix too
    for name in routes.ALL_CASES:
        if name in routes.ENGINE_CASES:
            assert len({(c["b_rowptr"], c["b_col"], c["b_val"], c["nnz"]) for c in g[name]}) == 1, name
    for matrix in ("reads", "reads15", "dense"):
        assert len({g[n][0]["b_val"] for n, c in routes.ENGINE_CASES.items() if c[0] == matrix}) == 1, matrix
    assert g["empty_matrix"][0]["nnz"] == 0 and g["one_row"][0]["nnz"] == 1
    # the sharded cases: the ranks' rows add up to the same matrix whatever the exchange; the empty rank holds nothing
    for w in (2, 3):
        totals = {tuple(sum(rank[n]["nnz"] for rank in g["sharded_w%d_%s" % (w, x)]) for n in range(2)) for x in ("slots", "tiny", "counted", "no_exchange")}
        assert len(totals) == 1, w
    assert all(c["nnz"] == 0 and c["products"] == 0 for c in g["sharded_empty_rank"][1])


@pytest.mark.parametrize("name", routes.ALL_CASES)
def test_digests_and_statistics_equal_the_recorded_ones(name):
    got = routes.run_case(name)
    print(name, got)
    assert got == GOLDEN[name]
