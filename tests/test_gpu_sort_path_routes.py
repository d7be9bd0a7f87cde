"""-m gpu: the routes through the host driver of the k-mer stage's SORT path (csrc/kmer.hip), pinned.  The oracle-equality tests also pass when the
path quietly takes another branch — pairs instead of packed words, per-head instead of fused, one pass instead of three; here every case
(tests/sort_path_routes.py: one-word packed and pairs, dropped index bits, two and three words in one pass and in value-range passes, dominant
prefixes, nothing kept, no instance, two counts on one engine, a second matrix build after one count, the owner side of exchange #1) must take the
route recorded in tests/golden/sort_path_routes.json (the diagnostic counters), give the recorded counts and the recorded digests of the column
pointers, the columns, the reliable k-mers and their counts, and, where the oracle counts the case's reads, the oracle's A."""
import json
import os

import pytest

import gpu_util as gu
import sort_path_routes as routes
import util
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

with open(os.path.join(util.GOLDEN, "sort_path_routes.json")) as _f:
    GOLDEN = json.load(_f)

_oracles = {}


def _oracle(reads, k, lo, up):
    key = (reads, k, lo, up)
    if key not in _oracles:
        o = po.Oracle(k, lo, up)
        o.count_and_build(*routes.read_set(reads))
        _oracles[key] = (o, o.A())
    return _oracles[key]


def _equals_oracle(ks, A, reads, k, lo, up):
    o, oA = _oracle(reads, k, lo, up)
    if ks is not None:
        assert tuple(ks[f] for f in routes.COUNTS) == (o.stat("I"), o.stat("ndistinct"), o.stat("N"), o.stat("Z"))
    gu.assert_A_equal(A, oA)


def _records(name, counts_only=False):
    g = GOLDEN[name]
    return [r for r in (g if isinstance(g, list) else [g]) if "kmer_path" in r or not counts_only]      # (a second matrix build records no count)


def test_the_fixture_holds_every_case_and_the_shapes_the_cases_are_for():
    assert sorted(GOLDEN) == sorted(routes.ALL_CASES)
    g = GOLDEN
    counted = [c for c in routes.ALL_CASES if c not in routes.DIST_CASES]
    assert all(r["kmer_path"] == 0 for c in counted for r in _records(c, True)) and all(_records(c, True) for c in counted)
    assert not any(f in r for c in routes.ALL_CASES for r in _records(c) for f in routes.LEFT_OUT)
    for c in counted:
        if c in routes.PASSES_FORCED:
            assert g[c]["kmer_passes"] >= 3 and g[c]["kmer_largest_pass"] < g[c]["instances"], c
        elif c != routes.ENGINE_CASE:
            assert all(r["kmer_passes"] == 1 and r["kmer_largest_pass"] == r["instances"] for r in _records(c, True)), c
    # the fused column pass hands its sort keys to the CSR build; the per-head emit, by option or by UPPER, and pairs do not change the matrix
    for c in ("k17_emit_plain", "k17_unfused", "k17_pairs"):
        assert {f: v for f, v in g[c].items()} == g["k17_packed_fused"], c
    assert g["k17_upper80"]["reliable"] > g["k17_packed_fused"]["reliable"]
    assert g["k17_drop1"] == g["k17_drop3"] and g["k17_drop1"]["reliable"] > 0
    assert [g[c]["kmer_words"] for c in ("k31_pairs_by_width", "k33", "k63", "k65", "k95")] == [1, 2, 2, 3, 3]
    assert all(g[c]["reliable"] > 0 for c in ("k31_pairs_by_width", "k33", "k63", "k65", "k95"))
    for one, many in (("k33", "k33_passes"), ("k65", "k65_passes"), ("k33_nothing_kept", "k33_passes_nothing_kept")):
        assert {f: v for f, v in g[many].items() if f not in ("kmer_passes", "kmer_largest_pass")} == {f: v for f, v in g[one].items() if f not in ("kmer_passes", "kmer_largest_pass")}
    # a unit above the cap is a pass of its own; a heavy bin cut by its 24-bit prefixes keeps every pass under the cap
    assert g["k63_unit_above_cap"]["kmer_largest_pass"] > g["k63_unit_above_cap"]["instances"] // 2      # (the cap is a sixth)
    assert g["k95_heavy_bin_refined"]["kmer_passes"] >= 200 and g["k95_heavy_bin_refined"]["kmer_largest_pass"] <= g["k95_heavy_bin_refined"]["instances"] // 200 + 1
    for c in ("k17_nothing_kept", "k33_nothing_kept", "k33_passes_nothing_kept"):
        assert g[c]["instances"] > 0 and g[c]["distinct"] > 0 and g[c]["reliable"] == 0 and g[c]["entries"] == 0
    assert all(g[routes.ZERO_CASE][f] == 0 for f in routes.COUNTS) and g[routes.ZERO_CASE]["kmer_passes"] == 1
    first, second = g[routes.ENGINE_CASE]
    assert first["kmer_passes"] >= 2 and second["kmer_passes"] >= 4 and second["kmer_largest_pass"] > first["kmer_largest_pass"]
    assert {f: v for f, v in second.items() if f not in ("kmer_passes", "kmer_largest_pass")} == {f: v for f, v in g["k33"].items() if f not in ("kmer_passes", "kmer_largest_pass")}
    once, again = g[routes.TWICE_CASE]
    assert once == g["k17_packed_fused"] and all(again[f] == once[f] for f in again)
    assert [g[c]["reliable"] > 0 for c in routes.DIST_CASES] == [True, True, True]


@pytest.mark.parametrize("name", routes.ALL_CASES)
def test_route_counts_and_digests_equal_the_recorded_ones(name):
    got = routes.run_case(name, check=_equals_oracle)
    print(name, got)
    assert got == GOLDEN[name]
