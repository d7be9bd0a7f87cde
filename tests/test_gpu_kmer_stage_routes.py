"""-m gpu: the routes through the k-mer stage's host driver (csrc/kmer_msd.hip, msd_run), pinned.  The oracle-equality tests also pass when the driver
quietly finds "no plan" and the sort path does the work; here every case — one pass and value-range passes at k = 17 and k = 31, crowded buckets and
pseudo-buckets, the re-emit without gather slots, "measure_prep", device triples, two routes on one engine (tests/kmer_stage_routes.py) — must take the
route recorded in tests/golden/kmer_stage_routes.json (the diagnostic counters), give the recorded counts and the recorded digests of the columns, the
reliable k-mers and their counts, and, where the oracle counts the case's reads, the oracle's A."""
import json
import os

import pytest

import gpu_util as gu
import kmer_stage_routes as routes
import util

pytestmark = pytest.mark.gpu

with open(os.path.join(util.GOLDEN, "kmer_stage_routes.json")) as _f:
    GOLDEN = json.load(_f)

_oracles = {}


def _oracle(reads, k, lo, up):
    key = (reads, k, lo, up)
    if key not in _oracles:
        _oracles[key] = gu.oracle_run(*routes.read_set(reads), k, lo, up, threads=8)
    return _oracles[key]


def _equals_oracle(e, ks, reads, k, lo, up):
    o = _oracle(reads, k, lo, up)
    assert tuple(ks[f] for f in routes.COUNTS) == (o.stat("I"), o.stat("ndistinct"), o.stat("N"), o.stat("Z"))
    gu.assert_A_equal(e.export_kmer_matrix(), o.A())


def test_the_fixture_holds_every_case_and_the_shapes_the_cases_are_for():
    assert sorted(GOLDEN) == sorted(routes.ALL_CASES)
    g = GOLDEN
    assert all(g[c]["kmer_path"] == 1 and g[c]["kmer_passes"] == 1 for c in ("k17_plain", "k17_no_rank", "k17_rank", "k17_small_cap", "slot_cap_one_pass", "measure_prep"))
    assert g["k17_small_cap"]["kmer_crowded_buckets"] >= 1                                   # k_msd_bucket runs
    assert all(g[c]["kmer_path"] == 1 and g[c]["kmer_passes"] >= 3 for c in ("k17_batched", "k17_batched_dominant_digit", "slot_cap_batched"))
    assert g["k17_batched_dominant_digit"]["kmer_largest_pass"] > g["k17_batched_dominant_digit"]["instances"] // 2
    assert g["k31_plain"]["kmer_path"] == 2 and g["k31_plain"]["kmer_passes"] == 1 and g["k31_plain"]["kmer_crowded_buckets"] == 0
    assert g["k31_crowded"]["kmer_passes"] == 1 and g["k31_crowded"]["kmer_crowded_buckets"] >= 1
    for c in ("k31_batched_crowded", "k31_batched_crowded_small_parent"):
        assert g[c]["kmer_path"] == 2 and g[c]["kmer_passes"] >= 3 and g[c]["kmer_crowded_buckets"] >= 1 and g[c]["kmer_crowded_small"] >= 1
    assert g["measure_prep"]["prep_measured"] == 1
    assert g["triples"]["triples_path"] == 1 and g["triples_empty_column"]["triples_path"] == 0
    first, second = g[routes.ENGINE_CASE]
    assert first["kmer_passes"] >= 2 and second["kmer_passes"] >= 4 and second["kmer_largest_pass"] > first["kmer_largest_pass"]


@pytest.mark.parametrize("name", routes.ALL_CASES)
def test_route_counts_and_digests_equal_the_recorded_ones(name):
    got = routes.run_case(name, check=_equals_oracle)
    print(name, got)
    assert got == GOLDEN[name]
