"""-m gpu: the late stages past their second size boundary, on the inputs of trip_cases.py sized from the device's own CU count.

  k_pl_candidates   more pairs than its capped grid has lanes (16 x CUs x 256): lanes with one, two and three trips, winners decided
                    across trips, the smallest bad pair on either side of the first trip
  k_gl_sum          64, 65, 256, 257 and 600 partials, the content in the partials of chosen workgroups only: every wavefront of the
                    sum, and its second and third trip over the partials
  text_index.hip    more records than the line and record kernels' capped grid has lanes (8 x CUs x 256), headers in the second trip
                    of the line kernels, a violation in the second trip alone and behind one in the first

All through the checks of the stages' own files: place_tables on the device's own contigs and flags, both link restatements on the
device's own S and contigs, index_numpy and the oracle's encoder."""
import time

import numpy as np
import pytest
import torch

import elba_amd
import placement_util as pu
import text_index_util as tx
import trip_cases as tc
from test_gpu_assembly_graph import _check as _check_links, _engine as _links_engine, _gen
from test_gpu_placement import INVALID_ARG, _check as _check_placement, _load, _packed

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cus():
    n = torch.cuda.get_device_properties(0).multi_processor_count
    assert n > 0
    return n


# ---- placement -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,ring", [(0, False), (1, False), (2, False), (2, True)], ids=["full-trip", "one-lane-twice", "three-trips", "three-trips-ring"])
def test_placement_past_one_trip_of_the_candidate_grid(cus, which, ring):
    """T = 16 x CUs x 256 pairs fill the grid once.  T pairs: a full single trip, the last lane included.  T + 1: lane 0 takes the last
    pair, the only one of read M - 1, in a second trip.  2 T + 77: every lane twice, 77 of them three times; reads whose best pair lies
    in the first, the second or the third trip, a tie across the trips, a read that is T of a pair in one trip and Q in another.  The
    candidate count is the constructed one: a lane that drops a trip loses its count too."""
    T = tc.placement_trip(cus)
    case = tc.placement_pairs(cus, (0, 1, T + 77)[which], ring=ring)
    assert case["T"] == T and case["n"] == T + (0, 1, T + 77)[which]
    lens, pairs = case["lens"], case["pairs"]
    t0 = time.perf_counter()
    e = elba_amd.Engine(17, 2, 8)
    got = _load(e, _packed(np.random.default_rng(which), lens), pairs, case["cflags"])
    chains = [[(int(got["chain_read"][i]), int(got["chain_prefix"][i]), int(got["chain_strand"][i])) for i in range(int(a), int(b))]
              for a, b in zip(got["chain_off"][:-1], got["chain_off"][1:])]
    assert chains == case["chains"] and (np.flatnonzero(e.export_read_flags(len(lens)) == pu.CONTAINED) == case["off"]).all()
    t1 = time.perf_counter()
    pl, st, _ = _check_placement(e, pairs, lens, loops=False, got=got)
    t2 = time.perf_counter()
    print("placement %d pairs: load %.2f s, place + restatement %.2f s, the call itself %.3f ms" % (case["n"], t1 - t0, t2 - t1, st["ms_total"]))
    assert st["candidates"] == case["candidates"] and st["chain"] == case["nchain"] and st["anchored"] == len(case["off"]) and st["unanchored"] == 0
    assert set(case["anchors"]) == ({"last"} if which < 2 else set(tc.ROLES))
    for role, (r, y) in case["anchors"].items():
        p = pl["reads"][r]
        a = case["index"][role]
        assert (int(p["kind"]), int(p["anchor"]), int(p["score"])) == (pu.ANCHORED, y, int(pairs[2]["score"][a])), (role, p, a)
    again, st2 = e.place_reads()                                 # the same context once more: nothing of the first call's trips is left
    assert pu.same_placements(again, pl) and again["reads"].tobytes() == pl["reads"].tobytes()
    assert {k: st2[k] for k in pu.STATS} == {k: st[k] for k in pu.STATS}
    e.close()


@pytest.mark.parametrize("first", [False, True], ids=["second-trip-only", "both-trips"])
def test_the_smallest_bad_pair_across_the_trips(cus, first):
    """A bad candidate at index T + 5 alone — seen only by lane 5 in its second trip — is named; with another at index 9 that one is.
    Nothing of the failed call is left in the counts."""
    T = tc.placement_trip(cus)
    case = tc.placement_pairs(cus, 77, bad=(9, T + 5) if first else (T + 5,))
    a = case["bad"]
    assert a == (9 if first else T + 5)
    lens, (rows, cols, vals) = case["lens"], case["pairs"]
    e = elba_amd.Engine(17, 2, 8)
    got = _load(e, _packed(np.random.default_rng(5), lens), case["pairs"], 0)
    with pytest.raises(elba_amd.ElbaError) as err:
        e.place_reads()
    assert err.value.status == INVALID_ARG and "pair %d (%d, %d)" % (a, rows[a], cols[a]) in str(err.value), str(err.value)
    for k in pu.GET_STATS:
        assert e.get_stat("place_" + k) == 0
    with pytest.raises(pu.BadInterval) as want:
        pu.place_tables(pu.inputs_of_export(rows, cols, vals, got, e.export_read_flags(len(lens)), lens))
    assert want.value.pair == a
    e.close()


# ---- links -----------------------------------------------------------------------------------------------------------------------------------
LINKS = tc.links_cases()


@pytest.mark.parametrize("nb,hot", LINKS, ids=["%d-%s" % (nb, "+".join(map(str, hot))) for nb, hot in LINKS])
def test_link_counters_from_chosen_workgroups_of_the_count_pass(nb, hot):
    """nb count-pass workgroups, structures of every counter kind in the columns of the workgroups `hot` alone: partial b is added up by
    lane b mod 256 of k_gl_sum, in wavefront (b mod 256) / 64, in trip b / 256.  Under contig flags 3 links, closures, twisted, clamped
    and asymmetric are nonzero; under 1 (no single-read contigs: no branch read has one) every candidate is unplaced."""
    g = tc.links_graph(nb, hot)
    lens = g["lens"]
    e, s = _links_engine(*_packed(np.random.default_rng(nb), lens), *g["pairs"])
    assert (len(lens) + 1 + 255) // 256 == nb
    for flags in (3, 1):
        _gen(e, flags)
        recs, st, _ = _check_links(e, s, lens)
        assert {k: st[k] for k in tc.LINK_COUNTERS} == g["expected"][flags], (flags, st, g["expected"][flags])
        per = np.bincount(recs["from_read"] // 256, minlength=nb)
        assert per.sum() == len(recs) == st["links"] + st["closures"] and sorted(np.flatnonzero(per).tolist()) == sorted(hot)
    e.close()


# ---- text ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    e = elba_amd.Engine(17, 2, 8)
    yield e
    e.close()


TEXTS = {"fasta": lambda c: tc.fasta_text(c), "fasta-no-final-newline": lambda c: tc.fasta_text(c, final_newline=False),
         "fasta-multi": lambda c: tc.fasta_text(c, multi=True), "fasta-multi-no-final-newline": lambda c: tc.fasta_text(c, multi=True, final_newline=False),
         "fastq": lambda c: tc.fastq_text(c), "fastq-no-final-newline": lambda c: tc.fastq_text(c, final_newline=False)}


@pytest.mark.parametrize("name", sorted(TEXTS))
def test_more_records_than_the_record_kernels_have_lanes(eng, cus, name):
    """8 x CUs x 256 + 3 records: k_fa_records / k_fq_records (over records + 1) and k_text_names take a second trip, k_fa_flags,
    k_fa_scatter and k_fa_shape (over lines) too — with 2 - 3 sequence lines per record most headers lie in their second and later
    trips.  Empty reads and a missing final newline included; field for field as in test_gpu_text_ingest.py."""
    t = TEXTS[name](cus)
    st, _ = tx.device_check(eng, t["data"])
    assert st["nreads"] == t["R"] == tc.text_trip(cus) + 3 and st["lines"] > (3 if "multi" in name else 1) * tc.text_trip(cus) and st["format"] == tx.FMT[t["fmt"]]


@pytest.mark.parametrize("fmt", ["fasta", "fastq"])
def test_a_violation_in_the_second_trip_and_one_behind_another(eng, cus, fmt):
    """One violation in the last record alone is found (by a lane in its second trip); with one in record 7 and one in record R - 2 the
    earlier one is named.  The old reads stay."""
    good = tx.fasta_bytes(tx.random_seqs(np.random.default_rng(1), [70, 0, 5, 130]), 60)
    st, _ = tx.device_check(eng, good, file_off=77)
    before = tx.device_exported(eng, st["nreads"], st["packed_bytes"])
    R = tc.text_trip(cus) + 3
    build = (lambda broken: tc.fasta_text(cus, multi=True, broken=broken)) if fmt == "fasta" else (lambda broken: tc.fastq_text(cus, broken=broken))
    for broken, rec in (((R - 1,), R - 1), ((7, R - 2), 7)):
        t = build(broken)
        kind, off, r = t["error"]
        assert r == rec
        got, named = tx.device_rejected(eng, t["data"], loop=False)
        assert got == (kind, off) and named == rec
        assert tx.same_export(tx.device_exported(eng, st["nreads"], st["packed_bytes"]), before)
    assert eng.export_read_index()[0] == ["read0", "read1", "read2", "read3"]
