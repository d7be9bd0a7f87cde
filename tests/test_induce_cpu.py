"""CPU tests of the induced sub-problem's restatement (tests/induce_util.py): the two forms against each other and against the hand cases,
the order of the kept pairs, the builder's planted conditions — a partition of the overlaps graph splits no passed pair, failed pairs do
leave parts, and one read's bad flag depends on them —, the oracle's string graph of a part against the whole's, and the boundary."""
import ctypes

import numpy as np
import pytest

import comp_util as ku
import elba_amd
import induce_util as iu
from elba_amd import capi
from oracle import pyoracle as po

BLOCKS = (("layout", 60), ("random", 25), ("layout", 40), ("random", 12), ("layout", 9))


@pytest.fixture(scope="module")
def built():
    return [iu.build_input(seed, BLOCKS, n_failed=nf, lone=3) for seed, nf in ((1, 0), (2, 30), (3, 200))]


def _parts(g, nparts, min_reads=1):
    t = ku.tables(g["M"], *ku.edges_of_overlaps(g["rows"], g["cols"], g["vals"]))
    return ku.partition_of_reads(t, nparts, "reads", min_reads)[0], t


@pytest.mark.parametrize("case", iu.hand_cases(), ids=lambda c: c[0])
def test_hand_cases_hold_in_both_forms(case):
    M, rows, cols, vals, part_of_read, part = iu.case_input(case)
    for form in (iu.induce_loop, iu.induce_numpy):
        iu.check_case(case, form(M, rows, cols, vals, part_of_read, part))


def test_the_two_forms_agree_under_shuffled_selections(built):
    rng = np.random.default_rng(5)
    for g in built:
        for nparts in (1, 2, 5, g["M"]):
            part_of_read = rng.integers(-1, nparts, g["M"]).astype(np.int32)
            for part in sorted(set([-1, 0, nparts - 1, nparts])):
                a = iu.induce_loop(g["M"], g["rows"], g["cols"], g["vals"], part_of_read, part, g["reads"])
                b = iu.induce_numpy(g["M"], g["rows"], g["cols"], g["vals"], part_of_read, part, g["reads"])
                assert iu.same_induced(a, b) is None and (a["split_pairs"], a["split_passed"]) == (b["split_pairs"], b["split_passed"])
                assert a["pairs"] == 0 or iu.strictly_ascending(a["rows"], a["cols"])          # the numbering is monotone
                assert (np.diff(a["old_of_new"]) > 0).all() and a["split_pairs"] == int(a["outside_aligned"].sum())
                assert a["packed"][a["packed_bytes"]:].tolist() == [0] * 16


def test_reads_of_odd_lengths_keep_their_bases_and_lose_their_low_bits():
    import contig_util as cu
    rng = np.random.default_rng(6)
    packed, off, lens = cu.random_packed(rng, 40, 0, 35)           # (random low bits in every last byte)
    part_of_read = (np.arange(40) % 2).astype(np.int32)
    none = np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=po.OVERLAP_DTYPE)
    for part in (0, 1):
        a = iu.induce_loop(40, *none, part_of_read, part, (packed, off, lens))
        b = iu.induce_numpy(40, *none, part_of_read, part, (packed, off, lens))
        assert iu.same_induced(a, b) is None
        assert cu.seqs_of(a["packed"], a["byte_off"], a["len"]) == [s for v, s in enumerate(cu.seqs_of(packed, off, lens)) if v % 2 == part]
        assert cu.pack(cu.seqs_of(a["packed"], a["byte_off"], a["len"]))[0].tobytes() == a["packed"].tobytes()      # low bits zero, guard bytes zero


def test_a_partition_of_the_overlaps_graph_splits_no_passed_pair_but_failed_ones(built):
    split = []
    for g in built:
        for nparts in (1, 2, 3, 7):
            for min_reads in (1, 2, 5):
                part_of_read, t = _parts(g, nparts, min_reads)
                total = 0
                for part in range(-1, nparts):
                    a = iu.induce_numpy(g["M"], g["rows"], g["cols"], g["vals"], part_of_read, part)
                    assert a["split_passed"] == 0 and int(a["outside_passed"].sum()) == 0
                    total += a["split_pairs"]
                split.append(total)
    assert max(split) > 0                                           # at least one built input has pairs that leave their part


def test_the_planted_read_is_bad_only_with_the_outside_counts(built):
    """The condition the feature exists for, planted and asserted: with the outside counts the part's bad reads are the whole run's,
    without them the planted read comes out good."""
    differs = 0
    for g in built:
        M, x = g["M"], g["planted"]
        whole = iu.bad_reads(M, g["rows"], g["cols"], g["vals"])
        assert whole[x]
        n = len(_parts(g, 1)[1]["reads"])                           # as many parts as components: every component alone, every planted pair leaves
        part_of_read, _ = _parts(g, n)
        for part in range(n):
            a = iu.induce_numpy(M, g["rows"], g["cols"], g["vals"], part_of_read, part)
            with_counts = iu.bad_reads(a["reads"], a["rows"], a["cols"], a["vals"], a["outside_aligned"], a["outside_passed"])
            without = iu.bad_reads(a["reads"], a["rows"], a["cols"], a["vals"])
            assert (with_counts == whole[a["old_of_new"]]).all()
            if part_of_read[x] == part:
                w = int(np.searchsorted(a["old_of_new"], x))
                assert a["outside_aligned"][w] == 3 and with_counts[w] and not without[w]
                differs += 1
    assert differs == len(built)


def test_the_oracles_string_graph_of_a_part_is_the_wholes_restricted(built):
    g = built[1]
    M = g["M"]
    comp = ku.tables(M, *ku.edges_of_overlaps(g["rows"], g["cols"], g["vals"]))["comp_of_read"]
    keep = (g["vals"]["passed"] != 0) | (comp[g["rows"]] == comp[g["cols"]])      # without the failed pairs between components: no pair straddles
    assert 0 < keep.sum() < len(keep)
    rows, cols, vals = g["rows"][keep], g["cols"][keep], g["vals"][keep]
    S, flags, st = po.string_graph(M, rows, cols, vals, cutoff=0.65, fuzz=0)
    t = ku.tables(M, *ku.edges_of_overlaps(rows, cols, vals))
    part_of_read = ku.partition_of_reads(t, 3, "reads", 1)[0]
    seen = 0
    for part in range(3):
        a = iu.induce_numpy(M, rows, cols, vals, part_of_read, part)
        assert a["split_pairs"] == 0
        P, pflags, pst = po.string_graph(a["reads"], a["rows"], a["cols"], a["vals"], cutoff=0.65, fuzz=0)
        sel = np.zeros(M, dtype=bool); sel[a["old_of_new"]] = True
        new_of_old = np.cumsum(sel) - 1
        assert (pflags == flags[a["old_of_new"]]).all()
        assert iu._same_s(P, S, a["old_of_new"], new_of_old, sel) is None
        seen += P["n"]
    assert seen == S["n"] > 0


def test_the_library_exports_the_entry_points_and_the_abi_version_stays():
    L = elba_amd.load_library()
    for name in ("elba_induce_part", "elba_free_induced", "elba_set_overlaps_device", "elba_set_outside_counts", "elba_set_outside_counts_device"):
        assert hasattr(L, name) and name in capi.EXPORTED_SYMBOLS, name
    for name in ("induce_part", "load_part", "set_overlaps_device", "set_outside_counts", "set_outside_counts_device"):
        assert hasattr(elba_amd.Engine, name), name
    L.elba_abi_version.restype = ctypes.c_int
    assert L.elba_abi_version() == 3
    assert ctypes.sizeof(capi.InduceCfg) == 16 and ctypes.sizeof(capi.Induced) == 3 * 8 + 18 * 8 and ctypes.sizeof(capi.InduceStats) == 9 * 8 + 3 * 4 + 4
    assert L.elba_induce_part(None, None, None, 0, None, None) == 1
    L.elba_free_induced(None)
