"""-m gpu: the read pileup and the prune (pileup.hip) at their kernels' own boundaries, on the cases of pileup_cases.py: sort keys of 32, 34
and 35 bits, launches with no endpoint, no pair or no read, endpoint counts around the 256-lane block edge, the emission rules one by
one, the closed form of the trim rule at its clamps, the flags at their thresholds, one context over changing sizes, which pair the
bad-interval report names, and the prune under every kind of mask, chained, after loaded pairs and after own alignments.  Every
comparison is exact equality with pileup_util.pileup / pileup_util.prune (test_gpu_pileup._check: every segment, offset, trimmed interval,
flag and stat); test_pileup_cases_cpu.py holds the cases' claims and the restatement itself on the CPU."""
import numpy as np
import pytest

import elba_amd
import gpu_util as gu
import pileup_cases as pc
import pileup_util as pu
import string_graph_util as sgu
import trim_util as tu
from elba_amd.capi import OVERLAP_DTYPE
from test_gpu_pileup import _check
from test_gpu_trim import _check as _check_trim, _source

pytestmark = pytest.mark.gpu

SG_STATS = ("bad_reads", "contained_reads", "edges_kept", "products", "marked", "removed", "nnz")


@pytest.fixture(autouse=True)
def _reference_once(monkeypatch):
    """_check asks pileup_util.pileup for the expected result: every (case, settings) is computed once and shared between the tests."""
    monkeypatch.setattr(pu, "pileup", pc.pileup_memo)


def _ids(cases):
    return [c.name for c in cases]


def _load(e, case):
    packed, off = _source(case.lens)
    e.set_reads(packed, off, case.lens.astype(np.uint32))
    e.set_overlaps(len(case.lens), case.rows, case.cols, case.vals)
    return packed, off


def _segs(p, v):
    a, b = int(p["seg_off"][v]), int(p["seg_off"][v + 1])
    return [(int(s), int(d)) for s, d in zip(p["seg_start"][a:b], p["seg_depth"][a:b])]


def _run(case, e=None):
    """Every setting of the case on a context (a fresh one unless given); the case's own claims about cfgs[0] are held against the device too."""
    own = e is None
    if own:
        e = elba_amd.Engine(17, 2, 8)
    _load(e, case)
    for i, cfg in enumerate(case.cfgs):
        got, st = _check(e, *case.args, **cfg)
        if i == 0:
            cl = case.claims
            if "E" in cl:
                assert st["intervals"] * 2 == cl["E"]
            if "max_depth" in cl:
                assert st["max_depth"] == cl["max_depth"]
            for v, want in cl.get("segs", {}).items():
                assert _segs(got, v) == want, v
            for v, want in cl.get("trim", {}).items():
                assert (int(got["trim_beg"][v]), int(got["trim_end"][v])) == want, v
            for v, want in cl.get("flags", {}).items():
                assert int(got["flags"][v]) == want, v
    if own:
        e.close()


@pytest.mark.parametrize("case", pc.wide_key_cases(), ids=_ids(pc.wide_key_cases()))
def test_sort_keys_of_32_34_and_35_bits(case):
    """Read ids with bit mb - 1 and positions with bit pb - 1 set, on four and on five passes of the sort; elba_trim_reads reads the same
    segments at the same widths."""
    e = elba_amd.Engine(17, 2, 8)
    packed, off = _load(e, case)
    for cfg in case.cfgs:
        got, st = _check(e, *case.args, **cfg)
        assert st["intervals"] > 400
        for mode in (0, 1):
            _check_trim(e, *tu.trim_of(packed, off, case.lens, pc.reference(case, cfg), cfg, mode=mode, min_len=1), mode, 1)
    e.close()


@pytest.mark.parametrize("case", pc.degenerate_cases(), ids=_ids(pc.degenerate_cases()))
def test_launches_without_endpoints_pairs_or_reads(case):
    e = elba_amd.Engine(17, 2, 8)
    _load(e, case)
    for cfg in case.cfgs[:2]:
        got, st = _check(e, *case.args, **cfg)
        for k, want in case.claims["stats"].items():
            assert st[k] == want, (k, st[k], want)
        assert st["intervals"] == 0 and st["max_depth"] == 0
        assert st["segments"] == int((case.lens > 0).sum()) and st["unsupported"] == len(case.lens)
        assert (got["seg_depth"] == 0).all() and (got["seg_start"] == 0).all()
    for cfg in case.cfgs[2:]:                                       # (one less margin: an interval survives)
        got, st = _check(e, *case.args, **cfg)
        assert st["intervals"] > 0
    e.close()


@pytest.mark.parametrize("case", pc.block_edge_cases(), ids=_ids(pc.block_edge_cases()))
def test_endpoint_and_read_counts_around_the_block_edge(case):
    _run(case)


@pytest.mark.parametrize("case", pc.emission_cases(), ids=_ids(pc.emission_cases()))
def test_emission_rules(case):
    _run(case)


@pytest.mark.parametrize("case", pc.trim_cases(), ids=_ids(pc.trim_cases()))
def test_trim_closed_form(case):
    _run(case)


@pytest.mark.parametrize("case", pc.flag_cases(), ids=_ids(pc.flag_cases()))
def test_flags_at_their_thresholds(case):
    _run(case)


def test_one_context_over_changing_sizes():
    """Closing slots, token memory and buffers of a larger run must not show in a smaller one behind it, nor a released workspace in the next."""
    wide = {c.claims["key_bits"]: c for c in pc.wide_key_cases()}
    by_name = {c.name: c for c in pc.degenerate_cases() + pc.block_edge_cases() + pc.emission_cases()}
    e = elba_amd.Engine(17, 2, 8)
    for case in (wide[35], by_name["M0"], by_name["margin_int_max"], by_name["E256_M257"], wide[34]):
        _load(e, case)
        _check(e, *case.args, **case.cfgs[0])
    e.release_workspace()
    _run(by_name["mid_64_ends_63_starts"], e)
    _run(by_name["n0_M257"], e)
    e.close()


@pytest.mark.parametrize("first,second", [(300, 700), (64, 65)], ids=["two_blocks", "one_wavefront"])
def test_bad_interval_report_names_the_smallest_accepted_pair(first, second):
    M = 60
    lens = np.full(M, 100, np.int64)
    rows, cols = (a.astype(np.int64) for a in np.triu_indices(M, 1))
    good = np.zeros(len(rows), OVERLAP_DTYPE)
    good["endQ"] = 50; good["begT"] = 20; good["endT"] = 100
    good["passed"] = 1; good["score"] = 1
    good["begQ"][5], good["endQ"][5], good["passed"][5], good["score"][5] = 60, 40, 0, 0        # bad, but accepted in neither mode
    bad = good.copy()
    bad["endT"][first] = 101                                       # outside [0, len]
    bad["begQ"][second], bad["endQ"][second] = 31, 30              # beg > end
    e = elba_amd.Engine(17, 2, 8)
    e.set_reads(*_source(lens), lens.astype(np.uint32))
    for mode in (0, 1):
        e.set_overlaps(M, rows, cols, bad)
        with pytest.raises(elba_amd.ElbaError) as x:
            e.read_pileup(mode=mode)
        assert x.value.status == 1
        assert "pair %d (%d, %d)" % (first, rows[first], cols[first]) in str(x.value), str(x.value)
        assert "T [20, 101)" in str(x.value)
        with pytest.raises(elba_amd.ElbaError) as x:
            e.export_pileup()
        assert x.value.status == 5
        e.set_overlaps(M, rows, cols, good)                        # the corrected list on the same context
        _check(e, lens, rows, cols, good, mode=mode, margin=2, min_depth=3, min_run=10, trim_len=10)
    e.close()


def _string_graph(e, M, rows, cols, vals, fuzz):
    sst = e.transitive_reduction(0.65, fuzz)
    _, _, wst = sgu.python_string_graph(M, rows, cols, vals, 0.65, fuzz)
    for k in SG_STATS:
        assert sst[k] == wst[k], (k, sst[k], wst[k])
    return sst


def _prune(e, lens, rows, cols, vals, flags, mask, cfg, fuzz):
    """One prune against the restatement: the count, then the kept pairs' content through a full pileup of them and through the string graph."""
    kept = e.prune_reads(mask)
    r, c, v = pu.prune(rows, cols, vals, flags, mask)
    assert kept == len(r), (mask, kept, len(r))
    with pytest.raises(elba_amd.ElbaError) as x:
        e.export_pileup()                                          # the prune invalidates the pileup
    assert x.value.status == 5
    got, _ = _check(e, lens, r, c, v, **cfg)
    _string_graph(e, len(lens), r, c, v, fuzz)
    return r, c, v, got


@pytest.mark.parametrize("mask", [0, 1, 2, 3, 4, 255])
def test_prune_masks_on_a_loaded_list(mask):
    case = pc.prune_list()
    cfg = case.cfgs[0]
    e = elba_amd.Engine(17, 2, 8)
    _load(e, case)
    got, _ = _check(e, *case.args, **cfg)
    r, c, v, _ = _prune(e, case.lens, case.rows, case.cols, case.vals, got["flags"], mask, cfg, 100)
    if mask in (0, 4):
        assert len(r) == len(case.rows)                            # no flag has the bit: everything is kept
    else:
        assert 0 < len(r) < len(case.rows)
    e.close()


def test_prune_masks_on_own_alignments():
    packed, off, lens, info = elba_amd.synth_reads(8, 60000, 10, 3000, 500, error_rate=0.02, min_len=500)
    e, _, _, _ = gu.gpu_full(packed, off, lens, 17, 2, 12)
    lens64 = lens.astype(np.int64)
    # chosen on the CPU with oracle/pyoracle.py's align_upper (the device's alignments) and pileup_util: of the 200 reads one is
    # unsupported and six are split, and masks 1, 2 and 3 keep 1888, 1794 and 1788 of the 1894 pairs
    cfg = dict(mode=0, margin=100, min_depth=4, min_run=500, trim_len=500)
    kept = {}
    for mask in (0, 1, 2, 3, 4, 255):
        e.align_seeds()                                            # (a prune makes its kept pairs the loaded list: align again for the own ones)
        ov = e.export_overlaps()
        got, _ = _check(e, lens64, ov["rows"], ov["cols"], ov["vals"], **cfg)
        r, c, v, _ = _prune(e, lens64, ov["rows"], ov["cols"], ov["vals"], got["flags"], mask, cfg, 1000)
        kept[mask] = len(r)
        assert e.export_overlaps()["n"] == ov["n"]                 # the alignments stay
    assert kept[0] == kept[4] == ov["n"] and kept[3] == kept[255] < kept[2] < kept[1] < kept[0]
    e.close()


def test_prune_that_keeps_nothing_and_empty_list():
    case = pc.all_unsupported_case()
    cfg = case.cfgs[0]
    e = elba_amd.Engine(17, 2, 8)
    _load(e, case)
    got, _ = _check(e, *case.args, **cfg)
    assert (got["flags"] == 1).all()
    r, c, v, got = _prune(e, case.lens, case.rows, case.cols, case.vals, got["flags"], 1, cfg, 100)
    assert len(r) == 0
    for mask in (0, 3):                                            # n = 0: a prune of the empty list
        r, c, v, got = _prune(e, case.lens, r, c, v, got["flags"], mask, cfg, 100)
        assert len(r) == 0
    e.set_overlaps(len(case.lens), case.rows[:0], case.cols[:0], case.vals[:0])
    got, _ = _check(e, case.lens, case.rows[:0], case.cols[:0], case.vals[:0], **cfg)
    _prune(e, case.lens, case.rows[:0], case.cols[:0], case.vals[:0], got["flags"], 255, cfg, 100)
    e.close()


def test_prune_chain_swaps_buffers_and_invalid_masks():
    """pileup -> prune(2) -> pileup -> prune(1) -> pileup -> string graph: the second prune reads the buffers the first one wrote and writes
    the ones it read.  Then the original list again, and masks outside one byte."""
    case = pc.prune_list()
    cfg = case.cfgs[0]
    steps = pc.prune_chain(case)
    e = elba_amd.Engine(17, 2, 8)
    _load(e, case)
    first, _ = _check(e, *case.args, **cfg)
    r, c, v, got = _prune(e, case.lens, case.rows, case.cols, case.vals, first["flags"], 2, cfg, 100)
    assert (r == steps[1][0]).all() and (c == steps[1][1]).all() and (got["flags"] == steps[1][3][0]["flags"]).all()
    r, c, v, got = _prune(e, case.lens, r, c, v, got["flags"], 1, cfg, 100)
    assert (r == steps[2][0]).all() and (c == steps[2][1]).all() and (v == steps[2][2]).all()
    assert 0 < len(r) < len(steps[1][0]) < len(case.rows)
    e.set_overlaps(len(case.lens), case.rows, case.cols, case.vals)
    again, _ = _check(e, *case.args, **cfg)
    for k in ("seg_off", "seg_start", "seg_depth", "trim_beg", "trim_end", "flags"):
        assert (again[k] == first[k]).all(), k
    for mask in (-1, 256):
        with pytest.raises(elba_amd.ElbaError) as x:
            e.prune_reads(mask)
        assert x.value.status == 1
        still = e.export_pileup()                                  # the pileup stays valid
        assert (still["flags"] == first["flags"]).all() and (still["seg_depth"] == first["seg_depth"]).all()
    assert e.prune_reads(3) == len(pu.prune(case.rows, case.cols, case.vals, first["flags"], 3)[0])
    e.close()
