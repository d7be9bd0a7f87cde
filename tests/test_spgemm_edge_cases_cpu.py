"""CPU: every case of spgemm_edge_cases.py is what it claims, proved with the repository's own oracle (Oracle.set_triples + spgemm) alone: the widths of
the hub rows of the oracle's B, the owned partners and mirror images counted from the oracle's columns of A under the ownership rule, the longest
column, the largest position and the bit count of the one-word CSR sort on the claimed side of their switches.  A case that misses its claim fails
here, before tests/test_gpu_spgemm_edges.py spends GPU time on it.

The tier limits are restated as literals (TIER_LIMITS) from the (block, tbits) pairs of the tier table; elba_amd/hostcpp/test_ov_plan.cpp holds the same
literals against plan_ov.  If the geometry changes, both fail: re-derive group a (tier_case, guaranteed_case: the owned-partner counts and the entries
that place a hub by the cold estimate)."""
import functools

import numpy as np
import pytest

import spgemm_edge_cases as ec
from oracle import pyoracle as po

CASES = ec.all_cases()


@functools.lru_cache(maxsize=None)
def _oracle(case):
    o = po.Oracle(17, 2, 8)
    o.set_triples(*case.triples)
    o.spgemm(4)
    return o


def test_tier_limits_restate_the_tier_table():
    """min(3T/4, T - block) - 1 of every family's (block, tbits) pairs; the values the issue of this file names"""
    for family, rows in ec.TIER_BLOCKS.items():
        for t, (block, tbits) in enumerate(rows):
            T = 1 << tbits
            assert tbits == ec.LDS_TBITS0 + t
            assert ec.TIER_LIMITS[family][t] == min(3 * T // 4, T - block) - 1, (family, t)
    assert ec.TIER_LIMITS["s32"] == ec.TIER_LIMITS["pay"] == ec.TIER_LIMITS["pay16"] == (383, 767, 1535, 3071, 6143)
    assert ec.TIER_LIMITS["dense1"] == (255, 511, 1535, 3071, 6143)


def test_ownership_rule():
    assert ec.owns(0, 2) and not ec.owns(0, 3) and ec.owns(3, 0) and not ec.owns(2, 0) and ec.owns(5, 7) and not ec.owns(7, 5) and ec.owns(7, 4) and not ec.owns(4, 7)
    assert ec.owns(0, 3, dense=True) and not ec.owns(3, 0, dense=True)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_case_is_what_it_claims(case):
    o = _oracle(case)
    cl = case.claims
    A, B = o.A(), o.B()
    assert (A["M"], A["N"], A["Z"]) == (case.M, case.N, len(case.rows))
    widths = np.diff(B["rowptr"])
    entries = np.diff(A["rowptr"])
    owned, images, longest = ec.pattern_facts(case.M, A["colptr"], A["csc_read"], cl["dense"])
    assert longest == cl["max_col"], (longest, cl["max_col"])
    for h, c in cl["hubs"].items():
        got = {"width": int(widths[h]), "owned": int(owned[h]), "images": int(images[h]), "entries": int(entries[h])}
        assert got == {k: c[k] for k in got}, (case.name, h, got, c)
    maxpos = int(case.vals.max())
    assert (maxpos < 65536) == cl["pos16"], maxpos
    if "max_pos" in cl:
        assert maxpos == cl["max_pos"]
    if "hints" in cl:
        assert (ec.bits_for(maxpos) <= 30) == bool(cl["hints"])
    if "bits" in cl:
        assert ec.bits_for(case.M - 1) + ec.bits_for(case.N - 1) + ec.bits_for(maxpos) + 2 == cl["bits"] and (cl["bits"] <= 64) == bool(cl["csr_words"])
    if "sort_rows" in cl:
        assert (int(((widths > ec.FIN_WAVE2_MAX) & (widths <= ec.FIN_LDS_MAX)).sum()), int((widths > ec.FIN_LDS_MAX).sum())) == tuple(cl["sort_rows"])
    if "partner_width_max" in cl:
        others = np.delete(widths, list(cl["hubs"]))
        assert others.max() <= cl["partner_width_max"]
    if "other_rows_owned_max" in cl:      # the hub alone can pass a limit
        assert np.delete(owned, list(cl["hubs"])).max() <= cl["other_rows_owned_max"]
    if cl.get("one_bucket"):      # every column of a hub's row of B, the diagonal included, falls into one bucket of the sort that takes the row
        for h, c in cl["hubs"].items():
            b = ec.fin_bucket(B["col"][int(B["rowptr"][h]):int(B["rowptr"][h + 1])], c["width"], case.M)
            assert len(b) == c["width"] and len(np.unique(b)) == 1, (h, np.unique(b))
        assert ec.fin_bucket(case.M - 1, 4096, case.M) == ec.FIN_BUCKETS - 1 and int(B["col"].max()) == case.M - 1
        w12 = ec.widths_case("consecutive", "rec16")      # (at M = 12 000 a consecutive row of 1025 entries spans a dozen buckets, one of 4096 entries all 512)
        assert len(np.unique(ec.fin_bucket(np.arange(5000, 6025), 1025, w12.M))) >= 11 and len(np.unique(ec.fin_bucket(np.arange(5000, 9096), 4096, w12.M))) > 170
    if "max_numshared" in cl:
        assert o.stat("maxshared") == cl["max_numshared"]
        for (i, j), n in cl["pair_numshared"].items():
            a, b = int(B["rowptr"][i]), int(B["rowptr"][i + 1])
            k = a + int(np.searchsorted(B["col"][a:b], j))
            assert int(B["col"][k]) == j and int(B["val"]["numshared"][k]) == n and n > (1 << 15)
    if "pay16" in cl:
        assert (int(entries.max()) << cl["fbits"] <= 65536) == bool(cl["pay16"]) and int(entries.max()) == cl["hubs"][0]["entries"]
        # the hub's last 400 entries are the surviving pairs: its row of A ends in them
        a, b = int(A["rowptr"][0]), int(A["rowptr"][1])
        last = A["csr_kid"][b - 400:b]
        assert (np.diff(A["colptr"])[last] == 2).all() and last.min() >= case.N - 400


def test_cases_of_one_switch_differ_in_one_entry():
    """group e: the two matrices of a switch are the same matrix but for one entry (the longest column: one entry per copy of the column)"""
    def triples(c):
        return set(zip(c.rows.tolist(), c.cols.tolist(), c.vals.tolist()))
    for a, b, n in [(ec.column_case(L), ec.column_case(L + 1), 2) for L in (4, 16, 32, 64)] + [(ec.pay16_case(4, 16384), ec.pay16_case(4, 16385), None), (ec.pay16_case(8, 8192), ec.pay16_case(8, 8193), None)]:
        if n is not None:
            assert len(triples(a) ^ triples(b)) == n and len(b.rows) == len(a.rows) + n, (a.name, b.name)
        else:
            assert len(b.rows) == len(a.rows) + 1 and b.claims["hubs"][0]["entries"] == a.claims["hubs"][0]["entries"] + 1
    for lo, hi in ((65535, 65536), ((1 << 30) - 1, 1 << 30)):
        a, b = ec.position_case(lo), ec.position_case(hi)
        assert (a.rows == b.rows).all() and (a.cols == b.cols).all() and int((a.vals != b.vals).sum()) == 1
    a, b = ec.csr_words_case(False), ec.csr_words_case(True)
    assert len(b.rows) == len(a.rows) + 2 and b.N == a.N + 1 and (a.rows == b.rows[:len(a.rows)]).all()


def test_slab_sizes_use_the_floor_of_the_product():
    rp = np.array([0, 3, 3, 10, 11])
    assert (ec.slab_sizes(rp, 1) == 16).all()
    assert list(ec.slab_sizes(rp, 20000)) == [16, 16, 19, 16] and list(((rp * 20000) >> 16) + 16 * np.arange(5)) == [0, 16, 32, 51, 67]
