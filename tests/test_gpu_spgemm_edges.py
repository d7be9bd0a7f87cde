"""-m gpu: the overlap SpGEMM and the build of A it reads at their tables', sorts' and slabs' own limits (csrc/spgemm.hip, spgemm_direct.hpp,
spgemm_table.hpp, ov_plan.hpp, matrix.hip).  The matrices of tests/spgemm_edge_cases.py — proved on the CPU by tests/test_spgemm_edge_cases_cpu.py —
put a row ON a constant; every case first proves from the diagnostics of elba_get_stat ("matrix_*", "overlap_tier_*", "overlap_sort_rows_*",
"overlap_family", "overlap_pay16", "overlap_rec16", "overlap_mirror_placed") that the row went where the case says, then compares A and B entry for entry
with the oracle, and requires a cold, a steady and a second cold call on the same engine to give bit-identical B.

  a. tier limits: a hub row with limit - 1, limit, limit + 1, T/2 and T/2 + 1 owned partners on every LDS tier of every kernel family (the limit read from
     "overlap_tier_limit_t"), placed by option "tune7" and by the cold estimate; guaranteed_tbits at need = T/2 | T/2 + 1
  b. finalize widths 1 .. 8193 in three partner layouts and three record formats; a pair with numshared > 2^15 in a 600-wide row; rows of 300, 1024,
     1025 and 4096 entries whose columns all fall into ONE bucket of their sort (M = 2^21: at M = 12 000 a consecutive row spans a dozen buckets or more)
  c. mirror slabs of exactly SLAB_PAD entries that receive 0 .. 300 images, a generous ratio, a ratio whose slab bases are no multiples of 16, no slabs
  d. row pointers of B for M around RP_TILE, 2 RP_TILE and 2^17
  e. the shape switches of A: longest column, largest position, the bit count of the one-word CSR sort, max_row_nnz << fbits, each also with "no_symmetry"
(The sharded entry points take reads, not triples, through DistributedOverlap: an edge matrix cannot reach them without changing distributed.py.)"""
import functools

import numpy as np
import pytest

import elba_amd
import gpu_util as gu
import spgemm_edge_cases as ec
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

NUM_TIERS = ec.NUM_LDS_TIERS + 1


@functools.lru_cache(maxsize=None)
def _oracle(case):
    """the oracle of a case after its multiplication: computed once, shared, never changed"""
    o = po.Oracle(17, 2, 8)
    o.set_triples(*case.triples)
    o.spgemm(8)
    return o


@functools.lru_cache(maxsize=None)
def _facts(case):
    A = _oracle(case).A()
    return ec.pattern_facts(case.M, A["colptr"], A["csc_read"], case.claims["dense"])


def _engine(case, **extra):
    # Below 2^18 row entries in all, the in-call prediction of a cold call (spgemm_direct.hpp: `gu >= 1 << 18`) never forwards a row: where a row starts
    # and ends is then a function of the matrix alone, which the exact queued / done vectors and "overlap_forwarded" == 0 below rely on.  A larger case
    # would depend on which rows finished first.
    assert len(case.rows) < (1 << 18), case.name
    e = elba_amd.Engine(17, 2, 8, options={**case.options, **extra})
    ms = e.set_kmer_matrix(*case.triples)
    assert (ms["nrows"], ms["ncols"], ms["nnz"]) == (case.M, case.N, len(case.rows))
    return e


def _tiers(e):
    return [e.get_stat("overlap_tier_queued_%d" % t) for t in range(NUM_TIERS)], [e.get_stat("overlap_tier_done_%d" % t) for t in range(NUM_TIERS)]


def _call(e, case, reach=None):
    """one create_seed_matrix: the reach check, then B and the statistics against the oracle; returns B"""
    o = _oracle(case)
    st = e.create_seed_matrix()
    if reach is not None:
        reach(st)
    B = e.export_csr()
    gu.assert_B_equal(B, o.B())
    gu.assert_stats_equal(st, o)
    assert st["rows_lds"] + st["rows_global"] == len(np.unique(case.rows)), (st["rows_lds"], st["rows_global"])
    queued, done = _tiers(e)
    assert sum(done) == st["rows_lds"] + st["rows_global"] and done[ec.NUM_LDS_TIERS] == st["rows_global"]
    return B


def _same(B, B0):
    assert (B["rowptr"] == B0["rowptr"]).all() and (B["col"] == B0["col"]).all() and B["val"].tobytes() == B0["val"].tobytes()


def _three_calls(e, case, reach=None, compare_A=True):
    """cold (with the reach check), steady, cold again: all three B equal the oracle's and are bit-identical; A equals the oracle's"""
    if compare_A:
        gu.assert_A_equal(e.export_kmer_matrix(), _oracle(case).A())
    B0 = _call(e, case, reach)
    _same(_call(e, case), B0)
    e.set_option("overlap_cold_calls", 1)
    _same(_call(e, case, reach), B0)
    e.set_option("overlap_cold_calls", 0)
    return B0


# ---- a. tier limits -----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _limits(family):
    """the family's tier limits as the engine reports them after a call on a small matrix of the family"""
    case = ec.tier_case(family, 0, 48)
    e = _engine(case, no_sample=1)
    e.create_seed_matrix()
    _check_family(e, family)
    lim = tuple(e.get_stat("overlap_tier_limit_%d" % t) for t in range(ec.NUM_LDS_TIERS))
    e.close()
    assert all(0 < lim[t] < (1 << (ec.LDS_TBITS0 + t)) for t in range(ec.NUM_LDS_TIERS)), lim
    return lim


def _check_family(e, family):
    _, fam, pay16, rec16 = ec.FAMILIES[family]
    assert (e.get_stat("overlap_family"), e.get_stat("overlap_pay16"), e.get_stat("overlap_rec16")) == (fam, pay16, rec16), family
    assert e.get_stat("matrix_suffix") == (1 if family.startswith("dense") else 0) and e.get_stat("matrix_pos16") == (0 if family == "s32" else 1)


def _hub_reach(e, case, family, tier, limit, nonempty, others_tier):
    """the reach check of a hub row with `owned` owned partners queued on `tier`: it completes there with <= limit of them, is handed on to tier + 1
    (5: the HBM tables) with limit + 1; every other row completes on `others_tier`"""
    owned = case.claims["hubs"][0]["owned"]
    assert _facts(case)[0][0] == owned

    def reach(st):
        _check_family(e, family)
        assert e.get_stat("overlap_tier_limit_%d" % tier) == limit
        queued, done = _tiers(e)
        want_q, want_d = [0] * NUM_TIERS, [0] * NUM_TIERS
        want_q[others_tier] += nonempty - 1; want_d[others_tier] += nonempty - 1
        want_q[tier] += 1
        if owned <= limit:
            want_d[tier] += 1
        else:
            want_q[tier + 1] += 1; want_d[tier + 1] += 1
        assert (queued, done) == (want_q, want_d), (case.name, owned, limit, queued, done)
        assert st["rows_escalated"] == (0 if owned <= limit else 1)
        assert e.get_stat("overlap_forwarded") == 0
    return reach


# (the dense family never starts a row below tier "dense_up" — k_classify_direct lifts it there after "tune7" —: its tiers below receive no row at all)
TIER_CASES = [(f, t) for f in ec.FAMILIES for t in range(ec.NUM_LDS_TIERS) if t >= ec.DENSE_UP.get(f, 0)]


@pytest.mark.parametrize("family,tier", TIER_CASES)
def test_a_row_at_a_tier_limit_completes_and_one_partner_more_is_handed_on(family, tier):
    """Table::insert_lds abandons a row at the claim that finds misc[9] >= limit: `limit` owned partners complete on the tier, limit + 1 hand the row on
    and the workgroup goes on with the partners' short rows on a re-initialised table.  Every row starts on the tier (option tune7)."""
    limit = _limits(family)[tier]
    for owned in ec.tier_counts(tier, limit):
        case = ec.tier_case(family, tier, owned)
        e = _engine(case, no_sample=1)      # (row 0 of 8192 rows or more would be a row of the cold call's sample, which runs on tier 3 first)
        nonempty = len(np.unique(case.rows))
        assert nonempty > 40
        _three_calls(e, case, _hub_reach(e, case, family, tier, limit, nonempty, tier))
        e.close()


@pytest.mark.parametrize("family", list(ec.FAMILIES))
def test_a_row_placed_by_the_cold_estimate_at_its_tier_limit(family):
    """no tune7: k_classify_direct's estimate max(64, entries / 4) alone starts the hub on the tier, every other row on the family's lowest"""
    tier = ec.ESTIMATE_TIER[family]
    limit = _limits(family)[tier]
    assert limit == ec.TIER_LIMITS[family][tier]      # (the hub's padding entries were sized from the restated limits)
    others = ec.DENSE_UP.get(family, 0)
    for owned in (limit, limit + 1):
        case = ec.tier_case(family, tier, owned, "estimate")
        e = _engine(case, no_sample=1)
        _three_calls(e, case, _hub_reach(e, case, family, tier, limit, len(np.unique(case.rows)), others))
        e.close()


@pytest.mark.parametrize("pos16", [True, False])
@pytest.mark.parametrize("tier", range(ec.NUM_LDS_TIERS))
def test_guaranteed_tier_switches_at_half_the_table(tier, pos16):
    """M = T/2 rows: the hub, whose estimate asks for tier + 1, starts on `tier` (guaranteed to fit M partners at load 1/2); M = T/2 + 1: on tier + 1"""
    for above in (False, True):
        case = ec.guaranteed_case(tier, above, pos16)
        e = _engine(case)
        nonempty = len(np.unique(case.rows))
        start = tier + (1 if above else 0)

        def reach(st):
            assert e.get_stat("overlap_tier_limit_%d" % tier) < case.claims["hubs"][0]["entries"] // 4
            queued, done = _tiers(e)
            want = [0] * NUM_TIERS
            want[0] += nonempty - 1; want[start] += 1
            assert queued == want and done == want, (case.name, queued, done)
            assert st["rows_escalated"] == 0 and st["rows_global"] == (1 if start == ec.NUM_LDS_TIERS else 0)
        _three_calls(e, case, reach)
        e.close()


# ---- b. finalize widths -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", list(ec.FORMATS))
@pytest.mark.parametrize("layout", ["spread", "consecutive", "ends"])
def test_rows_of_every_finalize_width(layout, fmt):
    """k_finalize_wave (<= 256), _mid / _mid16 (<= 1024), _bucket (<= 4096), _huge: one row per width at and around every switch"""
    case = ec.widths_case(layout, fmt)
    e = _engine(case)
    assert e.get_stat("matrix_pos16") == (1 if case.claims["pos16"] else 0)

    def reach(st):
        assert e.get_stat("overlap_rec16") == case.claims["rec16"]
        assert (e.get_stat("overlap_sort_rows_bucket"), e.get_stat("overlap_sort_rows_huge")) == case.claims["sort_rows"]
    B = _three_calls(e, case, reach)
    got = np.diff(B["rowptr"])
    assert sorted(int(got[h]) for h in case.claims["hubs"]) == list(ec.WIDTHS)
    if layout != "spread":
        assert B["col"].max() == case.M - 1 and got[0] > 0 and got[case.M - 1] > 0      # (column M - 1: the last bucket of the bucket sorts)
    e.close()


@pytest.mark.parametrize("fmt", ["rec16", "mir32"])
def test_rows_whose_columns_all_fall_into_one_bucket(fmt):
    """k_finalize_mid16 / _mid (rec16 / mir32) and k_finalize_bucket with every entry of a row in one bucket: the sort degrades to a rank sort, never to a wrong result"""
    case = ec.one_bucket_case(fmt)
    e = _engine(case)

    def reach(st):
        assert e.get_stat("overlap_rec16") == case.claims["rec16"] and e.get_stat("matrix_pos16") == 1
        assert (e.get_stat("overlap_sort_rows_bucket"), e.get_stat("overlap_sort_rows_huge")) == case.claims["sort_rows"]
    B = _three_calls(e, case, reach)
    for h, c in case.claims["hubs"].items():
        cols = B["col"][int(B["rowptr"][h]):int(B["rowptr"][h + 1])]
        assert len(cols) == c["width"] and len(np.unique(ec.fin_bucket(cols, c["width"], case.M))) == 1
    assert int(B["col"].max()) == case.M - 1
    e.close()


def test_a_large_numshared_in_a_row_of_the_mid16_sort():
    case = ec.numshared_case()
    e = _engine(case)

    def reach(st):
        assert e.get_stat("overlap_rec16") == 1 and e.get_stat("overlap_family") == ec.OV_PAY
        assert st["max_numshared"] == case.claims["max_numshared"] > (1 << 15)
        assert (e.get_stat("overlap_sort_rows_bucket"), e.get_stat("overlap_sort_rows_huge")) == (0, 0)
    B = _three_calls(e, case, reach)
    (h, c), = case.claims["hubs"].items()
    a, b = int(B["rowptr"][h]), int(B["rowptr"][h + 1])
    assert b - a == c["width"] and ec.FIN_WAVE_MAX < b - a <= ec.FIN_WAVE2_MAX
    for (i, j), n in case.claims["pair_numshared"].items():
        assert int(B["val"]["numshared"][a + int(np.searchsorted(B["col"][a:b], j))]) == n
    e.close()


# ---- c. mirror slabs ------------------------------------------------------------------------------------------------------------------------------------
def test_mirror_slabs_that_receive_as_many_images_as_they_hold_one_fewer_and_one_more():
    case = ec.slab_case()
    o = _oracle(case)
    images = _facts(case)[1]
    for r, c in case.claims["hubs"].items():
        assert images[r] == c["images"]
    a_rowptr = o.A()["rowptr"]
    e = _engine(case)
    assert e.get_stat("matrix_pos16") == 1 and len(case.rows) < 65536

    def run(q16, pct, expect_q16, expect_placed, no_slab=0):
        e.set_option("slab_q16", q16); e.set_option("slab_pct", pct); e.set_option("no_slab", no_slab)

        def reach(st):
            assert e.get_stat("overlap_rec16") == 1
            assert (e.get_stat("overlap_slab_q16"), e.get_stat("overlap_mirror_placed")) == (expect_q16, expect_placed), (q16, pct, no_slab)
        # (all three calls with the forced ratio: the option overrides what a steady call would carry over)
        e.set_option("overlap_cold_calls", 1)
        B0 = _call(e, case, reach)
        e.set_option("overlap_cold_calls", 0)
        _same(_call(e, case, reach), B0)
        e.set_option("overlap_cold_calls", 1)
        _same(_call(e, case, reach), B0)
        return B0

    gu.assert_A_equal(e.export_kmer_matrix(), o.A())
    exact = int(np.maximum(images - ec.SLAB_PAD, 0).sum())
    assert exact == (17 - 16) + (40 - 16) + (300 - 16)
    B1 = run(1, 175, 1, exact)                                   # every slab exactly SLAB_PAD entries
    _same(run(1 << 18, 100, 1 << 18, 0), B1)                      # four entries per row entry + the pad: no ticket drawn
    sizes = ec.slab_sizes(a_rowptr, 20000)
    bases = np.cumsum(sizes) - sizes
    ratio = int(np.maximum(images - sizes, 0).sum())
    assert (bases % 16 != 0).sum() > 100 and 0 < ratio < exact
    _same(run(20000, 100, 20000, ratio), B1)                      # slab bases from the floor of the product, no multiples of 16
    _same(run(0, 175, 0, int(images.sum()), no_slab=1), B1)       # no slabs: every image takes a ticket
    e.close()


# ---- d. row pointers ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", ec.ROWPTR_M)
def test_row_pointers_of_B_around_the_tile_and_the_scan(M):
    """k_row_pointers scans RP_TILE counts per workgroup (M + 1 <= 2^17), k_sum_counts + the scan beyond; the widest row sits in the last tile"""
    case = ec.rowptr_case(M)
    e = _engine(case)
    (wide, c), = [(h, c) for h, c in case.claims["hubs"].items() if c["width"] > 2]
    assert wide // ec.RP_TILE == (M - 1) // ec.RP_TILE and case.claims["scan"] == (M + 1 > (1 << 17))

    def reach(st):
        assert st["nrows"] == M
        assert (e.get_stat("overlap_sort_rows_bucket"), e.get_stat("overlap_sort_rows_huge")) == case.claims["sort_rows"]
    B = _three_calls(e, case, reach)
    got = np.diff(B["rowptr"])
    assert wide == M - 1 and got[wide] == c["width"] and all(got[r] == 2 for r in (0, 1023, 1024) if r < M - 1)
    e.close()


# ---- e. shape switches of A ---------------------------------------------------------------------------------------------------------------------------
def _expected_family(cl, no_symmetry):
    """(overlap_family, overlap_pay16) of a pos16 matrix"""
    if cl.get("suffix"):
        return (ec.OV_PAY, 0) if no_symmetry else (ec.OV_DENSE, 0)
    if cl.get("stride", 4) and cl.get("pay16", 1):
        return (ec.OV_S32, 1)
    return (ec.OV_PAY, 0)


def _shape_case(case, no_symmetry, matrix_stats, call_stats=None):
    e = _engine(case, **({"no_symmetry": 1} if no_symmetry else {}))
    got = {k: e.get_stat(k) for k in matrix_stats}
    assert got == matrix_stats, (case.name, got)

    def reach(st):
        if call_stats:
            now = {k: e.get_stat(k) for k in call_stats}
            assert now == call_stats, (case.name, now)
    _three_calls(e, case, reach)
    e.close()


@pytest.mark.parametrize("no_symmetry", [0, 1])
@pytest.mark.parametrize("longest", [4, 5, 16, 17, 32, 33, 64, 65])
def test_longest_column_switches(longest, no_symmetry):
    case = ec.column_case(longest)
    cl = case.claims
    fam, pay16 = _expected_family(cl, no_symmetry)
    _shape_case(case, no_symmetry, {"matrix_col_stride": cl["stride"], "matrix_fbits": cl["fbits"], "matrix_suffix": cl["suffix"], "matrix_pos16": 1, "padded_columns": 1 if cl["stride"] else 0},
                {"overlap_family": fam, "overlap_pay16": pay16, "overlap_rec16": 1})


@pytest.mark.parametrize("no_symmetry", [0, 1])
@pytest.mark.parametrize("largest", [65535, 65536, (1 << 30) - 1, 1 << 30])
def test_largest_position_switches(largest, no_symmetry):
    case = ec.position_case(largest)
    cl = case.claims
    pos16 = 1 if cl["pos16"] else 0
    _shape_case(case, no_symmetry, {"matrix_pos16": pos16, "matrix_hints": cl["hints"], "matrix_inline": pos16 if not no_symmetry else 0, "matrix_suffix": 0, "matrix_col_stride": 4},
                {"overlap_family": ec.OV_S32, "overlap_pay16": pos16, "overlap_rec16": pos16})


@pytest.mark.parametrize("tune1", [0, 1])      # 1: the sorted words are unpacked by a kernel of its own (k_unpack_csr_words), not by the sort's last pass
@pytest.mark.parametrize("no_symmetry", [0, 1])
@pytest.mark.parametrize("over", [False, True])
def test_one_word_csr_sort_switch(over, no_symmetry, tune1):
    """mb + nb + pb + 2 = 64: the read's top bit is bit 63 of the sort word — rows beyond 2^16 of the 2^17 must not be taken for inline partners"""
    case = ec.csr_words_case(over)
    if tune1:
        case = ec.Case(case.name + "_tune1", *case.triples, case.claims, {"tune1": 1})
    _shape_case(case, no_symmetry, {"matrix_csr_words": case.claims["csr_words"], "matrix_hints": 0, "matrix_pos16": 0}, {"overlap_family": ec.OV_S32, "overlap_pay16": 0, "overlap_rec16": 0})


@pytest.mark.parametrize("no_symmetry", [0, 1])
@pytest.mark.parametrize("stride,entries", [(4, 16384), (4, 16385), (8, 8192), (8, 8193)])
def test_product_sequence_numbers_at_16_bits(stride, entries, no_symmetry):
    """pay16 needs max_row_nnz << fbits <= 65536; the hub's last entries carry surviving pairs whose seeds name their sequence numbers' positions"""
    case = ec.pay16_case(stride, entries)
    cl = case.claims
    fam, pay16 = _expected_family(cl, no_symmetry)
    _shape_case(case, no_symmetry, {"matrix_col_stride": stride, "matrix_fbits": cl["fbits"], "matrix_pos16": 1, "matrix_suffix": 0},
                {"overlap_family": fam, "overlap_pay16": pay16, "overlap_rec16": 1})
