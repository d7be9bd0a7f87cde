"""-m gpu: the compiled-geometry reads-path kernel of the overlap SpGEMM (k_spgemm_direct<..., TB, SPEC, GEOM>: table size, claim limit, column stride 8,
four lanes per row entry and fbits 3 are constants; csrc/ov_plan.hpp: ov_spec_geom_ok) and the one row-count kernel in front of the row pointers
(spgemm.hip: k_row_counts).

Matrices are triples from the builders of tests/spgemm_edge_cases.py, shaped so that the reads path takes them (columns of two or three rows: one gather
trip; positions below 2^16; hints and inline partners) and widened by ONE column of five rows to the stride of 8 entries.  Every case is multiplied by
three kernels on the same engine — the compiled-geometry one (stat "overlap_spec_geom" = 1), the reads path with run-time geometry (option "ov_generic"
= 2) and the general kernel ("ov_generic" = 1) —, each in a cold, a steady and a second cold call: all nine B (rowptr, col, the five value fields) must
equal the oracle's bit for bit and the calls' statistics must agree.

  a. a hub row with limit - 1, limit and limit + 1 owned partners on each of the LDS tiers 0 .. 4 (it stays, stays, is handed on); tier 4 runs the
     sweep's loop path, the others four slots per lane.  The hub's rows have a partial last chunk, its partners' rows one entry.
  b. fewer than 8192 rows (no sample, no slabs) and just above (a sampled cold call with slabs)
  c. longest column 5 and 8 (stride 8: compiled geometry), 9 (stride 16) and 4 (stride 4): the last two keep the run-time geometry
  d. slabs of exactly 16 entries that overflow: tickets, the list walk of k_mirror
  e. rows of 1025 and 4097 entries of B: the wide-row queues of k_row_counts / k_row_pointers feed k_finalize_bucket and k_finalize_huge — without slabs
     (k_row_pointers queues), with slabs (k_row_counts in front of k_row_pointers) and beyond 2^17 rows (k_row_counts in front of the scan)
  f. 32-byte records (a position >= 65536): the row walk of k_mirror"""
import functools

import numpy as np
import pytest

import elba_amd
import gpu_util as gu
import spgemm_edge_cases as ec
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

NUM_TIERS = ec.NUM_LDS_TIERS + 1
LIMITS = ec.TIER_LIMITS["pay16"]      # (383, 767, 1535, 3071, 6143): the GPU tests read them from the engine as well
ST_KEYS = ("nnz", "products", "nnz_before_prune", "nnz_diag", "nnz_upper", "max_numshared")
STATS = ("overlap_slab_q16", "overlap_mirror_placed", "overlap_sort_rows_bucket", "overlap_sort_rows_huge")
KERNELS = ((0, "geom"), (2, "rt"), (1, "general"))      # option "ov_generic" -> name


def _widen(case, members, name=None):
    """the case plus ONE column of len(members) rows (a longest column of 5 .. 8 makes the padded stride 8)"""
    members = np.asarray(members, np.int64)
    assert members.min() >= 0 and members.max() < case.M and len(np.unique(members)) == len(members)
    rows = np.concatenate([case.rows, members]); cols = np.concatenate([case.cols, np.full(len(members), case.N)])
    vals = np.concatenate([case.vals, (np.arange(len(members)) * 41 + 7).astype(np.uint32)])
    return ec.Case(name or case.name + "_w%d" % len(members), case.M, case.N + 1, rows, cols, vals, dict(case.claims), case.options)


@functools.lru_cache(maxsize=None)
def hub_case(tier, owned):
    """Hub row 0 with exactly `owned` owned partners (even rows, ONE shared column {0, partner} each but the first 40, which share two and survive) and 30
    partners it does not own (odd rows, two columns each: 30 mirror images); the last rows hold one column of five.  Columns of two rows: Z < 3 N."""
    M = 2 * owned + 200
    m = ec._Mat(M, 9000 + 17 * tier + owned)
    mine, theirs = 2 * np.arange(1, owned + 1), 2 * np.arange(30) + 1
    assert ec.owns(0, mine).all() and not ec.owns(0, theirs).any()
    m.star(0, mine[:40], shared=2)
    m.star(0, mine[40:], shared=1)
    m.star(0, theirs, shared=2)
    m.columns(np.array([[M - 9, M - 7, M - 5, M - 3, M - 1]]))      # (odd rows beyond every partner)
    Mx, N, rows, cols, vals = m.finish(0, 60000)
    claims = {"owned": owned, "tier": tier, "entries": owned + 40 + 60, "width": 1 + 40 + 30}
    return ec.Case("hub_t%d_%d" % (tier, owned), Mx, N, rows, cols, vals, claims, {"no_sample": 1})


@functools.lru_cache(maxsize=None)
def background_case(M):
    """columns of two and three rows all over M - 1 rows, one column of five; row M - 1 holds ONE entry"""
    m = ec._Mat(M, 9100)
    ec._background(m, M - 1, 3 * M, 0)
    m.columns(np.array([[1, 3, 5, 7, 9]]))
    m.columns(np.array([[0, M - 1]]))
    Mx, N, rows, cols, vals = m.finish(0, 60000)
    return ec.Case("background_%d" % M, Mx, N, rows, cols, vals, {}, {})


@functools.lru_cache(maxsize=None)
def wide_case(M):
    """two hub rows whose rows of B hold 1025 and 4097 entries (1024 / 4096 partners through two columns each + the diagonal)"""
    m = ec._Mat(M, 9200)
    h1, h2 = 311, 918
    p1 = ec._spread(M, 1024, {h1, h2})
    p2 = ec._spread(M, 4096, {h1, h2})
    m.star(h1, p1, shared=2)
    m.star(h2, p2, shared=2)
    m.columns(np.array([[h1, 0, 1, M // 2, M - 1]]))      # (the column of five; not on row h2: its 8192 entries << fbits are the most 16-bit sequence numbers hold)
    Mx, N, rows, cols, vals = m.finish(0, 60000)
    return ec.Case("wide_%d" % M, Mx, N, rows, cols, vals, {"sort_rows": (1, 1)}, {})


@functools.lru_cache(maxsize=None)
def _oracle(case):
    """the oracle of a case after its multiplication: computed once, shared, never changed"""
    o = po.Oracle(17, 2, 8)
    o.set_triples(*case.triples)
    o.spgemm(8)
    return o


def _tiers(e):
    return [e.get_stat("overlap_tier_queued_%d" % t) for t in range(NUM_TIERS)], [e.get_stat("overlap_tier_done_%d" % t) for t in range(NUM_TIERS)]


def _same(B, B0):
    assert (B["rowptr"] == B0["rowptr"]).all() and (B["col"] == B0["col"]).all() and B["val"].tobytes() == B0["val"].tobytes()


def _call(e, case, want):
    """one create_seed_matrix: which kernel ran, B and the statistics against the oracle; returns (B, statistics)"""
    o = _oracle(case)
    st = e.create_seed_matrix()
    assert (e.get_stat("overlap_spec"), e.get_stat("overlap_spec_geom")) == want, (case.name, want)
    B = e.export_csr()
    gu.assert_B_equal(B, o.B())
    gu.assert_stats_equal(st, o)
    rec = {k: st[k] for k in ST_KEYS}
    rec.update({n: e.get_stat(n) for n in STATS})
    return B, rec


def run_case(case, geom, spec=1, reach=None, options=None):
    """the three kernels x (cold, steady, cold) on one engine; geom / spec: what the plan must pick when no option forces another kernel; reach(e): checked
    after the first cold call of every kernel"""
    e = elba_amd.Engine(17, 2, 8, options={**case.options, **(options or {})})
    ms = e.set_kmer_matrix(*case.triples)
    assert (ms["nrows"], ms["ncols"], ms["nnz"]) == (case.M, case.N, len(case.rows))
    gu.assert_A_equal(e.export_kmer_matrix(), _oracle(case).A())
    B0, recs = None, {}
    for value, name in KERNELS:
        e.set_option("ov_generic", value)
        want = (spec, geom) if value == 0 else ((spec, 0) if value == 2 else (0, 0))
        e.set_option("overlap_cold_calls", 1)
        for call in ("cold", "steady", "cold2"):
            B, rec = _call(e, case, want)
            if B0 is None:
                B0 = B
            _same(B, B0)
            recs[name, call] = rec
            if call == "cold" and reach is not None:
                reach(e)
            e.set_option("overlap_cold_calls", 1 if call == "steady" else 0)
    e.close()
    for call in ("cold", "steady", "cold2"):
        for name in ("rt", "general"):
            assert recs[name, call] == recs["geom", call], (case.name, name, call, recs[name, call], recs["geom", call])
    return recs


# ---- a. the claim limits, compiled in ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tier", range(ec.NUM_LDS_TIERS))
@pytest.mark.parametrize("delta", (-1, 0, 1))
def test_a_hub_row_at_a_compiled_claim_limit_stays_and_one_partner_more_hands_it_on(tier, delta):
    """Table::insert_lds abandons a row at the claim that finds the claim counter >= limit: a row with `limit` owned partners completes on the tier, one
    with limit + 1 is handed to the next (tier 4: to the HBM tables).  The cold estimate (entries / 4) starts the hub below the tier; the tiers hand it up."""
    limit = LIMITS[tier]
    owned = limit + delta
    case = hub_case(tier, owned)
    A = _oracle(case).A()
    assert ec.pattern_facts(case.M, A["colptr"], A["csc_read"], False)[0][0] == owned      # (the oracle's columns: row 0 owns exactly `owned` partners)
    entries = case.claims["entries"]
    assert entries % 64 != 0 and (entries << 3) <= 65536
    start = next(t for t in range(ec.NUM_LDS_TIERS) if max(64, entries // 4) <= LIMITS[t])
    assert start <= tier
    end = tier if owned <= limit else tier + 1

    def reach(e):
        assert e.get_stat("matrix_col_stride") == 8 and e.get_stat("matrix_fbits") == 3
        assert [e.get_stat("overlap_tier_limit_%d" % t) for t in range(ec.NUM_LDS_TIERS)] == list(LIMITS)
        queued, done = _tiers(e)
        others = len(np.unique(case.rows)) - 1
        want_q, want_d = [0] * NUM_TIERS, [0] * NUM_TIERS
        want_q[0] += others; want_d[0] += others
        for t in range(start, end + 1):
            want_q[t] += 1
        want_d[end] += 1
        assert (queued, done) == (want_q, want_d), (case.name, queued, done, want_q, want_d)
        assert e.get_stat("overlap_forwarded") == 0

    run_case(case, geom=1, reach=reach)


# ---- b. no sample | a sampled cold call -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", (8000, 8200))
def test_below_and_above_the_sample_threshold(M):
    case = background_case(M)
    recs = run_case(case, geom=1)
    if M < 8192:
        assert recs["geom", "cold"]["overlap_slab_q16"] == 0      # (no sample: no ratio to size slabs by on a cold call)
    else:
        assert recs["geom", "cold"]["overlap_slab_q16"] > 0 and recs["geom", "cold2"]["overlap_slab_q16"] == recs["geom", "cold"]["overlap_slab_q16"]
    assert recs["geom", "steady"]["overlap_slab_q16"] > 0          # (a steady call sizes them by what the call before measured)


# ---- c. the strides ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("longest,stride,geom", ((4, 4, 0), (5, 8, 1), (8, 8, 1), (9, 16, 0)))
def test_only_a_stride_of_eight_takes_the_compiled_geometry(longest, stride, geom):
    case = ec.column_case(longest)

    def reach(e):
        assert e.get_stat("matrix_col_stride") == stride and e.get_stat("matrix_fbits") == {4: 2, 8: 3, 16: 4}[stride]

    run_case(case, geom=geom, spec=1, reach=reach)


# ---- d. tickets --------------------------------------------------------------------------------------------------------------------------------------
def test_full_slabs_hand_out_tickets_and_the_list_walk_places_them():
    base = ec.slab_case()
    case = _widen(base, [2891, 2893, 2895, 2897, 2899])
    want = sum(max(n - ec.SLAB_PAD, 0) for n in ec.IMAGES)      # images beyond a slab of exactly SLAB_PAD entries
    recs = run_case(case, geom=1, options={"slab_q16": 1})
    for rec in recs.values():
        assert rec["overlap_slab_q16"] == 1 and rec["overlap_mirror_placed"] == want, rec


# ---- e. the wide rows' queues ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", (6000, 12000))
def test_rows_of_1025_and_4097_entries_reach_the_block_sorts(M):
    """M = 6000: no sample, no slabs on the cold calls — k_row_pointers queues the wide rows; M = 12000: slabs — k_row_counts does"""
    case = wide_case(M)
    B = _oracle(case).B()
    width = np.diff(B["rowptr"])
    assert width[311] == 1025 and width[918] == 4097 and (np.delete(width, [311, 918]) <= ec.FIN_WAVE2_MAX).all()
    recs = run_case(case, geom=1)
    for rec in recs.values():
        assert (rec["overlap_sort_rows_bucket"], rec["overlap_sort_rows_huge"]) == (1, 1), rec
    assert (recs["geom", "cold"]["overlap_slab_q16"] > 0) == (M >= 8192)


@pytest.mark.parametrize("M,options", ((131071, {}), (131072, {}), (131072, {"no_slab": 1})))
def test_row_counts_in_front_of_the_scan(M, options):
    """M + 1 > 2^17: the row pointers are scanned from the lengths k_row_counts writes, with slab entries and without; M + 1 = 2^17: the largest tiled call"""
    base = ec.rowptr_case(M)
    case = _widen(base, [M - 12, M - 10, M - 8, M - 6, M - 4])
    recs = run_case(case, geom=1, options=options)
    for rec in recs.values():
        assert (rec["overlap_sort_rows_bucket"], rec["overlap_sort_rows_huge"]) == base.claims["sort_rows"], rec
    if options:
        assert all(rec["overlap_slab_q16"] == 0 for rec in recs.values())


# ---- f. 32-byte records -------------------------------------------------------------------------------------------------------------------------------
def test_32_byte_records_keep_the_row_walk_of_the_mirror_pass():
    case = ec.widths_case("spread", "pos32")
    recs = run_case(case, geom=0, spec=0)
    for rec in recs.values():
        assert (rec["overlap_sort_rows_bucket"], rec["overlap_sort_rows_huge"]) == case.claims["sort_rows"], rec
