"""-m gpu: elba_align_seeds driven with PLANTED seeds (tests/xdrop_util.py: set_reads + set_kmer_matrix with chosen triples, so that
B(i, j).seeds[0] is the seed a case asks for) against Oracle.align_upper on the same triples.  The families — rejected seeds, corner and
edge seeds, 1 : 100 length ratios, repeats with ties, long indels, a band-width ladder across the register tiers, extreme score sets, k from
3 to 95, reads of 70 000+ bases, numshared around the tier hint — and what each of them demonstrably does are checked on the CPU by
tests/test_xdrop_planted_cpu.py, where the oracle is also pinned to the reference's own build.  Exact equality on every field."""
import os

import numpy as np
import pytest

import elba_amd
import gpu_util as gu
import util
import xdrop_util as xu
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

BIG = 1 << 30
# (aln_tiers, aln_wide_hint, aln_long_hint); the library's defaults are (0 = all four tiers, 6, 6000)
TIER_CONFIGS = [(t, 6, 6000) for t in (0, 1, 2, 4, 8, 24, 1248)]
HINT_CONFIGS = [(0, -1, BIG),       # (a) both hints off: every extension starts on the first tier
                (0, BIG, BIG),      # (b) everything skips the first tier, nothing skips the second
                (0, BIG, 0),        # (c) everything skips the first tier and the second
                (1, BIG, BIG),      # and with the first tier alone: everything skips it, straight to the strided kernel ...
                (1, -1, BIG)]       # ... or nothing does: only what outgrows 64 columns reaches it
ALL_STRIDED, FIRST_TIER_ONLY = HINT_CONFIGS[3], HINT_CONFIGS[4]
CONFIGS = TIER_CONFIGS + HINT_CONFIGS


def _engine(k, pl):
    packed, off, lens, M, N, rows, cols, vals = pl
    e = elba_amd.Engine(k, 2, 8)
    e.set_reads(packed, off, lens)
    e.set_kmer_matrix(M, N, rows, cols, vals)
    e.create_seed_matrix()
    return e


def _oracle(k, pl):
    packed, off, lens, M, N, rows, cols, vals = pl
    o = po.Oracle(k, 2, 8)
    o.set_triples(M, N, rows, cols, vals)
    o.spgemm(1)
    return o


def _configure(e, cfg):
    e.set_option("aln_tiers", cfg[0]); e.set_option("aln_wide_hint", cfg[1]); e.set_option("aln_long_hint", cfg[2])


def _compare(e, want, params, what):
    rows, cols, ov, cells = want
    st = e.align_seeds(*params)
    g = e.export_overlaps()
    assert st["nalignments"] == len(rows) == g["n"], what
    assert (g["rows"] == rows).all() and (g["cols"] == cols).all(), what
    for f in ov.dtype.names:
        if f == "pad":
            continue
        bad = np.nonzero(g["vals"][f] != ov[f])[0]
        assert len(bad) == 0, (what, f, len(bad), bad[:5], g["vals"][bad[:5]], ov[bad[:5]])
    assert st["cells"] == cells, (what, st["cells"], cells)
    assert st["passed"] == int(ov["passed"].sum()), what
    assert st["seeds_rejected"] == int(((ov["score"] == -1) & (ov["endQ"] == 0) & (ov["endT"] == 0)).sum()), what
    return st


@pytest.mark.parametrize("name", xu.FAMILY_NAMES)
def test_planted_family_matches_oracle_whatever_the_tiers_and_hints(name):
    k, groups = xu.family(name)
    built = {}
    ran = all_strided = first_only = 0
    for params, cases in groups:
        if id(cases) not in built:
            pl = xu.planted(cases, k)
            built[id(cases)] = (pl, _engine(k, pl), _oracle(k, pl))
        pl, e, o = built[id(cases)]
        want = o.align_upper(pl[0], pl[1], pl[2], *params, nthreads=8)
        assert len(want[0]) == len(cases)
        if name == "rejected":
            assert (want[2]["score"] == -1).all()
        n_ext = sum(xu.extensions_run(cs, k) for cs in cases)
        for cfg in CONFIGS:
            _configure(e, cfg)
            st = _compare(e, want, params, (name, params, cfg))
            # the hints are not ignored: what they send on arrives.  Skipping the only tier hands every extension that runs to the strided kernel
            if cfg == ALL_STRIDED:
                assert st["extensions_strided"] == n_ext, (name, params, st["extensions_strided"], n_ext)
                all_strided += st["extensions_strided"]
            elif cfg == FIRST_TIER_ONLY:
                assert st["extensions_strided"] <= n_ext
                first_only += st["extensions_strided"]
            elif cfg == (0, 6, 6000) and name == "long" and params[3] >= 60:
                assert st["extensions_strided"] > 0          # the unrelated pair's band is beyond every register tier
        ran += n_ext
    for pl, e, o in built.values():
        e.close()
    assert all_strided == ran and (first_only < ran or ran == 0), (name, ran, all_strided, first_only)
    assert (ran == 0) == (name == "rejected")


def _widths(cases, k, params):
    """widest stored antidiagonal of every extension that runs, from the restatement"""
    return [i.widest for cs in cases for i in xu.restated(cs, k, params)[2] if i.ran]


@pytest.mark.parametrize("t", [1, 2, 4, 8])
def test_ladder_single_tier_keeps_what_fits_and_hands_over_what_does_not(t):
    """aln_tiers = t alone, hints off: the register kernel holds a window of W = 64 t columns that slides by whole lanes (t columns), so an
    antidiagonal of at most W - t + 1 stored columns always fits and one of more than W never does; between them it depends on where the
    band's lower edge falls inside a lane.  extensions_strided is bracketed by the two counts; on the pairs whose extensions all stay out
    of that grey zone both counts are equal, non-zero, and not everything: the tier holds exactly the width it claims."""
    k, groups = xu.family("ladder")
    W = 64 * t
    lo = hi = got = 0
    clear_leave = clear_got = clear_all = 0
    for params, cases in groups:
        grey = [any(W - t + 1 < i.widest <= W for i in xu.restated(cs, k, params)[2] if i.ran) for cs in cases]
        for clear, subset in ((True, [cs for cs, g in zip(cases, grey) if not g]), (False, [cs for cs, g in zip(cases, grey) if g])):
            if not subset:
                continue
            pl = xu.planted(subset, k)
            e, o = _engine(k, pl), _oracle(k, pl)
            _configure(e, (t, -1, BIG))
            st = _compare(e, o.align_upper(pl[0], pl[1], pl[2], *params, nthreads=4), params, ("ladder", params, t))
            e.close()
            w = _widths(subset, k, params)
            a, b = sum(x > W for x in w), sum(x > W - t + 1 for x in w)
            assert a <= st["extensions_strided"] <= b, (t, params, a, st["extensions_strided"], b)
            lo += a; hi += b; got += st["extensions_strided"]
            if clear:
                assert a == b
                clear_leave += a; clear_got += st["extensions_strided"]; clear_all += len(w)
    assert lo <= got <= hi
    assert clear_leave == clear_got and 0 < clear_leave < clear_all, (t, clear_leave, clear_got, clear_all)


@pytest.mark.parametrize("world", [2, 3])
def test_row_shards_align_planted_asymmetric_pairs_like_one_rank(world):
    """The lower-triangle swap: with the reads numbered at random the pairs straddle the ranks, and about half of them are taken from the
    mirrored entry B(j, i), whose two seed positions are exchanged back.  Gathered overlaps == one rank's == the oracle's."""
    import torch
    import dist_sim
    from elba_amd.distributed import DistributedOverlap, HipBackend
    from test_distributed_cpu import _shard
    k, groups = xu.family("asymmetric")
    params, cases = groups[0]
    ids = xu.scattered_ids(len(cases), 77)
    pl = xu.planted(cases, k, ids)
    packed, off, lens, M, N, rows, cols, vals = pl
    o = _oracle(k, pl)
    want = o.align_upper(packed, off, lens, *params, nthreads=8)
    assert sorted(zip(want[0].tolist(), want[1].tolist())) == sorted(ids)
    e = _engine(k, pl)
    _compare(e, want, params, "one rank")
    e.close()
    bounds = np.linspace(0, M, world + 1).astype(np.int64)
    # pairs whose rows live on two ranks, of both parities of i + j: both the upper and the mirrored entry are somebody's to align
    cross = [(a + b) & 1 for a, b in ids if np.searchsorted(bounds, a, side="right") != np.searchsorted(bounds, b, side="right")]
    assert cross.count(0) >= 4 and cross.count(1) >= 4

    def body(rank, h):
        a, b = int(bounds[rank]), int(bounds[rank + 1])
        d = DistributedOverlap(k, 2, 8, device=0, rank=rank, world=world, dist=h, backend=HipBackend(k, 2, 8, 0))
        d.set_reads(*_shard(packed, off, lens, a, b), a, bounds)
        rec = torch.from_numpy(xu.panel_records(rows, cols, vals, a, b)).to(d.be.dev)
        d.be.set_option("panel_inline", 0)
        d.be.set_panel(rec, M, N, a, b)
        d.be.create_seed_matrix()
        st = d.align_seeds(*params)
        g = d.export_overlaps()
        d.be.e.close()
        return st, g

    res = dist_sim.run_ranks(world, body)
    gr = np.concatenate([g["rows"] for _, g in res]); gc = np.concatenate([g["cols"] for _, g in res]); gv = np.concatenate([g["vals"] for _, g in res])
    assert sum(st["nalignments"] for st, _ in res) == len(want[0]) and min(st["nalignments"] for st, _ in res) > 0
    order = np.lexsort((gc, gr))
    assert (gr[order] == want[0]).all() and (gc[order] == want[1]).all()
    for f in want[2].dtype.names:
        if f != "pad":
            assert (gv[order][f] == want[2][f]).all(), f
    assert sum(st["cells"] for st, _ in res) == want[3]


def test_planted_route_equals_the_direct_route_on_real_reads():
    """The guard on the method itself: A built on the device from small_err.fa, exported as triples and handed back through
    set_kmer_matrix, gives the alignments of the direct path (and the oracle's)."""
    packed, off, lens = po.pack_reads(util.read_fasta(os.path.join(util.GOLDEN, "small_err.fa")))
    e, ks, ms, st = gu.gpu_full(packed, off, lens, 17, 2, 8)
    a = e.align_seeds()
    g = e.export_overlaps()
    A = e.export_kmer_matrix()
    e.close()
    o = gu.oracle_run(packed, off, lens, 17, 2, 8)
    want = o.align_upper(packed, off, lens, nthreads=8)
    e2 = elba_amd.Engine(17, 2, 8)
    e2.set_reads(packed, off, lens)
    e2.set_kmer_matrix(A["M"], A["N"], A["csc_read"], np.repeat(np.arange(A["N"], dtype=np.int64), np.diff(A["colptr"])), A["csc_pos"])
    e2.create_seed_matrix()
    b = _compare(e2, want, (1, -1, -1, 15), "triples handed back")
    g2 = e2.export_overlaps()
    e2.close()
    assert a["nalignments"] == b["nalignments"] > 100 and a["cells"] == b["cells"]
    assert (g["rows"] == g2["rows"]).all() and (g["cols"] == g2["cols"]).all()
    assert all((g["vals"][f] == g2["vals"][f]).all() for f in g["vals"].dtype.names if f != "pad")
