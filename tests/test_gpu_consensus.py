"""-m gpu: contig polishing on the GPU (elba_polish_contigs, polish.hip) against the two restatements of consensus_util.py, fed with the
device's own contigs, read flags and placements: polished sequences byte for byte, votes and per-read records entry for entry, counts.
The graphs come from the hand cases (a chain plus reads contained in it), from noisy reads laid on a single-read contig, and from
placement_util's ground-truth layouts with planted errors."""
import ctypes as C

import numpy as np
import pytest

import consensus_util as cs
import contig_ex_util as cx
import contig_util as cu
import elba_amd
import placement_util as pu
from elba_amd import capi

pytestmark = pytest.mark.gpu

INVALID_ARG, STATE = 1, 5                                                    # ELBA_ERR_* of include/elba_amd.h
HAND = cs.hand_cases()


def _load(e, seqs, pairs, cflags):
    e.set_reads(*cu.pack(seqs))
    e.set_overlaps(len(seqs), *pairs)
    e.transitive_reduction(0.0, 0)
    e.generate_contigs(circular=bool(cflags & 1), singletons=bool(cflags & 2))
    return e.export_contigs()


def _check(e, seqs, band=64, max_diff=0.25, min_depth=3, skip=1, loops=True, got=None):
    """The device's polished contigs, votes, records and counts are those of the restatements on the device's own contigs and placements."""
    got = e.export_contigs() if got is None else got
    pl, _ = e.place_reads(skip)
    out, st = e.polish_contigs(skip, band, max_diff, min_depth, votes=True)
    assert out["reads"].dtype == capi.POLISH_READ_DTYPE and st["ms_total"] > 0 and st["ms_align"] >= 0
    cin = cs.inputs_of(seqs, got["seqs"], got["kinds"], pl["reads"], band, max_diff, min_depth)
    for f in ((cs.polish_tables, cs.polish_loops) if loops else (cs.polish_tables,)):
        want, wst = f(cin)
        assert cs.first_difference(out, want) is None, cs.first_difference(out, want)
        assert {k: st[k] for k in cs.STATS} == wst, (st, wst)
    for k in cs.GET_STATS:
        assert e.get_stat("polish_" + k) == st[k]
    plain, st2 = e.polish_contigs(skip, band, max_diff, min_depth)           # without the votes: the same contigs, no vote arrays
    assert plain["seqs"] == out["seqs"] and "col" not in plain and {k: st2[k] for k in cs.STATS} == {k: st[k] for k in cs.STATS}
    return out, st, cin


@pytest.mark.parametrize("case", HAND, ids=[c["name"] for c in HAND])
def test_hand_cases(case):
    seqs, lens, pairs, cflags = cs.pairs_of_case(case)
    e = elba_amd.Engine(17, 2, 8)
    got = _load(e, seqs, pairs, cflags)
    pl, _ = e.place_reads()
    for f in ("start", "contig", "strand", "kind", "flags"):
        assert (pl["reads"][f] == case["cin"]["reads"][f]).all(), f
    cin = case["cin"]
    out, st, _ = _check(e, seqs, cin["band"], cin["max_diff_q16"] / 65536.0, cin["min_depth"], got=got)
    assert cs.check_claims(case, out, st) is None, cs.check_claims(case, out, st)
    e.close()


def _noisy(rng, glen, nreads, lo, hi, lens=None, rate=0.08, jitter=3):
    """One read that is the contig (a single-read contig) and `nreads` noisy reads contained in it, placed with a jitter; returns (seqs,
    pairs, cflags)."""
    genome = cx.random_genome(rng, glen)
    seqs, pairs = [genome], {}
    for x in range(nreads):
        l = int(lens[x]) if lens is not None else int(rng.integers(lo, hi + 1))
        a = int(rng.integers(0, glen - l + 1))
        out = []
        for ch in genome[a:a + l]:
            u = rng.random()
            if u < rate * 0.4:
                out.append("ACGT"[int(rng.integers(0, 4))])
            elif u < rate * 0.7:
                continue
            elif u < rate:
                out += [ch, "ACGT"[int(rng.integers(0, 4))]]
            else:
                out.append(ch)
        s = ("".join(out) + genome[a + l:a + 2 * l] + "ACGT" * l)[:l]          # the read keeps its length
        sx = int(rng.integers(0, 2))
        by = min(max(a + int(rng.integers(-jitter, jitter + 1)), 0), glen - l)
        seqs.append(cu.revcomp(s) if sx else s)
        pairs[(0, 1 + x)] = pu.pair(by, by + l, 0, l, rc=sx, score=l, containedT=1)
    return seqs, cu.upper(pairs), cx.SINGLETONS


@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 128, 129])
def test_rows_around_the_blocks_of_64(n):
    """Reads of n bases: the read bases and contig bytes come in blocks of 64 rows, the walk's LDS blocks hold 64 rows."""
    rng = np.random.default_rng(n)
    seqs, pairs, cflags = _noisy(rng, 400, 12, n, n, rate=0.1 if n > 1 else 0.0)
    e = elba_amd.Engine(17, 2, 8)
    _load(e, seqs, pairs, cflags)
    out, st, _ = _check(e, seqs, 64, 0.4, 2)
    assert st["voted"] + st["rejected"] == 13 and int(out["reads"]["n"][1:].max()) == n
    e.close()


@pytest.mark.parametrize("band", [64, 128, 256])
def test_bands(band):
    rng = np.random.default_rng(band)
    seqs, pairs, cflags = _noisy(rng, 700, 40, 40, 300, rate=0.1, jitter=band // 2 - 6)
    e = elba_amd.Engine(17, 2, 8)
    _load(e, seqs, pairs, cflags)
    out, st, _ = _check(e, seqs, band, 0.3, 3, loops=band == 64)
    assert st["voted"] > 30 and int(out["col"][:, 4].sum()) > 0 and int(out["gap"].sum()) > 0 and st["cells"] == int(out["reads"]["n"].sum()) * band
    e.close()


@pytest.mark.parametrize("nv", [63, 64, 65])
def test_voters_around_one_wavefront(nv):
    rng = np.random.default_rng(nv)
    seqs, pairs, cflags = _noisy(rng, 300, nv - 1, 40, 90)
    e = elba_amd.Engine(17, 2, 8)
    _load(e, seqs, pairs, cflags)
    out, st, _ = _check(e, seqs, 64, 1.0, 3, loops=False)
    assert st["voted"] == nv
    e.close()


def test_contig_kinds_under_flags_0_to_3():
    """A ring of 6 reads, a path of 3 and 4 lone reads, with contained reads on each (placement's own test graph, with real sequences): under
    every combination of the contig flags the device polishes the contigs that call made."""
    rng = np.random.default_rng(11)
    ringg, pathg = cs._genome(21, 120), cs._genome(22, 90)
    rr = ringg * 3
    seqs = [rr[20 * i:20 * i + 40] for i in range(6)]
    strands = [0, 1, 0, 0, 1, 0]
    seqs = [cu.revcomp(s) if st else s for s, st in zip(seqs, strands)]
    pst = [1, 0, 0]
    seqs += [cu.revcomp(pathg[0:40]), pathg[25:65], pathg[50:90]]
    lone = [cx.random_genome(rng, 30) for _ in range(4)]
    seqs += lone
    ring = [(i, 20, strands[i]) for i in range(6)]
    path = [(6, 25, pst[0]), (7, 25, pst[1]), (8, 40, pst[2])]
    lens = [len(s) for s in seqs] + [12] * 4
    pairs = dict(pu.edges_of_chains(lens, [ring, path], [cx.CIRCLE, cx.PATH]))
    sub = lambda s, i: s[:i] + cs._other(s[i]) + s[i + 1:]
    seqs.append(sub(pu.oriented(seqs[1], 1)[5:17], 4)); pairs[(1, 13)] = pu.pair(40 - 17, 40 - 5, 0, 12, rc=1, score=12, containedT=1)
    seqs.append(pu.oriented(seqs[5], 0)[15:27]); pairs[(5, 14)] = pu.pair(15, 27, 0, 12, score=12, containedT=1)
    seqs.append(sub(seqs[7][0:12], 6)); pairs[(7, 15)] = pu.pair(0, 12, 0, 12, score=12, containedT=1)
    seqs.append(cu.revcomp(lone[1][3:15])); pairs[(10, 16)] = pu.pair(3, 15, 0, 12, rc=1, score=12, containedT=1)
    pairs = cu.upper(pairs)
    e = elba_amd.Engine(17, 2, 8)
    for cflags in (0, 1, 2, 3):
        got = _load(e, seqs, pairs, cflags)
        out, st, _ = _check(e, seqs, 64, 0.25, 1, got=got)
        assert got["n"] == {0: 1, 1: 2, 2: 5, 3: 6}[cflags] and st["voted"] == {0: 4, 1: 12, 2: 9, 3: 17}[cflags]
    e.close()


def test_batches_do_not_change_the_result():
    """A polish_trace_bytes so small that the call takes many batches and the longest read a batch of its own."""
    rng = np.random.default_rng(5)
    lens = [60] * 20 + [300] + [50] * 20
    seqs, pairs, cflags = _noisy(rng, 500, len(lens), 0, 0, lens=lens)
    e = elba_amd.Engine(17, 2, 8)
    _load(e, seqs, pairs, cflags)
    one, st1, _ = _check(e, seqs, 64, 0.3, 3, loops=False)
    assert st1["batches"] == 1
    e.set_option("polish_trace_bytes", 200 * 16)                              # 200 rows of 16 bytes: three reads of 60, four of 50, never the one of 300
    many, st2 = e.polish_contigs(1, 64, 0.3, 3, votes=True)
    assert st2["batches"] >= 3 and st2["batches"] == e.get_stat("polish_batches") and cs.first_difference(one, many) is None
    assert {k: st1[k] for k in cs.STATS} == {k: st2[k] for k in cs.STATS}
    e.set_option("polish_trace_bytes", 1)                                     # every voter alone
    each, st3 = e.polish_contigs(1, 64, 0.3, 3, votes=True)
    assert st3["batches"] == st1["voted"] + st1["rejected"] and cs.first_difference(one, each) is None
    e.set_option("polish_trace_bytes", 0)
    with pytest.raises(elba_amd.ElbaError):
        e.set_option("polish_trace_bytes", -1)
    e.close()


def _truth(e, seed, glen, nchain, circular, ncont, nextra, nerr):
    t = pu.truth_set(np.random.default_rng(seed), glen, nchain, circular, ncont, nextra)
    seqs, sites = cs.mutate_truth(t, np.random.default_rng(seed + 1000), nerr)
    e.set_reads(*cu.pack(seqs))
    e.set_overlaps(len(seqs), *t["pairs"])
    return t, seqs, sites


def test_one_context_over_changing_sizes_repeats_and_changes_nothing():
    """Three sets on one context; on each three identical calls, and place_reads, export_pileup and export_contigs the same before and
    after; planted errors of about 1 % come back as the genome where the unpolished contig differs from it."""
    e = elba_amd.Engine(17, 2, 8)
    for seed, glen, nchain, circular, ncont, nextra, nerr in ((1, 900, 12, False, 60, 6, 12), (2, 1200, 9, True, 80, 8, 14), (7, 600, 6, False, 45, 3, 8)):
        t, seqs, sites = _truth(e, seed, glen, nchain, circular, ncont, nextra, nerr)
        e.read_pileup(mode=0, margin=0, min_depth=1, min_run=1, trim_len=0)
        e.transitive_reduction(0.0, 0)
        e.generate_contigs(circular=True)
        pile, contigs, (pl, pst) = e.export_pileup(), e.export_contigs(), e.place_reads()
        out, st, _ = _check(e, seqs, loops=glen <= 900)
        assert contigs["n"] == 1 and not cs.same_sequence(contigs["seqs"][0], t["genome"], circular)
        assert cs.same_sequence(out["seqs"][0], t["genome"], circular) and st["rejected"] == 0
        for _ in range(2):
            again, st2 = e.polish_contigs(votes=True)
            assert cs.first_difference(out, again) is None and {k: st2[k] for k in cs.STATS} == {k: st[k] for k in cs.STATS}
        pile2, contigs2, (pl2, pst2) = e.export_pileup(), e.export_contigs(), e.place_reads()
        assert all(np.array_equal(pile[k], pile2[k]) for k in pile if k != "n") and pile["n"] == pile2["n"]
        assert contigs["seqs"] == contigs2["seqs"] and all(np.array_equal(contigs[k], contigs2[k]) for k in contigs if k not in ("seqs", "n"))
        assert pu.same_placements(pl, pl2) and {k: pst[k] for k in pu.STATS} == {k: pst2[k] for k in pu.STATS}
        for k in pu.GET_STATS:
            assert e.get_stat("place_" + k) == pst2[k]
        e.release_workspace()
        again, _ = e.polish_contigs(votes=True)
        assert cs.first_difference(out, again) is None
    e.close()


def test_errors():
    e = elba_amd.Engine(17, 2, 8)
    case = next(c for c in HAND if c["name"] == "left-deletes-a-column")
    seqs, lens, pairs, cflags = cs.pairs_of_case(case)
    e.set_reads(*cu.pack(seqs))
    e.set_overlaps(len(seqs), *pairs)
    e.transitive_reduction(0.0, 0)
    with pytest.raises(elba_amd.ElbaError) as err:               # no contigs yet
        e.polish_contigs()
    assert err.value.status == STATE and e.get_stat("polish_voted") == 0
    e.generate_contigs(singletons=True)
    out, st = e.polish_contigs(min_depth=3)
    assert out["seqs"] == [case["seq"]] and e.get_stat("polish_voted") == 4 == st["voted"]
    for bad in (dict(band=32), dict(band=96), dict(band=512), dict(max_diff_q16=-1), dict(max_diff_q16=65537), dict(min_depth=0), dict(flags=2), dict(flags=3),
                dict(reserved=(1, 0, 0)), dict(reserved=(0, 0, 7)), dict(skip_flags=256), dict(skip_flags=-1)):
        with pytest.raises(elba_amd.ElbaError) as err:
            e.polish_contigs(**bad)
        assert err.value.status == INVALID_ARG and e.get_stat("polish_voted") == 0, bad      # nothing of the failed call is left
        e.polish_contigs()
        assert e.get_stat("polish_voted") == 4
    e.polish_contigs(max_diff_q16=65536); e.polish_contigs(max_diff_q16=0)
    o, s = capi.Polished(), capi.PolishStats()
    o.n, o.seq = 7, 8                                            # (stale values: the call zeroes them)
    assert e.L.elba_polish_contigs(e.h, None, C.byref(o), C.byref(s)) == INVALID_ARG and not o.seq and o.n == 0
    assert e.L.elba_polish_contigs(e.h, C.byref(capi.PolishCfg(1, 64, 16384, 3, 0)), None, C.byref(s)) == INVALID_ARG
    e.polish_contigs()
    assert e.get_stat("place_chain") == 0                        # no place_reads call yet on these contigs: its counts are its own
    e.clip_tips(2, 1)                                            # the contigs are gone: the counts read 0, the call is out of order
    assert e.get_stat("polish_voted") == 0 and e.get_stat("polish_cells") == 0
    with pytest.raises(elba_amd.ElbaError) as err:
        e.polish_contigs()
    assert err.value.status == STATE
    with pytest.raises(elba_amd.ElbaError):
        e.get_stat("polish_nothing")
    e.close()
