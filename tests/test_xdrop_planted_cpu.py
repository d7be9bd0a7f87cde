"""CPU: the planted-seed x-drop families (tests/xdrop_util.py) — the Python restatement of the reference's XDropAligner.cpp / Overlap.cpp, the
C oracle per pair (pyoracle.xdrop) and the C oracle through planted triples (Oracle.set_triples -> spgemm -> align_upper) must agree field
for field, cells included; every family must do what its name says, by the restatement's own account; and the oracle must return what the
reference's own build returned (tests/golden/xdrop_planted_k*.txt, recomputed live where oracle/_ref is built).

Left out of the Python restatement: the family "long" (reads of 70 000 ... 100 000 bases).  It is covered oracle-against-reference."""
import os

import numpy as np
import pytest

import util
import xdrop_util as xu
from oracle import pyoracle as po

G = util.GOLDEN


def _oracle_groups(name):
    k, groups = xu.family(name)
    for params, cases in groups:
        packed, off, lens, M, N, rows, cols, vals = xu.planted(cases, k)
        o = po.Oracle(k, 2, 8)
        o.set_triples(M, N, rows, cols, vals)
        o.spgemm(1)
        r, c, ov, cells = o.align_upper(packed, off, lens, *params, nthreads=4)
        yield k, params, cases, (packed, off, lens), (r, c, ov, cells)


@pytest.mark.parametrize("name", [n for n in xu.FAMILY_NAMES if n not in xu.PYTHON_SKIPS])
def test_restatement_oracle_and_planted_route_agree(name):
    for k, params, cases, (packed, off, lens), (r, c, ov, cells) in _oracle_groups(name):
        p2, o2, l2 = po.pack_reads([s for cs in cases for s in (cs.q, cs.t)])               # the generator's packer against the oracle's encoder
        assert (off == o2).all() and (lens == l2).all() and (packed[:len(p2) - 8] == p2[:len(p2) - 8]).all() and len(packed) >= len(p2) + 8
        assert len(r) == len(cases) and (r == 2 * np.arange(len(cases))).all() and (c == r + 1).all()
        total = 0
        for i, cs in enumerate(cases):
            want, ret, infos = xu.restated(cs, k, params)
            total += infos[0].cells + infos[1].cells
            assert xu.extensions_run(cs, k) == infos[0].ran + infos[1].ran, cs.name
            one = po.xdrop(packed[int(off[2 * i]):], len(cs.q), packed[int(off[2 * i + 1]):], len(cs.t), cs.q0, cs.t0, k, *params)
            assert one == (ret, want["begQ"], want["endQ"], want["begT"], want["endT"], want["score"], want["rc"], want["kind"]), (name, cs.name, params, one, want)
            for f in xu.OVERLAP_FIELDS:
                assert int(ov[i][f]) == want[f], (name, cs.name, params, f, ov[i], want)
        assert total == cells, (name, params, total, cells)


def _all(name):
    k, groups = xu.family(name)
    for params, cases in groups:
        for cs in cases:
            yield k, params, cs, xu.restated(cs, k, params)


def test_rejected_family_is_rejected():
    n = 0
    for k, params, cs, (o, ret, infos) in _all("rejected"):
        assert ret == -1 and o["score"] == -1 and (o["begQ"], o["endQ"], o["begT"], o["endT"], o["passed"]) == (0, 0, 0, 0, 0), cs.name
        assert not infos[0].ran and not infos[1].ran
        over = max(cs.q0 + k - len(cs.q), cs.t0 + k - len(cs.t), -cs.q0, -cs.t0)
        assert over <= k, (cs.name, over)                       # no planted position overshoots its read by more than k bases
        n += 1
    assert n >= 60


def test_edges_family_has_every_degenerate_geometry():
    seen = set()
    one_base = 0
    for k, params, cs, (o, ret, infos) in _all("edges"):
        if ret == -1:
            # only the pair with a read shorter than k, and corner seeds whose reverse-complement image is (0, 0)
            assert min(len(cs.q), len(cs.t)) < k or (cs.q0, cs.t0) == (0, 0), cs.name
            seen.add("short" if min(len(cs.q), len(cs.t)) < k else "zero-zero")
            continue
        seen.add((infos[0].ran, infos[1].ran))
        one_base += any(i.ran and i.ads == 1 for i in infos)
        if len(cs.q) == k or len(cs.t) == k:
            seen.add("length-k")
        if len(cs.q) == k + 1 or len(cs.t) == k + 1:
            seen.add("length-k+1")
    assert {(False, False), (False, True), (True, False), (True, True), "short", "zero-zero", "length-k", "length-k+1"} <= seen, seen
    assert one_base > 0


def test_ratio_family_is_moved_by_the_clamps():
    """At the x-drop that never trims, the band of a 1 : 100 pair is the whole rectangle: its width is bounded by the short read and its
    antidiagonals by the long one, which only the row / column clamps can produce."""
    hit = 0
    for k, params, cs, (o, ret, infos) in _all("ratio"):
        assert ret != -1 and max(len(cs.q), len(cs.t)) >= 100 * min(len(cs.q), len(cs.t)) * 0.95, cs.name
        if params[3] >= 20000:
            for i in infos:
                short = min(len(cs.q), len(cs.t))
                if i.ran and i.ads > 20 * short:
                    assert i.widest <= short + 2
                    hit += 1
    assert hit >= 8


def test_tie_families_have_ties():
    for k, params, cs, (o, ret, infos) in _all("ties"):
        assert ret != -1, cs.name
    by_case = {}
    for k, params, cs, (o, ret, infos) in _all("ties"):
        by_case[cs.name] = max(by_case.get(cs.name, 0), infos[0].max_beats, infos[1].max_beats)
    k, groups = xu.family("ties")
    ends = [cs for cs in groups[0][1] if cs.notes.get("tied_end")]
    assert len(ends) >= 16 and all(max(i.last_beats for i in xu.restated(cs, k, xu.P_DEFAULT)[2]) >= 2 for cs in ends)      # the end itself is a tie
    claimed = [cs.name for cs in groups[0][1] if cs.notes["ties"]]
    assert len(claimed) >= 24 and all(by_case[n] >= 2 for n in claimed), {n: by_case[n] for n in claimed if by_case[n] < 2}


def test_indel_family_stops_at_the_indel_or_spans_it():
    n = 0
    for k, params, cs, (o, ret, infos) in _all("indel"):
        size, x = cs.notes["indel"], params[3]
        lq, lt = len(cs.q), len(cs.t)
        sw = cs.notes.get("swapped", False)
        assert ret != -1
        short_len = min(lq, lt)
        # the read WITHOUT the insertion, in its own coordinates: aligned up to the indel, or to its end
        beg, end = (o["begT"], o["endT"]) if sw else (o["begQ"], o["endQ"])
        if sw and o["rc"]:
            beg, end = short_len - end, short_len - beg
        at = cs.notes["at"]
        if params[:3] != xu.INDEL_SCORES:
            continue
        if x >= xu.indel_bridge_x(size):
            assert (beg, end) == (0, short_len), (cs.name, params, beg, end)
            assert abs((o["endT"] - o["begT"]) - (o["endQ"] - o["begQ"])) == size
            n += 1
        elif x < 2 * size:
            if cs.notes["side"] == "right":
                assert beg == 0 and abs(end - at) <= x, (cs.name, params, beg, end, at)
            else:
                assert end == short_len and abs(beg - at) <= x, (cs.name, params, beg, end, at)
            n += 1
    assert n >= 2 * 24


def test_ladder_rungs_are_exact():
    k, groups = xu.family("ladder")
    rungs = []
    for params, cases in groups:
        for cs in cases:
            o, ret, infos = xu.restated(cs, k, params)
            assert max(infos[0].widest, infos[1].widest) == cs.notes["rung"], (cs.name, params, infos[0].widest, infos[1].widest)
            rungs.append(cs.notes["rung"])
    assert xu.LADDER_RUNGS == (63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513) and sorted(rungs) == sorted(4 * (xu.LADDER_RUNGS + xu.LADDER_CLEAR))          # every rung as written, /rc, /swap, /swap+rc


def test_score_family_meets_the_clamp_and_the_whole_rectangle():
    clamped, whole, undef_start = 0, 0, 0
    for k, params, cs, (o, ret, infos) in _all("scores"):
        if params in xu.SCORE_CLAMP_PARAMS:
            clamped += any(i.clamped for i in infos)
        if params[3] >= 1 << 30:
            for i, left in zip(infos, (True, False)):
                if i.ran:
                    lq = cs.q0 if left else len(cs.q) - cs.q0 - k
                    lt = (len(cs.t) - cs.t0 - k if left else cs.t0) if o["rc"] else (cs.t0 if left else len(cs.t) - cs.t0 - k)
                    assert i.cells == lq * lt, (cs.name, i.cells, lq, lt)          # every cell the reference's loop bounds allow
                    whole += i.widest > 512
        if -params[2] > params[3]:
            undef_start += 1
    assert clamped >= 5 * 20 and whole >= 8 and undef_start > 0
    # the clamp decides results: the same recurrence without it (unbounded integers) aligns some of these pairs differently
    k, groups = xu.family("scores")
    cases = groups[0][1]
    differ = sum(xu.extend_overlap(cs.q, cs.t, cs.q0, cs.t0, k, *p, clamp=False)[0] != xu.restated(cs, k, p)[0] for p in xu.SCORE_CLAMP_PARAMS for cs in cases)
    assert differ >= 4, differ


def test_hint_family_straddles_the_default_hint():
    k, groups = xu.family("hint")
    ns = sorted({cs.numshared for cs in groups[0][1]})
    assert ns == [2, 6, 7, 20]                                   # aln_wide_hint's default is 6 (elba_amd/csrc/common.hpp)
    wide = [max(i.widest for i in xu.restated(cs, k, p)[2]) for p, cases in groups for cs in cases]
    assert min(wide) <= 64 and max(wide) > 512


def test_asymmetric_family_cannot_hide_a_missed_swap():
    n = far = 0
    for k, params, cs, (o, ret, infos) in _all("asymmetric"):
        assert ret != -1 and cs.q0 != cs.t0 and abs(len(cs.q) - len(cs.t)) > 50, cs.name
        far += abs(cs.q0 - cs.t0) > 500
        if not o["rc"]:          # (a reverse-complement pair lies on q + t = const: its exchanged seed is another seed of the same alignment)
            swapped = xu.extend_overlap(cs.q, cs.t, cs.t0, cs.q0, k, *params)[0]
            assert swapped != o, cs.name
            n += 1
    assert n >= 48 and far >= n


def _vectors(k):
    rows = []
    for line in open(os.path.join(G, "xdrop_planted_k%d.txt" % k)):
        if line[0] != "#":
            w = line.split()
            rows.append((w[0], w[1], [int(x) for x in w[2:8]], int(w[8], 16), [int(x) for x in w[9:]]))
    return rows


@pytest.mark.parametrize("k", [17, 31, 33, 63, 95])
def test_oracle_matches_reference_vectors_on_planted_families(k):
    """Every family of this k, the long reads included: what the reference's xdrop_aligner + classify_alignment returned
    (tests/golden/make_golden.py planted) against the oracle; where oracle/_ref is built the reference is asked again."""
    R = po.ref_lib(k)
    live = R is not None and hasattr(R, "ref_xdrop")
    vec = _vectors(k)
    at = 0
    for name in xu.FAMILY_NAMES:
        fk, groups = xu.family(name)
        if fk != k:
            continue
        for params, cases in groups:
            packed, off, lens = xu.pack_ascii([s for cs in cases for s in (cs.q, cs.t)])
            for i, cs in enumerate(cases):
                fam, cname, inp, crc, want = vec[at]
                at += 1
                assert (fam, cname, inp, crc) == (name, cs.name, [cs.q0, cs.t0] + list(params), xu.case_crc(cs)), (fam, cname, name, cs.name)
                got = po.xdrop(packed[int(off[2 * i]):], len(cs.q), packed[int(off[2 * i + 1]):], len(cs.t), cs.q0, cs.t0, k, *params)
                assert list(got) == want, (name, cs.name, params, got, want)
                if live:
                    ref = po.ref_xdrop(R, packed[int(off[2 * i]):], len(cs.q), packed[int(off[2 * i + 1]):], len(cs.t), cs.q0, cs.t0, *params)
                    assert got == ref, (name, cs.name, params, got, ref)
    assert at == len(vec) and at >= (1400 if k == 17 else 72)
