"""CPU: the placement rule (elba_place_reads, include/elba_amd.h) as placement_util.py restates it — the hand cases' claims, the two
restatements against each other under shuffled visiting orders, the ground-truth sets (every placed read reads the same as the contig where
it lies), the identities between depth and credits, the PAF writer and the GFA depth tag.  No device."""
import ctypes
import os

import numpy as np
import pytest

import contig_ex_util as cx
import contig_util as cu
import elba_amd
import placement_util as pu
from elba_amd import capi, formats

HAND = pu.hand_cases()


def _both(inp):
    a, sa = pu.place_loops(inp)
    b, sb = pu.place_tables(inp)
    assert sa == sb, (sa, sb)
    assert pu.same_placements(a, b), pu.first_difference(a, b)
    return a, sa


@pytest.mark.parametrize("case", HAND, ids=[c["name"] for c in HAND])
def test_hand_cases_hold_their_claims_in_both_restatements(case):
    pl, st = _both(case["inp"])
    for r, want in case["reads"].items():
        p = pl["reads"][r]
        got = (int(p["contig"]), int(p["start"]), int(p["strand"]), int(p["kind"]), int(p["flags"]), int(p["anchor"]))
        assert got == tuple(want), (r, got, want)
    for k, v in case["stats"].items():
        assert st[k] == v, (k, st[k], v)
    L = pu.contig_lens(case["inp"])
    for c, d in case["depth"].items():
        assert pu.depth_of(pl, c, int(L[c])).tolist() == list(d)
    for c, (nr, nb) in case["credited"].items():
        assert (int(pl["credited_reads"][c]), int(pl["credited_bases"][c])) == (nr, nb)
    assert st["chain"] + st["anchored"] + st["unanchored"] + st["skipped"] + st["empty"] == st["nreads"]


@pytest.mark.parametrize("case", HAND, ids=[c["name"] for c in HAND])
def test_hand_case_graphs_give_their_chains(case):
    """edges_of_chains builds a string graph whose contigs are the case's chains (what the GPU tests load)."""
    inp = case["inp"]
    kinds = [int(k) for k in inp["kinds"]]
    edges = pu.edges_of_chains(inp["lens"], case["chains"], kinds)
    seqs = ["A" * int(l) for l in inp["lens"]]
    _, chains, got_kinds, _, _ = cx.generate_contigs_ex(inp["M"], *cu.symmetric(edges), seqs, case["cflags"], inp["read_flags"])
    assert chains == case["chains"] and got_kinds == kinds


def _truth(seed, glen, nchain, circular, ncont, nextra):
    rng = np.random.default_rng(seed)
    t = pu.truth_set(rng, glen, nchain, circular, ncont, nextra)
    M = len(t["lens"])
    contigs, chains, kinds, read_contig, _ = cx.generate_contigs_ex(M, *cu.symmetric(t["edges"]), t["seqs"], cx.CIRCULAR, t["read_flags"])
    inp = pu.inputs_of_chains(t["lens"], chains, kinds, *t["pairs"], t["read_flags"], 1)
    return t, contigs, chains, kinds, inp


TRUTH = [(1, 900, 12, False, 15, 6), (2, 1200, 9, True, 20, 8), (3, 700, 5, False, 0, 0), (4, 2000, 30, True, 40, 10), (5, 1500, 20, False, 30, 12)]


@pytest.mark.parametrize("seed,glen,nchain,circular,ncont,nextra", TRUTH)
def test_ground_truth_reads_read_like_their_contig(seed, glen, nchain, circular, ncont, nextra):
    t, contigs, chains, kinds, inp = _truth(seed, glen, nchain, circular, ncont, nextra)
    assert len(contigs) == 1 and kinds == [cx.CIRCLE if circular else cx.PATH] and len(contigs[0]) == glen
    pl, st = _both(inp)
    assert st["chain"] == nchain and st["anchored"] == ncont + nextra and st["unanchored"] == 0 and st["skipped"] == 0     # every extra read overlaps a chain read
    contig, L = contigs[0], glen
    for r, p in enumerate(pl["reads"]):
        assert int(p["kind"]) != pu.NONE and int(p["contig"]) == 0
        s, start, l = pu.oriented(t["seqs"][r], int(p["strand"])), int(p["start"]), t["lens"][r]
        if circular:
            assert l <= L and s == (contig * 3)[start % L:start % L + l], r
            assert bool(int(p["flags"]) & pu.WRAPPED) == (start % L + l > L)
        else:
            assert 0 <= start and start + l <= L and int(p["flags"]) == 0 and s == contig[start:start + l], r
    d = pu.depth_of(pl, 0, L)
    assert len(d) == L and (d >= 1).all()                        # chain reads tile the contig
    chain_only = pu.place_tables(dict(inp, rows=inp["rows"][:0], cols=inp["cols"][:0], vals=inp["vals"][:0]))[0]
    assert (pu.depth_of(chain_only, 0, L) >= 1).all()
    if not circular:                                             # the true starts: the layout's, mirrored when the walk ran against it
        walk_forward = chains[0][0][0] == t["chain_ids"][0]
        for r, p in enumerate(pl["reads"]):
            a, b, _ = t["where"][r]
            assert int(p["start"]) == (a if walk_forward else L - b), r


@pytest.mark.parametrize("seed,glen,nchain,circular,ncont,nextra", TRUTH)
def test_credits_are_the_area_under_the_depth(seed, glen, nchain, circular, ncont, nextra):
    t, contigs, chains, kinds, inp = _truth(seed, glen, nchain, circular, ncont, nextra)
    pl, st = _both(inp)
    for c, contig in enumerate(contigs):
        a, b = int(pl["seg_off"][c]), int(pl["seg_off"][c + 1])
        ends = np.concatenate([pl["seg_start"][a + 1:b], [len(contig)]]).astype(np.int64)
        assert int(((ends - pl["seg_start"][a:b]) * pl["seg_depth"][a:b]).sum()) == int(pl["credited_bases"][c])
        assert pl["seg_start"][a] == 0 and (np.diff(pl["seg_depth"][a:b]) != 0).all()      # maximal runs from 0
    assert st["credited_bases"] == int(pl["credited_bases"].sum()) and st["max_depth"] == int(pl["seg_depth"].max())


@pytest.mark.parametrize("seed", range(6))
def test_the_two_forms_agree_under_shuffled_visiting_orders(seed):
    """Random chains, random pairs (valid intervals, any score, passed or not, both sides), random flags: the loops in three visiting
    orders and the tables give the same records, segments and counts."""
    rng = np.random.default_rng(100 + seed)
    M = 60
    lens = rng.integers(0, 50, M)
    lens[rng.integers(0, M, 3)] = 0
    ids = rng.permutation(M)
    chains, kinds, at = [], [], 0
    for n, kd in ((6, cx.PATH), (5, cx.CIRCLE), (1, cx.SINGLE), (3, cx.PATH), (1, cx.SINGLE)):
        ch = [(int(r), int(rng.integers(0, lens[r] + 1)), int(rng.integers(0, 2))) for r in ids[at:at + n]]
        at += n
        chains.append(ch); kinds.append(kd)
    pairs = {}
    for _ in range(300):
        q, t = sorted(int(x) for x in rng.integers(0, M, 2))
        if q == t:
            continue
        bq, eq = sorted(int(x) for x in rng.integers(0, lens[q] + 1, 2)); bt, et = sorted(int(x) for x in rng.integers(0, lens[t] + 1, 2))
        pairs[(q, t)] = pu.pair(bq, eq, bt, et, rc=int(rng.integers(0, 2)), score=int(rng.integers(-3, 4)), passed=int(rng.random() < 0.8))
    rows, cols, vals = cu.upper(pairs)
    flags = (rng.random(M) < 0.2) * rng.integers(1, 64, M)
    for skip in (0, 1, 255):
        inp = pu.inputs_of_chains(lens, chains, kinds, rows, cols, vals, flags, skip)
        want, wst = _both(inp)
        for _ in range(3):
            got, st = pu.place_loops(inp, rng.permutation(len(rows)), rng.permutation(M))
            assert st == wst and pu.same_placements(got, want), pu.first_difference(got, want)
        assert wst["chain"] == 16 and wst["chain"] + wst["anchored"] + wst["unanchored"] + wst["skipped"] + wst["empty"] == M
    assert wst["skipped"] > 0 and wst["empty"] > 0


def test_a_bad_interval_is_named_only_when_it_is_a_candidate():
    case = next(c for c in HAND if c["name"] == "ties")
    inp = dict(case["inp"])                                      # list order: (0, 3) chain-chain, (0, 4), (1, 4), (1, 5), (2, 4), (2, 5), (3, 6) not passed, (6, 7) off-off
    for a, field, value, named in ((1, "endQ", 51, True), (2, "begT", -1, True), (3, "begT", 21, True), (0, "endQ", 99, False), (6, "begQ", -5, False), (7, "endT", 1000, False)):
        vals = inp["vals"].copy()
        vals[field][a] = value
        if named:
            vals["endT"][5] = 21                                 # a second bad candidate behind it: the smallest index is named
        bad = dict(inp, vals=vals)
        if not named:
            assert pu.place_loops(bad)[1] == pu.place_tables(bad)[1]
            continue
        for f in (pu.place_loops, pu.place_tables):
            with pytest.raises(pu.BadInterval) as e:
                f(bad)
            assert e.value.pair == a


def test_paf_round_trip(tmp_path):
    t, contigs, chains, kinds, inp = _truth(2, 1200, 9, True, 20, 8)
    pl, _ = _both(inp)
    names = ["read%d" % i for i in range(inp["M"])]
    path = str(tmp_path / "p.paf")
    formats.write_placements_paf(path, pl, names, t["lens"], [len(c) for c in contigs], kinds)
    recs = pu.parse_paf(path)
    placed = [r for r in range(inp["M"]) if int(pl["reads"][r]["kind"])]
    assert [x["qname"] for x in recs] == [names[r] for r in placed]
    contig = contigs[0]
    for x, r in zip(recs, placed):
        p = pl["reads"][r]
        assert x["qlen"] == t["lens"][r] and x["tname"] == "contig0" and x["tlen"] == len(contig) and x["mapq"] == 255 and x["score"] == int(p["score"])
        assert x["strand"] == "+-"[int(p["strand"])] and x["tbeg"] == int(p["start"]) % len(contig) and x["block"] == x["tend"] - x["tbeg"] == x["qend"] - x["qbeg"]
        assert pu.oriented(t["seqs"][r][x["qbeg"]:x["qend"]], int(p["strand"])) == (contig * 2)[x["tbeg"]:x["tend"]]
    # the clipped intervals of the hand case, in forward read coordinates
    case = next(c for c in HAND if c["name"] == "clip-path")
    pl, _ = _both(case["inp"])
    formats.write_placements_paf(path, pl["reads"], ["r%d" % i for i in range(7)], case["inp"]["lens"], [50])
    got = {x["qname"]: (x["qbeg"], x["qend"], x["tbeg"], x["tend"]) for x in pu.parse_paf(path)}
    assert got == {"r0": (0, 30, 0, 30), "r1": (0, 30, 20, 50), "r2": (5, 20, 0, 15), "r3": (0, 10, 40, 50), "r4": (0, 0, 50, 50), "r5": (10, 10, 0, 0), "r6": (20, 70, 0, 50)}
    p = np.zeros(1, pu.PLACEMENT)[0]
    p["start"], p["strand"], p["kind"] = -5, 1, 2
    assert formats.placement_interval(p, 20, 50, False) == (0, 15, 0, 15)       # reversed: the cut bases are the read's last five
    with pytest.raises(ValueError):
        formats.write_placements_paf(path, pl, ["x"], [1], [50])
    circle = next(c for c in HAND if c["name"] == "circle")      # a wrapped record says its contig is circular: without kinds it is refused
    cpl, _ = _both(circle["inp"])
    with pytest.raises(ValueError, match="wrapped"):
        formats.write_placements_paf(path, cpl, ["r%d" % i for i in range(6)], circle["inp"]["lens"], [100])
    formats.write_placements_paf(path, cpl, ["r%d" % i for i in range(6)], circle["inp"]["lens"], [100], [1])
    got = {x["qname"]: (x["qbeg"], x["qend"], x["tbeg"], x["tend"]) for x in pu.parse_paf(path)}
    assert got["r3"] == (0, 40, 75, 115) and got["r4"] == (0, 30, 90, 120) and got["r5"] == (0, 100, 75, 175) and got["r0"] == (0, 40, 0, 40)


def test_write_gfa_is_byte_identical_without_depth_and_tags_with_it(tmp_path):
    seqs, kinds = ["ACGTACGTAC", "GGG", ""], [0, 2, 0]
    links = np.zeros(1, dtype=capi.LINK_DTYPE)
    links[0] = (0, 1, 4, 9, 2, 0, 1, 0, 0)
    a, b, c = (str(tmp_path / n) for n in ("a.gfa", "b.gfa", "c.gfa"))
    formats.write_gfa(a, seqs, kinds, links, chains=[0, 3, 4, 4])
    formats.write_gfa(b, seqs, kinds, links, chains=[0, 3, 4, 4], depth=None)
    want = b"H\tVN:Z:1.0\nS\tcontig0\tACGTACGTAC\tLN:i:10\tRC:i:3\nS\tcontig1\tGGG\tLN:i:3\tRC:i:1\nS\tcontig2\t\tLN:i:0\tRC:i:0\nL\tcontig0\t+\tcontig1\t-\t2M\n"
    assert open(a, "rb").read() == open(b, "rb").read() == want
    formats.write_gfa(c, seqs, kinds, links, chains=[0, 3, 4, 4], depth=[25, 4, 0])
    lines = open(c, "rb").read().split(b"\n")
    assert lines[1].endswith(b"\tRC:i:3\tDP:f:2.50") and lines[2].endswith(b"\tDP:f:1.33") and lines[3].endswith(b"\tDP:f:0.00") and lines[4] == want.split(b"\n")[4]
    formats.write_gfa(c, seqs, kinds, links, depth=[25, 4, 0])
    assert open(c, "rb").read().split(b"\n")[1] == b"S\tcontig0\tACGTACGTAC\tLN:i:10\tDP:f:2.50"
    with pytest.raises(ValueError):
        formats.write_gfa(c, seqs, kinds, links, depth=[1, 2])


def test_the_library_exports_the_entry_points_and_the_abi_version_stays():
    L = ctypes.CDLL(elba_amd.lib_path())
    for name in ("elba_place_reads", "elba_free_placements"):
        assert hasattr(L, name) and name in capi.EXPORTED_SYMBOLS
    L.elba_abi_version.restype = ctypes.c_int
    assert L.elba_abi_version() == 3
    assert capi.PLACEMENT_DTYPE == pu.PLACEMENT and capi.PLACEMENT_DTYPE.itemsize == 24 and ctypes.sizeof(capi.PlaceCfg) == 16
    assert ctypes.sizeof(capi.PlaceStats) == 13 * 8 + 8 and ctypes.sizeof(capi.Placements) == 8 * 8
    assert [f[0] for f in capi.PlaceStats._fields_][:13] == list(pu.STATS) and hasattr(elba_amd.Engine, "place_reads")
    header = open(os.path.join(os.path.dirname(elba_amd.lib_path()), "..", "..", "include", "elba_amd.h")).read()
    for word in ("elba_place_cfg", "elba_placement_t", "elba_placements_t", "elba_place_stats", "elba_place_reads", "elba_free_placements"):
        assert word in header
