"""The inputs of trip_cases.py without a device.  With one CU's thresholds (a trip of 4096 pairs, of 2048 lines) the literal restatements
are affordable: place_loops against place_tables, links_walk against links_tables, index_loop against index_numpy, each on the
builders' output and against what the builders claim.  With 256 CUs' thresholds, the size the GPU tests run at, the builders meet their
own conditions and the vectorised restatements finish in seconds."""
import time

import numpy as np
import pytest

import contig_util as cu
import gfa_util as gu
import placement_util as pu
import text_index_util as tx
import trip_cases as tc

SECONDS = 20.0                                                   # "a few seconds" with room for a loaded machine


def _extras(cus):
    return (0, 1, tc.placement_trip(cus) + 77)


def _claims_hold(case, pl, st):
    assert st["candidates"] == case["candidates"] and st["chain"] == case["nchain"]
    assert st["anchored"] == len(case["off"]) and st["unanchored"] == st["skipped"] == st["empty"] == 0
    for role, (r, y) in case["anchors"].items():
        p = pl["reads"][r]
        assert (int(p["kind"]), int(p["anchor"])) == (pu.ANCHORED, y), (role, p)


def _roles_expected(case):
    T, n = case["T"], case["n"]
    want = {"last"}
    if n > T + 1000:
        want |= {"best_above", "best_below", "tie", "t_then_q"}
    if n > 2 * T + 50:
        want |= {"third_trip"}
    return want


# ---- placement -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ring", [False, True])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_one_cu_placement_both_restatements_and_the_planted_winners(which, ring):
    case = tc.placement_pairs(1, _extras(1)[which], ring=ring)
    assert case["T"] == 4096 and case["n"] == 4096 + _extras(1)[which] == len(case["pairs"][0])
    assert set(case["anchors"]) == _roles_expected(case)
    inp = tc.placement_input(case)
    (a, sa), (b, sb) = pu.place_loops(inp), pu.place_tables(inp)
    assert sa == sb and pu.same_placements(a, b), pu.first_difference(a, b)
    _claims_hold(case, b, sb)
    back = np.arange(case["n"])[::-1]                            # the loops in the other order: the winners do not depend on it
    c, sc = pu.place_loops(inp, pair_order=back)
    assert sc == sb and pu.same_placements(c, b)


@pytest.mark.parametrize("cus", [1, 256])
def test_the_winning_pairs_lie_where_the_roles_say(cus):
    case = tc.placement_pairs(cus, _extras(cus)[2])
    T, n, ix = case["T"], case["n"], case["index"]
    q, t, v = case["pairs"]
    assert ix["last"] == n - 1 and (q[n - 1], t[n - 1]) == (case["M"] - 2, case["M"] - 1)
    assert T <= ix["best_above"] < 2 * T and ix["best_below"] < T and ix["tie"] < T and ix["t_then_q"] >= T and ix["third_trip"] >= 2 * T
    r = case["anchors"]["t_then_q"][0]
    assert q[ix["t_then_q"]] == r
    mine = np.flatnonzero(((q == r) | (t == r)) & (case["what"] == tc.CAND))
    assert (t[mine[mine < T]] == r).any() and int(v["score"][mine].max()) == 90 == int(v["score"][ix["t_then_q"]])
    r = case["anchors"]["tie"][0]
    mine = np.flatnonzero(((q == r) | (t == r)) & (v["score"] == 90))
    assert (mine < T).sum() == 2 and (mine >= T).sum() == 2 and mine.min() == ix["tie"]
    for extra in _extras(cus)[:2]:                               # a full single trip; one lane with a second trip: its pair is the last read's
        small = tc.placement_pairs(cus, extra)
        assert small["n"] == T + extra and small["index"] == {"last": T + extra - 1}


@pytest.mark.parametrize("cus", [1, 256])
@pytest.mark.parametrize("first", [False, True])
def test_bad_intervals_name_the_smallest_candidate(cus, first):
    T = tc.placement_trip(cus)
    bad = (9, T + 5) if first else (T + 5,)
    case = tc.placement_pairs(cus, 77, bad=bad)
    assert case["bad"] == (9 if first else T + 5) and case["n"] == T + 77
    inp = tc.placement_input(case)
    for f in (pu.place_tables, pu.place_loops) if cus == 1 else (pu.place_tables,):
        with pytest.raises(pu.BadInterval) as e:
            f(inp)
        assert e.value.pair == case["bad"]


@pytest.mark.parametrize("ring", [False, True])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_256_cu_placement_meets_its_conditions_in_seconds(which, ring):
    t0 = time.perf_counter()
    case = tc.placement_pairs(256, _extras(256)[which], ring=ring)
    t1 = time.perf_counter()
    T, n = case["T"], case["n"]
    assert T == 1048576 and n == T + (0, 1, T + 77)[which] and (n > T) == (which > 0) and (n > 2 * T) == (which == 2)
    assert set(case["anchors"]) == _roles_expected(case) and 900 <= len(case["off"]) <= 1100
    w = case["what"]
    assert (w == tc.CHAIN_CHAIN).sum() > 100 and (w == tc.OFF_OFF).sum() > 100 and 0 < case["candidates"] < (w == tc.CAND).sum() + 1
    inp = tc.placement_input(case)
    t2 = time.perf_counter()
    pl, st = pu.place_tables(inp)
    t3 = time.perf_counter()
    print("placement_pairs(256, %d): built in %.2f s, place_tables in %.2f s" % (n - T, t1 - t0, t3 - t2))
    _claims_hold(case, pl, st)
    assert t1 - t0 < SECONDS and t3 - t2 < SECONDS
    if ring:
        assert st["wrapped"] >= 0 and len(pl["credited_reads"]) == 2 and int(pl["credited_reads"][1]) >= 24


# ---- links -----------------------------------------------------------------------------------------------------------------------------------
def _links_input(g, flags):
    rows, cols, vals = cu.symmetric({(int(i), int(j)): o for i, j, o in zip(*g["pairs"])})
    seqs = ["A" * int(n) for n in g["lens"]]
    inp, _ = gu.inputs_of_restatement(g["M"], rows, cols, vals, seqs, flags)
    return inp


CASES = tc.links_cases()


def test_the_link_cases_are_the_ones_asked_for():
    assert len(CASES) == 3 + 4 + 5 + 6 + 7 and (600, (0, 63, 64, 255, 256, 599)) in CASES and (65, (64,)) in CASES and (257, (256,)) in CASES


@pytest.mark.parametrize("nb,hot", CASES, ids=["%d-%s" % (nb, "+".join(map(str, hot))) for nb, hot in CASES])
def test_links_graphs_hold_what_they_claim_in_their_hot_workgroups_alone(nb, hot):
    g = tc.links_graph(nb, hot)
    rows, cols, _ = g["pairs"]
    assert g["M"] == 256 * nb - 1 and (g["M"] + 1 + 255) // 256 == nb                  # the count pass's grid
    assert int(g["lens"].min()) >= 4 and int(g["lens"].max()) <= 24
    blocks = np.unique(np.concatenate([rows, cols]) // 256)
    assert blocks.tolist() == sorted(hot) and (rows // 256 == cols // 256).all()
    adj = {}
    for i, j in zip(rows.tolist(), cols.tolist()):
        adj.setdefault(i, set()).add(j); adj.setdefault(j, set()).add(i)
    assert not any(adj[i] & adj[j] for i, j in zip(rows.tolist(), cols.tolist()))       # no triangle
    walk = nb <= 65 or len(hot) > 1                                                    # (the literal walk where it is cheap and on every full case)
    for flags in (3, 1):
        t0 = time.perf_counter()
        inp = _links_input(g, flags)
        t1 = time.perf_counter()
        recs, st = gu.links_tables(inp)
        t2 = time.perf_counter()
        assert t1 - t0 < SECONDS and t2 - t1 < SECONDS, (t1 - t0, t2 - t1)
        assert {k: st[k] for k in tc.LINK_COUNTERS} == g["expected"][flags], (flags, st)
        assert all(st[k] > 0 for k in (("candidates", "links", "closures", "twisted", "clamped", "asymmetric") if flags == 3 else ("candidates", "closures", "unplaced")))
        if walk:
            recs2, st2 = gu.links_walk(inp)
            assert st2 == st and gu.same_records(recs, recs2)
        # every hot workgroup's content, counted from the records and the graph alone
        per = np.bincount(recs["from_read"] // 256, minlength=nb)
        for b, copies in g["content"].items():
            assert per[b] == copies * (tc.PER_COPY[flags]["links"] + 1) and copies > 0
        assert per.sum() == sum(per[b] for b in g["content"])


# ---- text ------------------------------------------------------------------------------------------------------------------------------------
def _texts(cus):
    R = tc.text_trip(cus) + 3
    return [("fasta", tc.fasta_text(cus)), ("fasta-no-final-newline", tc.fasta_text(cus, final_newline=False)), ("fasta-multi", tc.fasta_text(cus, multi=True)),
            ("fasta-multi-no-final-newline", tc.fasta_text(cus, multi=True, final_newline=False)), ("fastq", tc.fastq_text(cus)),
            ("fastq-no-final-newline", tc.fastq_text(cus, final_newline=False)),
            ("fasta-broken-last", tc.fasta_text(cus, broken=(R - 1,))), ("fasta-broken-7-and-late", tc.fasta_text(cus, multi=True, broken=(7, R - 2))),
            ("fastq-broken-last", tc.fastq_text(cus, broken=(R - 1,))), ("fastq-broken-7-and-late", tc.fastq_text(cus, broken=(7, R - 2)))]


@pytest.mark.parametrize("cus", [1, 256])
def test_texts_against_the_restatements(cus):
    trip = tc.text_trip(cus)
    for label, t in _texts(cus):
        data, R = t["data"], t["R"]
        assert R == trip + 3 and len(data) < (1 << 20) * 16
        if t["error"] is None:
            t0 = time.perf_counter()
            want = tx.index_numpy(data, "auto")
            dt = time.perf_counter() - t0
            assert dt < SECONDS, (label, dt)
            assert len(want["recs"]) == R > trip and want["lines"] > trip and want["format"] == t["fmt"], label
            assert (want["recs"]["len"] == 0).sum() >= 4 and int(want["recs"]["len"][R - 3]) == 0            # an empty read in the second trip
            assert (data[-1:] != b"\n") == ("no-final" in label)
            if "multi" in label:
                nl = np.frombuffer(data, dtype=np.uint8)
                hdr_lines = np.flatnonzero(np.concatenate([[True], nl[:-1] == 0x0A]) & (nl == 0x3E))
                line_of = np.cumsum(np.concatenate([[0], nl[:-1] == 0x0A]))[hdr_lines]
                assert (line_of > trip).sum() > R // 2 and want["lines"] >= 3 * R                             # headers in the second trip of the line kernels
                nseq = np.diff(np.append(line_of, want["lines"])) - 1
                assert set(np.unique(nseq[want["recs"]["len"] > 0]).tolist()) == {2, 3}
            if cus == 1:
                assert tx.same_index(tx.index_loop(data, "auto"), want), label
        else:
            kind, off, rec = t["error"]
            assert tx.error_of(tx.index_numpy, data) == (kind, off), label
            assert rec == (7 if "7" in label else R - 1)
            assert (data[:off].count(b">") == rec + 1) if t["fmt"] == "fasta" else (data[:off].count(b"\n+\n") == rec)
            if cus == 1:
                assert tx.error_of(tx.index_loop, data) == (kind, off), label
