"""CPU: the two Python statements of the star rule (star_util.py) hold each other, whatever the order in which the second one visits the
reads, every hand-made case shows what its name says, the devices the generators rely on (an R-only pair, a truly transitive pair) are what
the oracle's reduction makes of them, and the guarantees the header gives are checked one by one.  These tests hold the yardstick of
tests/test_gpu_stars.py; they do not run the library, except for the last one, which checks that the binding declares the call."""
import ctypes as C

import numpy as np
import pytest

import star_util as su
import tip_util as tu
from elba_amd import capi
from oracle import pyoracle as po

CASES = su.hand_cases()
SEEDS = tuple(range(700, 724))


def _oracle_S(M, rows, cols, vals, cutoff=0.0, fuzz=0):
    got, flags, st = po.string_graph(M, rows, cols, vals, cutoff, fuzz)
    return (got["rows"], got["cols"], got["vals"]), flags, st


def _S(case, seed=0, extra=0):
    """(M, S rows, cols, vals, R) of a hand case: S is the oracle's reduction of the case's overlaps, R its pairs."""
    M, rows, cols, vals = su.case_overlaps(case, np.random.default_rng(seed), extra)
    S, flags, _ = _oracle_S(M, rows, cols, vals)
    assert not flags.any()
    return (M,) + S + (su.r_pairs(M, rows, cols, vals),)


def _symmetric(rows, cols):
    return set(zip(rows.tolist(), cols.tolist())) == set(zip(cols.tolist(), rows.tolist()))


def _guarantees(M, rows, cols, vals, R, rounds, want, trace):
    """Guarantees 2 to 4 of the header on a symmetric S, and what the stats must add up to.  (1, the order, is the peel tests'.)"""
    r, c, v, flags, st = want
    deg = np.bincount(cols, minlength=M)
    removed = []
    for rnd in trace:
        # 2. only reads of degree 2, on the round's own tables, are removed, and no centre of the round
        for u, e, w in rnd["centres"]:
            assert deg[u] == 3 and (w is None) == (e != 1)
            if w is not None:
                assert deg[w] == 2 and w in rnd["odd"]
        assert not rnd["odd"] & {u for u, _, _ in rnd["centres"]} and all(deg[w] == 2 for w in rnd["odd"])
        # 3. reads_removed <= resolved, with equality unless two centres name the same arm
        named = [w for _, e, w in rnd["centres"] if e == 1]
        assert len(rnd["odd"]) <= len(named) and (len(rnd["odd"]) == len(named)) == (len(set(named)) == len(named)) and set(named) == rnd["odd"]
        removed += sorted(rnd["odd"])
        gone = np.isin(rows, removed) | np.isin(cols, removed)
        deg = np.bincount(cols[~gone], minlength=M)
    assert len(removed) == len(set(removed)) == st["reads_removed"] <= st["pairs1"]
    assert st["centres"] == sum(len(rnd["centres"]) for rnd in trace) == st["pairs0"] + st["pairs1"] + st["pairs2"] + st["pairs3"]
    assert set(np.flatnonzero(flags).tolist()) == set(removed) and (flags[removed] == 32).all()
    # the survivors are the input's entries without the removed reads', in the input's order
    keep = ~np.isin(rows, removed) & ~np.isin(cols, removed)
    assert (r == rows[keep]).all() and (c == cols[keep]).all() and v.tobytes() == vals[keep].tobytes()
    assert st["entries_removed"] == int((~keep).sum()) == len(rows) - len(r) and st["nnz_after"] == len(r)
    # rounds_run counts the round that removed nothing, if one ran
    moving = sum(1 for rnd in trace if rnd["odd"])
    assert st["rounds_run"] == len(trace) == min(moving + 1, rounds)
    # 4. a round that removes nothing is a fixed point of the call
    if moving < len(trace):
        for again_rounds in (1, 64):
            again = su.resolve_stars(M, r, c, v, R, again_rounds)
            assert again[4]["reads_removed"] == 0 and again[4]["rounds_run"] == 1 and len(again[0]) == len(r) and not again[3].any()
            assert again[4]["centres"] == len(trace[-1]["centres"]) and again[4]["pairs1"] == 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_case_shows_what_its_name_says(name):
    case = CASES[name]
    M, rows, cols, vals, R = _S(case)
    assert _symmetric(rows, cols) != bool(case.get("one_image"))
    deg = np.bincount(cols, minlength=M)
    for x, d in case["deg"].items():
        assert deg[x] == d, (name, x, deg[x])
    trace = []
    want = su.resolve_stars(M, rows, cols, vals, R, 64, trace=trace)
    r, c, v, flags, st = want
    assert set(np.flatnonzero(flags).tolist()) == case["removed"] and set(np.flatnonzero(flags == 32).tolist()) == case["removed"]
    assert st["centres"] == case["centres"] and (st["pairs0"], st["pairs1"], st["pairs2"], st["pairs3"]) == case["by_e"], (name, st)
    assert st["rounds_run"] == case["moves"] + 1 and sum(1 for rnd in trace if rnd["odd"]) == case["moves"]
    after = np.bincount(c, minlength=M)
    for x, d in case["deg_after"].items():
        assert after[x] == d, (name, x, after[x])
    if not case.get("one_image"):
        _guarantees(M, rows, cols, vals, R, 64, want, trace)
    if case["perm"] is not None and "random" not in name:
        assert {0, M - 1} <= set(case["deg"])                   # the named reads do sit at both ends of the id range
    if "chain" in case:                                         # round k resolves the k-th star and no other
        cs, ws = case["chain"]
        assert [rnd["centres"] for rnd in trace[:-1]] == [[(ck, 1, wk)] for ck, wk in zip(cs, ws)] and trace[-1]["centres"] == []
        for rounds in range(1, len(cs) + 2):
            part = su.resolve_stars(M, rows, cols, vals, R, rounds)
            assert part[4]["reads_removed"] == min(rounds, len(cs)) and part[4]["rounds_run"] == min(rounds, len(cs) + 1)
            rest = su.resolve_stars(M, part[0], part[1], part[2], R, 64)        # a second call finishes
            assert rest[4]["reads_removed"] == len(cs) - part[4]["reads_removed"] and su.same((rest[0], rest[1], rest[2], part[3] | rest[3], st), want, ())


@pytest.mark.parametrize("name", sorted(n for n in CASES if not CASES[n].get("one_image")))
def test_the_second_form_gives_the_same_on_hand_cases_under_20_orders(name):
    case = CASES[name]
    M, rows, cols, vals, R = _S(case, extra=3)
    for rounds in (1, 64):
        want = su.resolve_stars(M, rows, cols, vals, R, rounds)
        for seed in range(20):
            order = np.random.default_rng(seed).permutation(M)
            assert su.same(want, su.resolve_stars_peel(M, rows, cols, vals, R, rounds, order=order)), (name, seed)
        assert su.same(want, su.resolve_stars_peel(M, rows, cols, vals, R, rounds))


@pytest.mark.parametrize("block", range(4))
def test_both_statements_agree_on_random_graphs_under_20_orders(block):
    for seed in SEEDS[6 * block:6 * block + 6]:
        M, rows, cols, vals = su.random_stars(seed)
        S, flags, _ = _oracle_S(M, rows, cols, vals)
        R = su.r_pairs(M, rows, cols, vals)
        for rounds in (1, 64):
            trace = []
            want = su.resolve_stars(M, *S, R, rounds, trace=trace)
            _guarantees(M, *S, R, rounds, want, trace)
            rng = np.random.default_rng(seed + 1000)
            for _ in range(20 if rounds == 64 else 3):
                assert su.same(want, su.resolve_stars_peel(M, *S, R, rounds, order=rng.permutation(M))), seed


def test_the_random_seeds_have_centres_of_every_kind_and_a_second_round():
    tot = dict.fromkeys(su.STATS, 0)
    moving = []
    for seed in SEEDS:
        M, rows, cols, vals = su.random_stars(seed)
        S, _, _ = _oracle_S(M, rows, cols, vals)
        st = su.resolve_stars(M, *S, su.r_pairs(M, rows, cols, vals), 64)[4]
        for k in su.STATS:
            tot[k] += st[k]
        moving.append(st["rounds_run"] - 1)
    assert tot["pairs0"] > 0 and tot["pairs1"] >= 24 and tot["pairs2"] > 0 and tot["pairs3"] > 0 and tot["reads_removed"] >= 24, tot
    assert max(moving) >= 2 and min(moving) == 0, moving


def test_an_R_only_pair_stays_in_R_never_reaches_S_and_takes_part_in_no_product():
    """The three things star_util relies on for an entry with passed = 1 and direction = directionT = -1, from the oracle's reduction: it is
    among the kept edges (R), S is entry for entry the S of the graph without it, and no product through it has a value: the reduction
    marks and removes exactly what it marks and removes without it.  (The `products` stat is the sum of the squared row lengths of R, the
    products a SpGEMM would form; that one grows with the row lengths, value or no value.)  On every hand case, and on a layout whose
    reduction does mark entries, between two reads with a common partner, with suffixes so small that a product through the pair, had it
    a value, would be below every entry's suffix + fuzz."""
    for name, case in sorted(CASES.items()):
        g = case["graph"]
        if not g.ronly:
            continue
        M, rows, cols, vals = g.overlaps(np.random.default_rng(0), perm=case["perm"])
        ronly = vals["direction"] == -1
        assert int(ronly.sum()) == len(g.ronly) and (vals["directionT"][ronly] == -1).all() and (vals["passed"] == 1).all()
        S, flags, st = _oracle_S(M, rows, cols, vals)
        S0, flags0, st0 = _oracle_S(M, rows[~ronly], cols[~ronly], vals[~ronly])
        assert st["edges_kept"] == len(rows) == st0["edges_kept"] + len(g.ronly) and not flags.any()
        assert (S[0] == S0[0]).all() and (S[1] == S0[1]).all() and S[2].tobytes() == S0[2].tobytes()
        assert st["marked"] == st0["marked"] == 0 and st["removed"] == st0["removed"] == 0 and st["products"] >= st0["products"]
        R = su.r_pairs(M, rows, cols, vals)
        assert all((int(r), int(c)) in R for r, c in zip(rows[ronly], cols[ronly])) and len(R) == len(rows)
    # with products around: an R-only pair between two reads that have common partners
    M, rows, cols, vals, centres, w = su.layout_stars(3, M=40, every=(10, 20))
    extra = np.zeros(1, dtype=vals.dtype)
    extra["passed"] = 1; extra["direction"] = -1; extra["directionT"] = -1; extra["suffix"] = -20000; extra["suffixT"] = -20000
    have = set(zip(rows.tolist(), cols.tolist()))
    pair = next((a, b) for a in range(40) for b in range(a + 1, 40) if (a, b) not in have and any((min(a, k), max(a, k)) in have and (min(b, k), max(b, k)) in have for k in range(40)))
    r2 = np.concatenate([rows, [pair[0]]]); c2 = np.concatenate([cols, [pair[1]]]); v2 = np.concatenate([vals, extra])
    order = np.lexsort((c2, r2))
    S, flags, st = _oracle_S(M, r2[order], c2[order], v2[order], 0.65, 1000)
    S0, flags0, st0 = _oracle_S(M, rows, cols, vals, 0.65, 1000)
    assert st0["marked"] > 0 and st["marked"] == st0["marked"] and st["removed"] == st0["removed"] and st["edges_kept"] == st0["edges_kept"] + 1 and (flags == flags0).all()
    assert (S[0] == S0[0]).all() and (S[1] == S0[1]).all() and S[2].tobytes() == S0[2].tobytes()


def test_a_truly_transitive_pair_is_in_R_and_not_in_S():
    """layout_stars: five reads of a layout, the middle one with a stray read.  The oracle's reduction at fuzz 1000 leaves the path 0 - 1 -
    2 - 3 - 4 and the stray chain; {1, 3} is in R as a removed, transitive entry, and the stray read is the odd arm."""
    for seed in range(4):
        M, rows, cols, vals, centres, w = su.layout_stars(seed)
        assert M == 7 and centres.tolist() == [2] and w.tolist() == [5] and len(rows) == 12
        S, flags, st = _oracle_S(M, rows, cols, vals, 0.65, 1000)
        assert not flags.any() and st["removed"] > 0
        pairs = set(zip(S[0].tolist(), S[1].tolist()))
        assert pairs == {(a, b) for a, b in ((0, 1), (1, 2), (2, 3), (3, 4), (2, 5), (5, 6)) for a, b in ((a, b), (b, a))}
        R = su.r_pairs(M, rows, cols, vals, 0.65, 1000)
        assert (1, 3) in R and (1, 5) not in R and (3, 5) not in R and (1, 3) not in pairs
        r, c, v, f, s = su.resolve_stars(M, *S, R, 64)
        assert np.flatnonzero(f).tolist() == [5] and s["pairs1"] == 1 and s["centres"] == 1 and s["rounds_run"] == 2
    M, rows, cols, vals, centres, w = su.layout_stars(3, M=400, every=range(5, 395, 10))
    S, flags, st = _oracle_S(M, rows, cols, vals, 0.65, 1000)
    s = su.resolve_stars(M, *S, su.r_pairs(M, rows, cols, vals, 0.65, 1000), 64)[4]
    assert s["pairs1"] >= 30 and s["reads_removed"] == s["pairs1"], s


def test_r_pairs_leaves_out_failed_pairs_and_pairs_of_bad_or_contained_reads():
    g = su.StarGraph(); u, arms = su._star(g, pairs=[(0, 1)])
    M, rows, cols, vals = g.overlaps(np.random.default_rng(1))
    vals = vals.copy()
    fail = int(np.flatnonzero((rows == arms[2][0]) & (cols == arms[2][1]))[0])
    vals["passed"][fail] = 0
    cont = int(np.flatnonzero((rows == arms[0][0]) & (cols == arms[0][1]))[0])
    vals["containedT"][cont] = 1                               # arms[0][1] is contained: its one pair leaves R
    R = su.r_pairs(M, rows, cols, vals)
    assert len(R) == len(rows) - 2 and (arms[2][0], arms[2][1]) not in R and (arms[0][0], arms[0][1]) not in R and (arms[0][0], arms[1][0]) in R


@pytest.mark.parametrize("length", su.LOOKUP_LENGTHS)
def test_lookup_cases_have_the_row_and_the_key_where_they_say(length):
    for place in su.LOOKUP_PLACES:
        for short in (0, 1):
            if place in ("first", "last") and length < 3:
                continue
            M, rows, cols, vals, info = su.lookup_case(length, place, short)
            R = su.r_pairs(M, rows, cols, vals)
            s, k = info["s"], info["k"]
            row_s = sorted([b for a, b in R if a == s] + [a for a, b in R if b == s]); row_k = [1 for a, b in R if k in (a, b)]
            assert len(row_s) == length and len(row_k) == length + 7 and (k in row_s) == info["present"] and (s < k) == (short == 1)
            others = [x for x in row_s if x != k]
            assert others == info["row"]
            want = {"first": all(x > k for x in others), "last": all(x < k for x in others), "below": all(x > k for x in others), "above": all(x < k for x in others),
                    "between": min(others) < k < max(others)}[place]
            assert want, (length, place, short)
            S, _, _ = _oracle_S(M, rows, cols, vals)
            r, c, v, f, st = su.resolve_stars(M, *S, R, 1)
            assert st["centres"] == 1 and st["pairs1"] == int(info["present"]) and st["pairs0"] == 1 - int(info["present"])
            assert np.flatnonzero(f).tolist() == ([info["odd"]] if info["present"] else [])


def test_planted_stars_are_what_the_restatement_resolves():
    rng = np.random.default_rng(9)
    M, rows, cols, vals = su.long_paths(rng, 10, 600)
    M2, r2, c2, v2, centres, w = su.plant_stars(rng, M, rows, cols, vals, 200)
    assert M2 == M + 400 and len(r2) == len(rows) + 600
    S, flags, st = _oracle_S(M2, r2, c2, v2)
    assert st["nnz"] == 2 * (len(rows) + 400) and not flags.any()
    R = su.r_pairs(M2, r2, c2, v2)
    r, c, v, f, s = su.resolve_stars(M2, *S, R, 64)
    assert set(np.flatnonzero(f).tolist()) == set(w.tolist()) and s["pairs1"] == s["centres"] == 200 and s["entries_removed"] == 800 and s["rounds_run"] == 2
    base = tu.symmetric_of(rows, cols, vals)
    assert (r == base[0]).all() and (c == base[1]).all() and v.tobytes() == base[2].tobytes()      # the paths as they were
    M3, r3, c3, v3, _, _ = su.plant_stars(np.random.default_rng(9), M, rows, cols, vals, 200, pairs_in_R=0)
    S3, _, _ = _oracle_S(M3, r3, c3, v3)
    s3 = su.resolve_stars(M3, *S3, su.r_pairs(M3, r3, c3, v3), 64)[4]
    assert s3["pairs0"] == s3["centres"] == 200 and s3["reads_removed"] == 0


def test_simplify_with_stars_ends_after_a_pass_that_removes_nothing():
    g = su.StarGraph(); u, arms = su._star(g, tails=(4, 4, 4), pairs=[(0, 1)])
    tip = g.arm(arms[0][0], 1)                                  # a tip on a neighbour hides the star until it is clipped
    M, rows, cols, vals = g.overlaps(np.random.default_rng(2))
    S, _, _ = _oracle_S(M, rows, cols, vals)
    R = su.r_pairs(M, rows, cols, vals)
    assert su.resolve_stars(M, *S, R, 64)[4]["centres"] == 0
    r, c, v, flags, passes = su.simplify(M, *S, R, 1, 3)
    assert {int(x): int(flags[x]) for x in np.flatnonzero(flags)} == {tip[0]: 4, arms[2][0]: 32}
    assert len(passes) == 2 and all(len(p) == 3 for p in passes) and passes[0][2]["pairs1"] == 1 and passes[1][2]["reads_removed"] == 0
    r, c, v, flags, passes = su.simplify(M, *S, R, 1, 3, q16=45875, bridges=(1, 3))
    assert all(len(p) == 5 for p in passes) and passes[0][4]["pairs1"] == 1


def test_binding_declares_resolve_stars():
    assert "elba_resolve_stars" in capi.EXPORTED_SYMBOLS
    assert C.sizeof(capi.StarCfg) == 16 and C.sizeof(capi.StarStats) == 10 * 8 + 4 * 4
    import elba_amd
    L = elba_amd.load_library()
    assert hasattr(L, "elba_resolve_stars") and hasattr(elba_amd.Engine, "resolve_stars") and L.elba_abi_version() == 3
