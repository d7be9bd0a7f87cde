"""CPU: the two Python statements of the bridge rule (bridge_util.py) hold each other, whatever the order in which the second one visits the
anchors, every hand-made case shows what its name says, and the guarantees the header gives for a symmetric S are checked one by one.  These
tests hold the yardstick of tests/test_gpu_bridges.py; they do not run the library, except for the last one, which checks that the binding
declares the call."""
import ctypes as C

import numpy as np
import pytest

import bridge_util as br
import bubble_util as bu
import rounds_util as ru
import tip_util as tu
from elba_amd import capi
from oracle import pyoracle as po

CASES = br.hand_cases()
SEEDS = tuple(range(600, 624))


def params_of(seed):
    """(max_bridge_reads, min_flank_reads) of a random seed: drawn from {(1, 2), (2, 3)} so that the set as a whole has bridges."""
    return (2, 3) if seed % 4 == 0 else (1, 2)


def _S(case, seed=0, extra=0):
    M, rows, cols, vals = br.case_overlaps(case, np.random.default_rng(seed), extra)
    return (M,) + tuple(tu.symmetric_of(rows, cols, vals))


def _random_S(seed):
    M, rows, cols, vals, _, _ = ru.random_graph(seed)
    return (M,) + tuple(tu.symmetric_of(rows, cols, vals))


def _components(M, rows, cols):
    parent = list(range(M))
    for u, v in zip(rows.tolist(), cols.tolist()):
        a, b = bu._root(parent, u), bu._root(parent, v)
        if a != b:
            parent[a] = b
    return [bu._root(parent, v) for v in range(M)]


def _guarantees(M, rows, cols, vals, mx, F, want, trace):
    """Guarantees 1 to 3 of the header on a symmetric S, and what the stats must add up to."""
    r, c, v, flags, st = want
    bridges = trace["bridges"]
    deg, after = np.bincount(cols, minlength=M), np.bincount(c, minlength=M)
    # 1. no chain is a long flank; an anchor has at most one bridge; bridges are disjoint; nobody else loses an entry
    for a, b, reads in trace["chains"]:
        assert (a, reads[0]) not in trace["long"] and (b, reads[-1]) not in trace["long"] and len(reads) <= mx < F
    ends = [x for a, b, _ in bridges for x in (a, b)]
    inner = [x for _, _, reads in bridges for x in reads]
    assert len(ends) == len(set(ends)) and len(inner) == len(set(inner)) and not set(ends) & set(inner)
    changed = set(np.flatnonzero(deg != after).tolist())
    assert changed == set(ends) | set(inner)
    assert all(deg[x] == 3 and after[x] == 2 for x in ends) and all(deg[x] == 2 and after[x] == 0 for x in inner)
    assert set(np.flatnonzero(flags).tolist()) == set(inner) and (flags[inner] == 16).all()
    assert st["entries_removed"] == 2 * sum(len(reads) + 1 for _, _, reads in bridges) == len(rows) - len(r)
    assert st["bridges"] == len(bridges) and st["reads_removed"] == len(inner) and st["anchors"] == int((deg >= 3).sum())
    # the survivors are the input's entries without the removed reads', in the input's order
    keep = ~np.isin(rows, inner) & ~np.isin(cols, inner)
    assert (r == rows[keep]).all() and (c == cols[keep]).all() and v.tobytes() == vals[keep].tobytes()
    # 2. no component is erased
    comp = _components(M, rows, cols)
    assert {comp[x] for x in rows.tolist()} == {comp[x] for x in r.tolist()}
    # 3. the pass is its own fixed point
    again = br.cut_bridges(M, r, c, v, mx, F)
    assert again[4]["reads_removed"] == 0 and again[4]["bridges"] == 0 and len(again[0]) == len(r) and not again[3].any()
    # chains are the arms of one round of elba_pop_bubbles
    assert st["chains"] == bu.pop_bubbles(M, rows, cols, vals, mx, 1)[4]["arms"]


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_case_shows_what_its_name_says(name):
    case = CASES[name]
    M, rows, cols, vals = _S(case)
    deg = np.bincount(cols, minlength=M)
    for x, d in case["deg"].items():
        assert deg[x] == d, (name, x)
    trace = {}
    want = br.cut_bridges(M, rows, cols, vals, case["mx"], case["F"], trace=trace)
    r, c, v, flags, st = want
    assert set(np.flatnonzero(flags).tolist()) == case["removed"] and set(np.flatnonzero(flags == 16).tolist()) == case["removed"]
    assert (st["chains"], st["long_flanks"], st["bridges"]) == (case["chains"], case["long_flanks"], case["bridges"]), (name, st)
    after = np.bincount(c, minlength=M)
    for x, d in case["deg_after"].items():
        assert after[x] == d, (name, x)
    _guarantees(M, rows, cols, vals, case["mx"], case["F"], want, trace)
    if case["perm"] is not None and "random" not in name:
        assert {0, M - 1} <= set(case["deg"])                   # the named reads do sit at both ends of the id range


@pytest.mark.parametrize("name", sorted(CASES))
def test_peeling_bridges_one_by_one_gives_the_same_on_hand_cases(name):
    case = CASES[name]
    M, rows, cols, vals = _S(case, extra=3)
    want = br.cut_bridges(M, rows, cols, vals, case["mx"], case["F"])
    for seed in range(20):
        order = np.random.default_rng(seed).permutation(M)
        assert br.same(want, br.cut_bridges_peel(M, rows, cols, vals, case["mx"], case["F"], order=order), br.PEEL_STATS), (name, seed)
    assert br.same(want, br.cut_bridges_peel(M, rows, cols, vals, case["mx"], case["F"]), br.PEEL_STATS)


def test_the_random_seeds_hold_the_guarantees_and_two_bridges():
    total = 0
    for seed in SEEDS:
        M, rows, cols, vals = _random_S(seed)
        mx, F = params_of(seed)
        trace = {}
        want = br.cut_bridges(M, rows, cols, vals, mx, F, trace=trace)
        _guarantees(M, rows, cols, vals, mx, F, want, trace)
        total += want[4]["bridges"]
    assert total == 2, total                                    # seeds 620 at (2, 3) and 622 at (1, 2) have one bridge each


@pytest.mark.parametrize("block", range(4))
def test_both_statements_agree_on_random_graphs_under_20_orders(block):
    for seed in SEEDS[6 * block:6 * block + 6]:
        M, rows, cols, vals = _random_S(seed)
        mx, F = params_of(seed)
        want = br.cut_bridges(M, rows, cols, vals, mx, F)
        rng = np.random.default_rng(seed + 1000)
        for _ in range(20):
            assert br.same(want, br.cut_bridges_peel(M, rows, cols, vals, mx, F, order=rng.permutation(M)), br.PEEL_STATS), seed


@pytest.mark.parametrize("mx,F,t,gap", [(1, 2, 1, 2), (1, 2, 1, 1), (2, 3, 2, 3), (2, 3, 1, 2), (3, 7, 3, 7), (3, 7, 2, 6), (3, 7, 4, 7)])
def test_crowded_planted_bridges_hold_the_guarantees_in_any_order(mx, F, t, gap):
    """H's planted gap reads apart on a few paths: at gap = F every planted chain of t <= mx reads is cut, at gap = F - 1 neighbouring
    anchors are each other's short flanks and only some are; either way the peeled result is the same in every order."""
    rng = np.random.default_rng(100 * mx + gap)
    M, rows, cols, vals = br.long_paths(rng, 4, 40 * (gap + 1))
    n = 60 if gap >= F else 20                                  # (40 anchors on 150 slots: some have both neighbouring slots free)
    M2, r2, c2, v2, planted, pairs = br.plant_bridges(rng, M, rows, cols, vals, n, t, gap=gap)
    S = tu.symmetric_of(r2, c2, v2)
    trace = {}
    want = br.cut_bridges(M2, *S, mx, F, trace=trace)
    _guarantees(M2, *S, mx, F, want, trace)
    if t > mx:
        assert want[4]["bridges"] == 0 and want[4]["chains"] == 0
    elif gap >= F:
        assert want[4]["bridges"] == 60 and set(np.flatnonzero(want[3]).tolist()) == set(planted.tolist())
    else:
        assert 0 < want[4]["bridges"] < n and want[4]["chains"] >= n
    for seed in range(5):
        assert br.same(want, br.cut_bridges_peel(M2, *S, mx, F, order=np.random.default_rng(seed).permutation(M2)), br.PEEL_STATS)


def test_200_planted_bridges_survive_the_reduction_and_are_what_the_restatement_removes():
    """Ten paths of 600 reads; 200 chains of one read planted between inner reads that lie 8 reads apart or more.  The oracle's reduction at
    fuzz 0 keeps every entry (suffixes in [5, 9]: a two-edge walk is at least 10), and the restatement takes exactly the planted reads out."""
    rng = np.random.default_rng(9)
    M, rows, cols, vals = br.long_paths(rng, 10, 600)
    M2, r2, c2, v2, planted, pairs = br.plant_bridges(rng, M, rows, cols, vals, 200, 1)
    assert M2 == M + 200 and len(planted) == 200 and len(r2) == len(rows) + 400
    S = tu.symmetric_of(r2, c2, v2)
    got, flags0, _ = po.string_graph(M2, r2, c2, v2, 0.0, 0)
    assert got["n"] == 2 * len(r2) and (got["rows"] == S[0]).all() and (got["cols"] == S[1]).all() and got["vals"].tobytes() == S[2].tobytes()
    assert not flags0.any()
    for mx, F in ((1, 2), (1, 8), (3, 7)):
        r, c, v, flags, st = br.cut_bridges(M2, *S, mx, F)
        assert set(np.flatnonzero(flags).tolist()) == set(planted.tolist())
        assert st["bridges"] == 200 and st["chains"] == 200 and st["anchors"] == 400 and st["long_flanks"] == 800 and st["entries_removed"] == 800
        base = tu.symmetric_of(rows, cols, vals)
        assert (r == base[0]).all() and (c == base[1]).all() and v.tobytes() == base[2].tobytes()
    assert br.cut_bridges(M2, *S, 1, 9)[4]["bridges"] < 200     # some anchors are exactly 8 reads apart


def test_simplify_with_bridges_ends_after_a_pass_that_removes_nothing():
    g = tu.Graph()
    a, b, ch, fl = br._h(g, 1, (3, 3, 3, 3))
    tip = g.arm(fl[0][1], 1)                                    # a tip on a flank hides the long flank until it is clipped
    M, rows, cols, vals = g.overlaps(np.random.default_rng(2))
    S = tu.symmetric_of(rows, cols, vals)
    assert br.cut_bridges(M, *S, 1, 3)[4]["bridges"] == 0
    r, c, v, flags, passes = br.simplify(M, *S, 1, 3, (1, 3))
    assert {int(x): int(flags[x]) for x in np.flatnonzero(flags)} == {tip[0]: 4, ch[0]: 16}
    assert len(passes) == 2 and all(len(p) == 3 for p in passes) and passes[0][2]["bridges"] == 1 and passes[1][2]["reads_removed"] == 0
    r, c, v, flags, passes = br.simplify(M, *S, 1, 3, (1, 3), q16=45875)
    assert len(passes) == 2 and all(len(p) == 4 for p in passes) and passes[0][3]["bridges"] == 1


def test_binding_declares_cut_bridges():
    assert "elba_cut_bridges" in capi.EXPORTED_SYMBOLS
    assert C.sizeof(capi.BridgeCfg) == 16 and C.sizeof(capi.BridgeStats) == 9 * 8 + 2 * 4
    import elba_amd
    L = elba_amd.load_library()
    assert hasattr(L, "elba_cut_bridges") and hasattr(elba_amd.Engine, "cut_bridges") and L.elba_abi_version() == 3
