"""CPU: the two Python statements of the bubble-popping rule (bubble_util.py) hold each other, whatever the order in which the second one
deletes the losing arms, and every hand-made case shows what its name says: the degrees, the arms found, the bubbles, the reads removed and
the rounds run are asserted from the case's own input.  These tests hold the yardstick of tests/test_gpu_bubbles.py; they do not run the
library, except for the last one, which checks that the binding declares the call."""
import ctypes as C

import numpy as np
import pytest

import bubble_util as bu
import contig_util as cu
import tip_util as tu
from elba_amd import capi
from oracle import pyoracle as po

CASES = bu.hand_cases()


def _S(case, seed=0, extra=0):
    M, rows, cols, vals = tu.case_overlaps(case, np.random.default_rng(seed), extra)
    return (M,) + tuple(tu.symmetric_of(rows, cols, vals))


def _components(M, rows, cols):
    parent = list(range(M))
    for u, v in zip(rows.tolist(), cols.tolist()):
        ru, rv = bu._root(parent, u), bu._root(parent, v)
        if ru != rv:
            parent[ru] = rv
    return [bu._root(parent, v) for v in range(M)]


def _guarantees(M, rows, cols, trace_round, removed_round):
    """On a symmetric S: the arms of a round are disjoint, every bubble keeps one arm, no component loses all its entries."""
    arms, gone = trace_round
    reads = [v for _, _, chain in arms for v in chain]
    assert len(reads) == len(set(reads))
    groups = {}
    for a, b, chain in arms:
        groups.setdefault((a, b), []).append(chain)
    lost = {}
    for a, b, chain in gone:
        lost[(a, b)] = lost.get((a, b), 0) + 1
    for key, n in lost.items():
        assert n == len(groups[key]) - 1
    comp = _components(M, rows, cols)
    keep = ~np.isin(rows, list(removed_round)) & ~np.isin(cols, list(removed_round))
    assert {comp[v] for v in rows.tolist()} == {comp[v] for v in rows[keep].tolist()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_case_shows_what_its_name_says(name):
    case = CASES[name]
    M, rows, cols, vals = _S(case)
    deg = np.bincount(cols, minlength=M)
    for v, d in case["deg"].items():
        assert deg[v] == d, (name, v)
    trace = []
    r, c, v, flags, st = bu.pop_bubbles(M, rows, cols, vals, case["max"], case["rounds"], trace=trace)
    arms, gone = trace[0]
    assert sorted(len(chain) for _, _, chain in arms) == case["arm_lengths"]
    assert all(a < b and deg[a] >= 3 and deg[b] >= 3 and all(deg[x] == 2 for x in chain) for a, b, chain in arms)
    assert len({(a, b) for a, b, _ in gone}) == case["bubbles"]
    assert set(np.flatnonzero(flags == 8).tolist()) == case["removed"] and set(np.flatnonzero(flags).tolist()) == case["removed"]
    assert st["rounds_run"] == case["rounds_run"] and st["reads_removed"] == len(case["removed"])
    assert st["anchors"] == int((deg >= 3).sum()) and st["nnz_before"] == len(rows) and st["nnz_after"] == len(r)
    after = np.bincount(c, minlength=M)
    for x, d in case["deg_after"].items():
        assert after[x] == d, (name, x)
    # the survivors are the input's entries without the removed reads', in the input's order
    keep = ~np.isin(rows, list(case["removed"])) & ~np.isin(cols, list(case["removed"]))
    assert (r == rows[keep]).all() and (c == cols[keep]).all() and v.tobytes() == vals[keep].tobytes()
    assert st["entries_removed"] == int((~keep).sum())
    _guarantees(M, rows, cols, trace[0], {x for _, _, chain in gone for x in chain})
    if name.startswith("direct_edge"):
        a = min(case["deg"])
        b = max(case["deg"])
        assert ((r == a) & (c == b)).sum() == 1 and ((r == b) & (c == a)).sum() == 1          # the direct entry stays
    if name == "theta_ends_as_a_path":
        assert sorted(after[after > 0].tolist()) == [1, 1, 2, 2, 2]                           # one path: the component survives


@pytest.mark.parametrize("name", sorted(CASES))
def test_deleting_one_arm_at_a_time_gives_the_same_on_hand_cases(name):
    case = CASES[name]
    M, rows, cols, vals = _S(case, extra=3)
    want = bu.pop_bubbles(M, rows, cols, vals, case["max"], case["rounds"])
    for seed in range(3):
        order = np.random.default_rng(seed).permutation(M)
        assert tu.same(want, bu.pop_bubbles_chains(M, rows, cols, vals, case["max"], case["rounds"], order=order)), (name, seed)
    assert tu.same(want, bu.pop_bubbles_chains(M, rows, cols, vals, case["max"], case["rounds"]))


def _random_graph(rng):
    """A sparse random string graph with a few chains planted between reads it already has: random edges alone rarely close a bubble."""
    M = int(rng.integers(4, 100))
    lens = rng.integers(20, 41, M)
    rows, cols, vals = cu.random_string_graph(rng, M, lens, n_paths=int(rng.integers(1, M // 3 + 2)), p_extra=float(rng.choice([0.05, 0.15, 0.4])))
    k = int(rng.integers(0, 7))
    ends = rng.integers(0, M, (k, 2))
    if k and rng.random() < 0.5:
        ends[1:] = np.where(rng.random((k - 1, 1)) < 0.6, ends[0], ends[1:])                  # several chains between the same two reads
    ends = ends[ends[:, 0] != ends[:, 1]]
    return bu.plant_bubbles(rng, M, rows, cols, vals, [tuple(e) for e in ends.tolist()], rng.integers(1, 4, len(ends)))[:4]


@pytest.mark.parametrize("block", range(6))
def test_both_statements_agree_on_random_graphs(block):
    removed = rounds_seen = bubbles = 0
    for seed in range(50):
        rng = np.random.default_rng(1000 * block + seed)
        M, rows, cols, vals = _random_graph(rng)
        S = tu.symmetric_of(rows, cols, vals)
        mx, rounds = int(rng.choice([1, 2, 3, 7, 50])), int(rng.choice([1, 2, 5, 64]))
        trace = []
        want = bu.pop_bubbles(M, *S, mx, rounds, trace=trace)
        assert tu.same(want, bu.pop_bubbles_chains(M, *S, mx, rounds, order=rng.permutation(M))), (block, seed)
        st = want[4]
        assert st["rounds_run"] <= rounds and st["nnz_after"] == len(want[0]) and st["reads_removed"] == int((want[3] == 8).sum())
        assert st["arms_removed"] >= st["bubbles"] and st["arms"] >= st["arms_removed"] + st["bubbles"]
        _guarantees(M, S[0], S[1], trace[0], {x for _, _, chain in trace[0][1] for x in chain})
        removed += st["reads_removed"]; rounds_seen = max(rounds_seen, st["rounds_run"]); bubbles += st["bubbles"]
    assert removed > 0 and bubbles > 0 and rounds_seen >= 2    # the random graphs do have bubbles


def test_a_second_pop_of_a_popped_graph_removes_nothing():
    for name, case in CASES.items():
        M, rows, cols, vals = _S(case)
        r, c, v, _, st = bu.pop_bubbles(M, rows, cols, vals, case["max"], 64)
        again = bu.pop_bubbles(M, r, c, v, case["max"], 64)
        assert again[4]["reads_removed"] == 0 and again[4]["rounds_run"] == 1 and len(again[0]) == len(r), name


@pytest.mark.parametrize("name", ["tip_on_an_arm", "bubble_inside_a_dead_end_chain"])
def test_alternation_cases(name):
    case = CASES[name]
    M, rows, cols, vals = _S(case)
    tips_alone = tu.clip_tips(M, rows, cols, vals, case["max_tip"], 64)
    pops_alone = bu.pop_bubbles(M, rows, cols, vals, case["max"], 64)
    if name == "tip_on_an_arm":
        assert pops_alone[4]["reads_removed"] == 0 and tips_alone[4]["reads_removed"] == 1
    else:
        assert tips_alone[4]["reads_removed"] == 0 and tips_alone[4]["dead_ends"] == 3
    r, c, v, flags, passes = bu.simplify(M, rows, cols, vals, case["max_tip"], case["max"])
    assert {int(x): int(flags[x]) for x in np.flatnonzero(flags)} == case["removed_simplify"]
    assert len(passes) == 2 and passes[-1][0]["reads_removed"] == 0 and passes[-1][1]["reads_removed"] == 0


def test_planted_arms_survive_the_reduction_and_are_what_the_restatement_removes():
    """A path; one-read and two-read chains planted across stretches of three reads.  The oracle's reduction at fuzz 0 keeps every entry
    (suffixes in [5, 9]: a two-edge walk is at least 10), and the restatement takes exactly the planted reads back out."""
    rng = np.random.default_rng(5)
    g = tu.Graph()
    path = g.chain(g.new(60))
    M, rows, cols, vals = g.overlaps(rng)
    pairs, lengths = [(5, 9), (20, 24), (33, 37), (45, 49)], [1, 2, 1, 2]
    M2, r2, c2, v2, planted = bu.plant_bubbles(rng, M, rows, cols, vals, pairs, lengths)
    assert M2 == M + sum(lengths) and len(planted) == sum(lengths) and len(r2) == len(rows) + sum(lengths) + len(pairs)
    S = tu.symmetric_of(r2, c2, v2)
    got, flags0, _ = po.string_graph(M2, r2, c2, v2, 0.0, 0)
    assert got["n"] == 2 * len(r2) and (got["rows"] == S[0]).all() and (got["cols"] == S[1]).all() and got["vals"].tobytes() == S[2].tobytes()
    assert not flags0.any()
    r, c, v, flags, st = bu.pop_bubbles(M2, *S, 4, 1)
    assert set(np.flatnonzero(flags).tolist()) == set(planted.tolist()) and st["bubbles"] == 4 and st["arms"] == 8 and st["anchors"] == 8
    base = tu.symmetric_of(rows, cols, vals)
    assert (r == base[0]).all() and (c == base[1]).all() and v.tobytes() == base[2].tobytes()
    assert path[0] == 0


def test_binding_declares_pop_bubbles():
    assert "elba_pop_bubbles" in capi.EXPORTED_SYMBOLS
    assert C.sizeof(capi.BubbleCfg) == 16 and C.sizeof(capi.BubbleStats) == 9 * 8 + 2 * 4 + 2 * 4
    import elba_amd
    assert hasattr(elba_amd.load_library(), "elba_pop_bubbles") and hasattr(elba_amd.Engine, "pop_bubbles") and hasattr(elba_amd.Engine, "simplify_graph")
