"""CPU: the two Python statements of the tip-clipping rule (tip_util.py) hold each other, whatever the order in which the peeling one visits
the anchors, and every hand-made case shows what its name says: the degrees, the tip lengths, the spared anchors, the reads removed and the
rounds run are asserted from the case's own input.  These tests hold the yardstick of tests/test_gpu_tips.py; they do not run the library,
except for the last one, which checks that the binding declares the call."""
import ctypes as C

import numpy as np
import pytest

import contig_util as cu
import tip_util as tu
from elba_amd import capi

CASES = tu.hand_cases()


def _S(case, seed=0, extra=0):
    M, rows, cols, vals = tu.case_overlaps(case, np.random.default_rng(seed), extra)
    return (M,) + tuple(tu.symmetric_of(rows, cols, vals))


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_case_shows_what_its_name_says(name):
    case = CASES[name]
    M, rows, cols, vals = _S(case)
    deg = np.bincount(cols, minlength=M)
    for v, d in case["deg"].items():
        assert deg[v] == d, (name, v)
    trace = []
    r, c, v, flags, st = tu.clip_tips(M, rows, cols, vals, case["max"], case["rounds"], trace=trace)
    tips, spared = trace[0]
    assert sorted(len(chain) for _, chain, _ in tips) == case["tip_lengths"]
    assert all(deg[v1] == 1 and deg[b] >= 3 and all(deg[x] == 2 for x in chain[1:]) for v1, chain, b in tips)
    assert spared == case["spared"] and all(deg[b] == sum(1 for t in tips if t[2] == b) for b in spared)
    assert set(np.flatnonzero(flags == 4).tolist()) == case["removed"] and set(np.flatnonzero(flags).tolist()) == case["removed"]
    assert st["rounds_run"] == case["rounds_run"] and st["reads_removed"] == len(case["removed"])
    assert st["dead_ends"] == int((deg == 1).sum()) and st["nnz_before"] == len(rows) and st["nnz_after"] == len(r)
    after = np.bincount(c, minlength=M)
    for x, d in case["deg_after"].items():
        assert after[x] == d, (name, x)
    # the survivors are the input's entries without the removed reads', in the input's order
    keep = ~np.isin(rows, list(case["removed"])) & ~np.isin(cols, list(case["removed"]))
    assert (r == rows[keep]).all() and (c == cols[keep]).all() and v.tobytes() == vals[keep].tobytes()
    assert st["entries_removed"] == int((~keep).sum())
    if "star" in name:
        assert st["spared_anchors"] == 1 and st["reads_removed"] == 0 and st["tips"] == len(case["tip_lengths"])
    if name == "plain_path":
        assert st["tips"] == 0 and st["dead_ends"] == 2


@pytest.mark.parametrize("name", sorted(CASES))
def test_peeling_one_tip_at_a_time_gives_the_same_on_hand_cases(name):
    case = CASES[name]
    M, rows, cols, vals = _S(case, extra=3)
    want = tu.clip_tips(M, rows, cols, vals, case["max"], case["rounds"])
    for seed in range(3):
        order = np.random.default_rng(seed).permutation(M)
        assert tu.same(want, tu.clip_tips_peel(M, rows, cols, vals, case["max"], case["rounds"], order=order)), (name, seed)
    assert tu.same(want, tu.clip_tips_peel(M, rows, cols, vals, case["max"], case["rounds"]))


@pytest.mark.parametrize("block", range(6))
def test_peeling_gives_the_same_on_random_graphs(block):
    removed = rounds_seen = 0
    for seed in range(50):
        rng = np.random.default_rng(1000 * block + seed)
        M = int(rng.integers(2, 120))
        lens = rng.integers(20, 41, M)
        rows, cols, vals = cu.random_string_graph(rng, M, lens, n_paths=int(rng.integers(1, M // 3 + 2)), p_extra=float(rng.choice([0.05, 0.15, 0.4])))
        S = tu.symmetric_of(rows, cols, vals)
        mx, rounds = int(rng.choice([1, 2, 3, 7, 50])), int(rng.choice([1, 2, 5, 64]))
        want = tu.clip_tips(M, *S, mx, rounds)
        assert tu.same(want, tu.clip_tips_peel(M, *S, mx, rounds, order=rng.permutation(M))), (block, seed)
        st = want[4]
        assert st["rounds_run"] <= rounds and st["nnz_after"] == len(want[0]) and st["reads_removed"] == int((want[3] == 4).sum())
        removed += st["reads_removed"]; rounds_seen = max(rounds_seen, st["rounds_run"])
    assert removed > 0 and rounds_seen >= 2                    # the random graphs do have tips, and tips on tips


def test_a_second_clip_of_a_clipped_graph_removes_nothing():
    for name, case in CASES.items():
        M, rows, cols, vals = _S(case)
        r, c, v, _, st = tu.clip_tips(M, rows, cols, vals, case["max"], 64)
        again = tu.clip_tips(M, r, c, v, case["max"], 64)
        assert again[4]["reads_removed"] == 0 and again[4]["rounds_run"] == 1 and len(again[0]) == len(r), name


def test_planted_tips_are_what_the_restatement_removes():
    rng = np.random.default_rng(5)
    g = tu.Graph()
    path = g.chain(g.new(40))
    M, rows, cols, vals = g.overlaps(rng)
    anchors, lengths = [5, 11, 20, 33], [1, 2, 3, 1]
    M2, r2, c2, v2, planted = tu.plant_tips(rng, M, rows, cols, vals, anchors, lengths)
    assert M2 == M + sum(lengths) and len(planted) == sum(lengths)
    S = tu.symmetric_of(r2, c2, v2)
    r, c, v, flags, st = tu.clip_tips(M2, *S, 3, 2)
    assert set(np.flatnonzero(flags).tolist()) == set(planted.tolist()) and st["tips"] == 4 and st["rounds_run"] == 2
    base = tu.symmetric_of(rows, cols, vals)
    assert (r == base[0]).all() and (c == base[1]).all() and v.tobytes() == base[2].tobytes()
    assert path[0] == 0


def test_binding_declares_clip_tips():
    assert "elba_clip_tips" in capi.EXPORTED_SYMBOLS
    assert C.sizeof(capi.TipCfg) == 16 and C.sizeof(capi.TipStats) == 8 * 8 + 2 * 4 + 2 * 4
    import elba_amd
    assert hasattr(elba_amd.load_library(), "elba_clip_tips") and hasattr(elba_amd.Engine, "clip_tips")
