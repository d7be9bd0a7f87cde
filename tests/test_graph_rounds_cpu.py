"""CPU: every claim that tests/test_gpu_graph_rounds.py rests on, from the restatements (tip_util, bubble_util, weak_util) alone.  The
graphs of rounds_util.py take the number of rounds their names say, in closed form; the two statements of each rule agree on them; the
forests' S falls across tile edges of the compaction between two rounds; and the random sets hold what they are drawn for.  A graph that
does not show what the GPU test names it for fails here first.  Nothing here runs the library."""
import numpy as np
import pytest

import bubble_util as bu
import rounds_util as ru
import tip_util as tu
import weak_util as wu

B = ru.SG_BATCH


def _S(g, seed, perm=None):
    M, rows, cols, vals = g.overlaps(np.random.default_rng(seed), perm=perm)
    return (M,) + tuple(tu.symmetric_of(rows, cols, vals))


def test_the_named_round_counts_follow_the_protocol_s_constants():
    assert B == 4 and ru.SG_MAX_ROUNDS == 64 and ru.SG_TILE == 256 and ru.SCAN_TILE == 2048
    assert ru.TREE_DEPTHS == (3, 4, 5, 7, 8, 9) and ru.NEST_DEPTHS == (3, 4, 5, 8, 9, 63, 64, 65)
    # moves that end in the second buffer (odd) and in the first (even), inside a batch, at its edge and past it; rounds that run out in
    # the middle of the second batch (D - 1, D, D + 1 round 2 B - 1 .. 2 B + 1)
    assert {D % 2 for D in ru.TREE_DEPTHS} == {0, 1} and any(B < D < 2 * B for D in ru.TREE_DEPTHS) and max(ru.TREE_DEPTHS) > 2 * B


@pytest.mark.parametrize("D", ru.TREE_DEPTHS)
def test_a_tip_tree_goes_one_level_per_round(D):
    g, cyc, levels = ru.tree_on_cycle(D)
    assert [len(lv) for lv in levels] == [2 ** k for k in range(D)] and g.n == 6 + 2 ** D - 1
    M, rows, cols, vals = _S(g, D)
    assert len(rows) == 2 * M                                   # a tree on a cycle: as many pairs as reads
    for rounds in (64, D - 1, D, D + 1):
        trace = []
        want = tu.clip_tips(M, rows, cols, vals, 1, rounds, trace=trace)
        st = want[4]
        assert st["rounds_run"] == ru.rounds_run(D, rounds) == (D + 1 if rounds > D else rounds)
        assert st["reads_removed"] == ru.tree_reads_removed(D, rounds) and st["spared_anchors"] == 0
        for k in range(min(D, rounds)):                         # round k takes level D - k, whole
            tips, spared = trace[k]
            assert {t[0] for t in tips} == set(levels[D - 1 - k]) and all(len(t[1]) == 1 for t in tips) and not spared
        left = set(range(M)) - set(np.flatnonzero(want[3]).tolist())
        assert left == set(cyc) | {v for lv in levels[:max(D - rounds, 0)] for v in lv}
        if rounds == D - 1:
            assert left - set(cyc) == set(levels[0])            # one read stays behind
        assert tu.same(want, tu.clip_tips_peel(M, rows, cols, vals, 1, rounds, order=np.random.default_rng(D).permutation(M)))


def test_the_tip_tree_of_depth_10():
    g, cyc, levels = ru.tree_on_cycle(10)
    M, rows, cols, vals = _S(g, 10)
    st = tu.clip_tips(M, rows, cols, vals, 1, 64)[4]
    assert M == 1029 and st["rounds_run"] == 11 and st["reads_removed"] == 1023


@pytest.mark.parametrize("d", ru.NEST_DEPTHS)
def test_nested_bubbles_go_one_read_per_round(d):
    g, goes, ends = ru.nest(d)
    assert g.n == 5 * d + 10 and len(goes) == d
    M, rows, cols, vals = _S(g, d, perm=np.random.default_rng(d + 1).permutation(g.n))
    perm = np.random.default_rng(d + 1).permutation(g.n)
    for rounds in sorted({64, min(d - 1, 64), min(d, 64), min(d + 1, 64)}):
        trace = []
        want = bu.pop_bubbles(M, rows, cols, vals, ru.MAX_ARM, rounds, trace=trace)
        st = want[4]
        moving = min(d, rounds)
        assert st["rounds_run"] == ru.rounds_run(d, rounds) and st["reads_removed"] == moving == st["bubbles"] == st["arms_removed"]
        for k in range(moving):                                 # round k takes the k-th innermost bubble's one-read arm
            arms, gone = trace[k]
            assert [a[2] for a in gone] == [(int(perm[goes[k]]),)]
        assert set(np.flatnonzero(want[3]).tolist()) == {int(perm[v]) for v in goes[:moving]}
        assert tu.same(want, bu.pop_bubbles_chains(M, rows, cols, vals, ru.MAX_ARM, rounds, order=np.random.default_rng(d).permutation(M)))
    if d == ru.SG_MAX_ROUNDS + 1:                               # one bubble left: a second call of one round pops it, a third finds nothing
        r1 = bu.pop_bubbles(M, rows, cols, vals, ru.MAX_ARM, 64)
        r2 = bu.pop_bubbles(M, r1[0], r1[1], r1[2], ru.MAX_ARM, 1)
        assert r2[4]["reads_removed"] == 1 and r2[4]["bubbles"] == 1 and r2[4]["rounds_run"] == 1
        r3 = bu.pop_bubbles(M, r2[0], r2[1], r2[2], ru.MAX_ARM, 64)
        assert r3[4]["reads_removed"] == 0 and r3[4]["rounds_run"] == 1 and len(r3[0]) == len(r2[0])


def test_the_cap_of_64_rounds_on_nests_of_63_64_and_65():
    got = {}
    for d in (63, 64, 65):
        g, goes, ends = ru.nest(d)
        M, rows, cols, vals = _S(g, d)
        st = bu.pop_bubbles(M, rows, cols, vals, ru.MAX_ARM, 64)[4]
        got[d] = (st["rounds_run"], st["reads_removed"])
    assert got == {63: (64, 63), 64: (64, 64), 65: (64, 64)}


def test_the_tip_forest_spans_many_tiles_and_falls_across_their_edges():
    g, perm = ru.tip_forest()
    M, rows, cols, vals = _S(g, 1, perm=perm)
    assert M == 10108 and len(rows) == 20216 and len(rows) > 9 * ru.SCAN_TILE and (len(rows) + ru.SG_TILE - 1) // ru.SG_TILE == 79
    want = {3: (5367, 3), 4: (5748, 4), 5: (5937, 5), 8: (6096, 8), 9: (6105, 9), 64: (6108, 11)}
    assert tuple(sorted(want)) == ru.FOREST_ROUNDS
    for rounds, (removed, run) in want.items():
        res = tu.clip_tips(M, rows, cols, vals, 1, rounds)
        assert (res[4]["reads_removed"], res[4]["rounds_run"]) == (removed, run) and removed == ru.forest_tree_reads_removed(rounds)
        if rounds in (5, 64):
            assert tu.same(res, tu.clip_tips_peel(M, rows, cols, vals, 1, rounds, order=np.random.default_rng(rounds).permutation(M)))
    nnz = ru.per_round_nnz(tu.clip_tips, M, rows, cols, vals, 1, 64)
    assert nnz == [2 * (M - ru.forest_tree_reads_removed(k)) for k in range(11)] and nnz[-1] == 8000
    # every one of the first six moves drops scatter tiles, four of them scan tiles too: on both sides of the first batch's read-back
    assert ru.edges_crossed(nnz, ru.SG_TILE) == [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 6)]
    assert ru.edges_crossed(nnz, ru.SCAN_TILE) == [(0, 1), (1, 2), (2, 3), (5, 6)]
    # the reads of one tree are spread over the columns
    deep = perm[g.n - 1023:]                                    # the last tree, of depth 10
    assert deep.max() - deep.min() > M // 2 and len(set((deep // 128).tolist())) > 64


def test_the_bubble_forest_falls_across_a_scan_tile_edge_in_its_first_round():
    g, perm = ru.bubble_forest()
    M, rows, cols, vals = _S(g, 1, perm=perm)
    assert M == 1480 + sum(5 * d + 10 for d in range(1, 13)) and len(rows) == 2 * ru.SCAN_TILE + 40
    for rounds in ru.FOREST_ROUNDS:
        res = bu.pop_bubbles(M, rows, cols, vals, ru.MAX_ARM, rounds)
        assert res[4]["reads_removed"] == sum(min(d, rounds) for d in range(1, 13)) and res[4]["rounds_run"] == ru.rounds_run(12, rounds)
        assert tu.same(res, bu.pop_bubbles_chains(M, rows, cols, vals, ru.MAX_ARM, rounds, order=np.random.default_rng(rounds).permutation(M)))
    nnz = ru.per_round_nnz(bu.pop_bubbles, M, rows, cols, vals, ru.MAX_ARM, 64)
    assert nnz == [len(rows) - 4 * sum(min(d, k) for d in range(1, 13)) for k in range(13)]      # a popped read takes its two pairs
    assert ru.edges_crossed(nnz, ru.SCAN_TILE) == [(0, 1)] and ru.edges_crossed(nnz, ru.SG_TILE) == [(0, 1), (9, 10)]


def test_the_mixed_forest_needs_more_than_a_batch_of_tip_rounds_in_its_first_pass():
    g, perm = ru.mixed_forest()
    M, rows, cols, vals = _S(g, 1, perm=perm)
    passes = bu.simplify(M, rows, cols, vals, 1, ru.MAX_ARM)[4]
    assert len(passes) == 2 and passes[0][0]["rounds_run"] == B + 3 > B and passes[0][0]["reads_removed"] == sum(2 ** D - 1 for D in range(1, B + 3))
    assert passes[0][1]["rounds_run"] == 4 and passes[0][1]["reads_removed"] == 6
    assert passes[1][0]["reads_removed"] == 0 and passes[1][1]["reads_removed"] == 0


@pytest.mark.parametrize("kind", ["tips", "bubbles"])
@pytest.mark.parametrize("moves", [B, B + 1])
def test_what_is_left_after_4_and_5_moves_has_work_for_the_later_stages(kind, moves):
    M, rows, cols, vals = ru.moving_rounds(kind, moves, 10 * moves + len(kind))
    S = wu.S_of(rows, cols, vals)
    assert len(S[0]) == 2 * len(rows)
    first = tu.clip_tips(M, *S, 1, 64) if kind == "tips" else bu.pop_bubbles(M, *S, ru.MAX_ARM, 64)
    assert first[4]["rounds_run"] == moves + 1 and first[4]["reads_removed"] == (2 ** moves - 1 if kind == "tips" else moves)
    cut = wu.cut_weak(M, first[0], first[1], first[2], wu.Q07)
    assert cut[3]["entries_removed"] == 6 and cut[3]["weak_entries"] == 3 and cut[3]["sides_emptied"] == 3      # the three overlaps of score 60
    again = tu.clip_tips(M, cut[0], cut[1], cut[2], 3, 64)       # two arms of three reads beside the arm of eight, at every star
    assert again[4]["reads_removed"] == 18 and again[4]["tips"] == 6 and again[4]["rounds_run"] == 2 and again[4]["spared_anchors"] == 0
    if kind == "bubbles":                                       # a second pop finds the nest gone
        assert bu.pop_bubbles(M, cut[0], cut[1], cut[2], ru.MAX_ARM, 64)[4]["bubbles"] == 0


def test_the_random_graphs_for_tips_remove_reads_in_several_rounds():
    later = spared = 0
    for seed in ru.TIP_SEEDS:
        M, rows, cols, vals, mx, rounds = ru.random_graph(seed)
        assert 2 <= M <= 3000
        S = tu.symmetric_of(rows, cols, vals)
        want = tu.clip_tips(M, *S, mx, rounds)
        nnz = ru.per_round_nnz(tu.clip_tips, M, *S, mx, rounds)
        later += len(nnz) >= 3                                  # removed reads in at least two different rounds
        spared += want[4]["spared_anchors"]
        if seed % 4 == 0:
            assert tu.same(want, tu.clip_tips_peel(M, *S, mx, rounds, order=np.random.default_rng(seed).permutation(M)))
    assert later >= 5 and spared > 0 and len(ru.TIP_SEEDS) == 24


def test_the_random_graphs_for_bubbles_pop_some():
    popped = two_rounds = 0
    for seed in ru.BUBBLE_SEEDS:
        M, rows, cols, vals, mx, rounds = ru.random_graph(seed)
        S = tu.symmetric_of(rows, cols, vals)
        want = bu.pop_bubbles(M, *S, mx, rounds)
        popped += want[4]["bubbles"]; two_rounds += want[4]["rounds_run"] >= 2
        if seed % 4 == 0:
            assert tu.same(want, bu.pop_bubbles_chains(M, *S, mx, rounds, order=np.random.default_rng(seed).permutation(M)))
    assert popped >= 10 and two_rounds >= 3 and len(ru.BUBBLE_SEEDS) == 24


def test_the_random_S_for_the_weak_cut_holds_every_clause():
    ties = low_best = one_image = mirror_only = 0
    seen_q = set()
    for seed in ru.WEAK_SEEDS:
        (M, rows, cols, vals), S, q16 = ru.random_weak(seed)
        seen_q.add(q16)
        trace = {}
        got = wu.cut_weak(M, S[0], S[1], S[2], q16, trace)
        if M < 400:
            assert wu.same(got, wu.cut_weak_sorted(M, S[0], S[1], S[2], q16))
        one_image += 2 * len(rows) - len(S[0])                  # pairs that keep one image
        low_best += sum(1 for k, b in trace["best"].items() if b <= 0 and trace["cnt"][k] >= 2)
        mirror_only += sum(1 for (r, c) in trace["removed"] if (r, c) not in trace["weak"])
        side = S[2]["direction"] & 1
        for r, c, e, s in zip(S[0].tolist(), S[1].tolist(), side.tolist(), S[2]["score"].tolist()):
            k = (c, e)
            ties += trace["cnt"][k] >= 2 and trace["best"][k] > 0 and s * 65536 == q16 * trace["best"][k]      # at the threshold: stays
    assert ties > 0 and low_best > 0 and one_image > 0 and mirror_only > 0
    assert seen_q == set(ru.RATIOS_Q16) == {wu.q16_of(x) for x in (1 / 65536, 0.5, 0.7, 1.0)} and len(ru.WEAK_SEEDS) == 24


def test_simplify_takes_2_or_3_passes_on_the_random_graphs():
    n = []
    for seed in ru.SIMPLIFY_SEEDS:
        M, rows, cols, vals, mx, ma = ru.random_scored(seed)
        n.append(len(bu.simplify(M, *tu.symmetric_of(rows, cols, vals), mx, ma)[4]))
    assert set(n) <= {2, 3} and len(n) == 12
    n = []
    for seed in ru.SIMPLIFY_WEAK_SEEDS:
        M, rows, cols, vals, mx, ma = ru.random_scored(seed)
        n.append(len(wu.simplify(M, *wu.S_of(rows, cols, vals), mx, ma, wu.Q07)[4]))
    assert set(n) == {2, 3} and len(n) == 12
