"""-m gpu: the round protocol of elba_amd/csrc/sg_rounds.hpp past its first batch of SG_BATCH rounds, and the three cleaning calls
(elba_clip_tips, elba_pop_bubbles, elba_cut_weak_overlaps) and Engine.simplify_graph on random graphs, against the restatements of
tip_util.py, bubble_util.py and weak_util.py: every entry of S in order, every byte of every value, the read flags and every stat, exactly.

The graphs of rounds_util.py take a chosen number of rounds: a tip_tree of depth D moves S D times, nested_bubbles(d) d times.  With D and d
round SG_BATCH, twice SG_BATCH and the cap of SG_MAX_ROUNDS, the host loop of sg_run_rounds goes round again, S ends in either buffer after
moves inside a batch, at its edge and past it, `rounds` runs out in the middle of a batch, and the counters reach their last slots.
tests/test_graph_rounds_cpu.py asserts what each graph is named for from the restatements alone.  Graphs are loaded with elba_set_overlaps
with suffixes in [5, 9], which the reduction keeps at fuzz 0; each load asserts that."""
import functools

import numpy as np
import pytest

import bubble_util as bu
import contig_ex_util as cx
import contig_util as cu
import elba_amd
import rounds_util as ru
import tip_util as tu
import weak_util as wu

pytestmark = pytest.mark.gpu

B = ru.SG_BATCH
CONTIG_STATS = ("nreads", "branches", "components", "used_components", "contigs", "cycles", "contig_reads", "bases", "longest")


def _same_S(g, rows, cols, vals):
    assert g["n"] == len(rows) and (g["rows"] == rows).all() and (g["cols"] == cols).all()
    assert g["vals"].tobytes() == np.asarray(vals).tobytes()


def _load(e, M, rows, cols, vals, exact=False):
    e.set_overlaps(M, rows, cols, vals)
    s = e.transitive_reduction(0.0, 0)
    if exact:                                                   # one-image pairs included
        _same_S(e.export_string_graph(), *wu.S_of(rows, cols, vals))
    else:
        assert s["nnz"] == 2 * len(rows)                        # the reduction keeps the graph as built
    return s


def _clip(e, M, mx, rounds):
    """clip_tips on the engine's S equals the restatement on the S exported before the call.  Returns (stats, restatement's result)."""
    g = e.export_string_graph()
    f0 = e.export_read_flags(M)
    want = tu.clip_tips(M, g["rows"], g["cols"], g["vals"], mx, rounds)
    st = e.clip_tips(mx, rounds)
    for k in tu.STATS:
        assert st[k] == want[4][k], (k, st, want[4])
    _same_S(e.export_string_graph(), want[0], want[1], want[2])
    assert (e.export_read_flags(M) == (f0 | want[3])).all()
    return st, want


def _pop(e, M, mx, rounds):
    g = e.export_string_graph()
    f0 = e.export_read_flags(M)
    want = bu.pop_bubbles(M, g["rows"], g["cols"], g["vals"], mx, rounds)
    st = e.pop_bubbles(mx, rounds)
    for k in bu.STATS:
        assert st[k] == want[4][k], (k, st, want[4])
    _same_S(e.export_string_graph(), want[0], want[1], want[2])
    assert (e.export_read_flags(M) == (f0 | want[3])).all()
    return st, want


def _cut(e, M, q16):
    g = e.export_string_graph()
    f0 = e.export_read_flags(M)
    want = wu.cut_weak(M, g["rows"], g["cols"], g["vals"], q16)
    st = e.cut_weak_overlaps(q16 / 65536)                       # exact: q16 / 65536 * 65536 is q16 again
    for k in wu.STATS:
        assert st[k] == want[3][k], (k, st, want[3])
    _same_S(e.export_string_graph(), want[0], want[1], want[2])
    assert (e.export_read_flags(M) == f0).all()
    return st, want


def _contigs(e, M, seqs):
    """generate_contigs(circular, singletons) equals contig_ex_util on the exported S and read flags: every contig, chain, kind and count."""
    g = e.export_string_graph()
    flags = cx.CIRCULAR | cx.SINGLETONS
    contigs, chains, kinds, read_contig, want = cx.generate_contigs_ex(M, g["rows"], g["cols"], g["vals"], seqs, flags, e.export_read_flags(M))
    st = e.generate_contigs(circular=True, singletons=True)
    for k in CONTIG_STATS:
        assert st[k] == want[k], (k, st, want)
    got = e.export_contigs()
    assert got["n"] == len(contigs) and got["seqs"] == contigs and got["kinds"].tolist() == kinds
    flat = [el for ch in chains for el in ch]
    assert got["chain_off"].tolist() == np.concatenate([[0], np.cumsum([len(c) for c in chains])]).tolist()
    assert got["chain_read"].tolist() == [r for r, _, _ in flat] and got["chain_prefix"].tolist() == [p for _, p, _ in flat]
    assert got["chain_strand"].tolist() == [s for _, _, s in flat]
    assert (e.export_read_contigs(M) == np.array(read_contig, dtype=np.int64)).all()
    return st, kinds


@pytest.fixture(scope="module")
def eng():
    e = elba_amd.Engine(17, 2, 8)
    yield e
    e.close()


# --- (a) depth against SG_BATCH, tips ---

@functools.lru_cache(maxsize=None)
def _tree(D):
    g = ru.tree_on_cycle(D)[0]
    return g.overlaps(np.random.default_rng(D), perm=np.random.default_rng(D + 100).permutation(g.n))


@pytest.mark.parametrize("rounds", ["64", "D-1", "D", "D+1"])
@pytest.mark.parametrize("D", ru.TREE_DEPTHS)
def test_tip_trees_of_depths_round_the_batch(eng, D, rounds):
    rounds = {"64": 64, "D-1": D - 1, "D": D, "D+1": D + 1}[rounds]
    M, rows, cols, vals = _tree(D)
    _load(eng, M, rows, cols, vals)
    st, _ = _clip(eng, M, 1, rounds)
    assert st["rounds_run"] == (D + 1 if rounds > D else rounds) and st["reads_removed"] == 2 ** D - 2 ** max(D - rounds, 0)
    assert st["nnz_after"] == 2 * (M - st["reads_removed"]) and eng.export_read_flags(M).sum() == 4 * st["reads_removed"]


# --- (b) depth against SG_BATCH and the cap, bubbles ---

@functools.lru_cache(maxsize=None)
def _nest(d):
    g = ru.nest(d)[0]
    return g.overlaps(np.random.default_rng(d), perm=np.random.default_rng(d + 100).permutation(g.n))


@pytest.mark.parametrize("d,rounds", [(d, 64) for d in ru.NEST_DEPTHS] + [(2 * B + 1, r) for r in (2 * B, 2 * B + 1, 2 * B + 2)])
def test_nested_bubbles_of_depths_round_the_batch_and_the_cap(eng, d, rounds):
    M, rows, cols, vals = _nest(d)
    assert M == 5 * d + 10
    _load(eng, M, rows, cols, vals)
    st, _ = _pop(eng, M, ru.MAX_ARM, rounds)
    moving = min(d, rounds)
    assert st["rounds_run"] == (moving + 1 if rounds > moving else rounds) and st["reads_removed"] == moving == st["bubbles"]
    assert st["nnz_after"] == 2 * len(rows) - 4 * moving and eng.export_read_flags(M).sum() == 8 * moving


def test_the_bubble_left_at_the_cap_goes_in_a_second_call(eng):
    d = ru.SG_MAX_ROUNDS + 1
    M, rows, cols, vals = _nest(d)
    _load(eng, M, rows, cols, vals)
    st, _ = _pop(eng, M, ru.MAX_ARM, ru.SG_MAX_ROUNDS)
    assert st["rounds_run"] == ru.SG_MAX_ROUNDS and st["reads_removed"] == ru.SG_MAX_ROUNDS        # an even number of moves, the last counters in the last slots
    st, _ = _pop(eng, M, ru.MAX_ARM, 1)
    assert st["reads_removed"] == 1 and st["bubbles"] == 1 and st["rounds_run"] == 1 and st["anchors"] == 2
    before = eng.export_string_graph()
    f = eng.export_read_flags(M)
    st, _ = _pop(eng, M, ru.MAX_ARM, ru.SG_MAX_ROUNDS)
    assert st["reads_removed"] == 0 and st["anchors"] == 0 and st["rounds_run"] == 1 and st["nnz_after"] == st["nnz_before"] == before["n"]
    _same_S(eng.export_string_graph(), before["rows"], before["cols"], before["vals"])
    assert (eng.export_read_flags(M) == f).all() and f.sum() == 8 * d


# --- (c) the forests: an S of many tiles whose nnz falls across tile edges while the launches stay sized by the first nnz ---

@functools.lru_cache(maxsize=None)
def _forest(which):
    g, perm = getattr(ru, which)()
    return g.overlaps(np.random.default_rng(1), perm=perm)


@pytest.mark.parametrize("rounds", ru.FOREST_ROUNDS)
def test_tip_forest_over_79_scatter_tiles(eng, rounds):
    """Per round the restatement's nnz is 20216, 14078, 11012, 9482, 8720, 8342, 8156, 8066, 8024, 8006, 8000: the tiles of k_sg_scatter
    (256 entries) that hold entries fall between every two of the first seven rounds, the scan's (2048) between rounds 0 - 1, 1 - 2, 2 - 3 and
    5 - 6, on both sides of the first batch's read-back."""
    M, rows, cols, vals = _forest("tip_forest")
    _load(eng, M, rows, cols, vals)
    st, _ = _clip(eng, M, 1, rounds)
    want = {3: (5367, 3), 4: (5748, 4), 5: (5937, 5), 8: (6096, 8), 9: (6105, 9), 64: (6108, 11)}[rounds]
    assert (st["reads_removed"], st["rounds_run"]) == want and st["nnz_before"] == 20216
    if rounds == 64:
        S = wu.S_of(rows, cols, vals)
        nnz = ru.per_round_nnz(tu.clip_tips, M, S[0], S[1], S[2], 1, 64)
        assert nnz[0] == st["nnz_before"] and nnz[-1] == st["nnz_after"] and len(nnz) == st["rounds_run"]
        assert ru.edges_crossed(nnz, ru.SG_TILE) and ru.edges_crossed(nnz, ru.SCAN_TILE)
        assert any(r >= B for r, _ in ru.edges_crossed(nnz, ru.SCAN_TILE))                    # one of them behind the first batch


@pytest.mark.parametrize("rounds", ru.FOREST_ROUNDS)
def test_bubble_forest_of_nests_1_to_12(eng, rounds):
    """Per round the restatement's nnz is 4136, 4088, 4044, ..: the first round takes S below two scan tiles (4096, a scatter-tile edge too),
    and rounds 9 - 10 cross the scatter-tile edge at 3840, in the third batch."""
    M, rows, cols, vals = _forest("bubble_forest")
    _load(eng, M, rows, cols, vals)
    st, _ = _pop(eng, M, ru.MAX_ARM, rounds)
    assert st["reads_removed"] == sum(min(d, rounds) for d in range(1, 13)) and st["rounds_run"] == (13 if rounds > 12 else rounds)
    if rounds == 64:
        S = wu.S_of(rows, cols, vals)
        nnz = ru.per_round_nnz(bu.pop_bubbles, M, S[0], S[1], S[2], ru.MAX_ARM, 64)
        assert nnz[0] == st["nnz_before"] and nnz[-1] == st["nnz_after"] and len(nnz) == st["rounds_run"]
        assert ru.edges_crossed(nnz, ru.SCAN_TILE) == [(0, 1)] and (9, 10) in ru.edges_crossed(nnz, ru.SG_TILE)


# --- (d) what comes after an odd and an even number of moves ---

@pytest.mark.parametrize("kind", ["tips", "bubbles"])
@pytest.mark.parametrize("moves", [B, B + 1])
def test_later_stages_read_the_buffer_S_ended_in(kind, moves):
    M, rows, cols, vals = ru.moving_rounds(kind, moves, 10 * moves + len(kind))
    rng = np.random.default_rng(moves)
    packed, off, lens = cu.random_packed(rng, M, 20, 40)
    seqs = cu.seqs_of(packed, off, lens)
    e = elba_amd.Engine(17, 2, 8)
    e.set_reads(packed, off, lens)
    _load(e, M, rows, cols, vals, exact=True)
    st, _ = _clip(e, M, 1, 64) if kind == "tips" else _pop(e, M, ru.MAX_ARM, 64)
    assert st["rounds_run"] == moves + 1 and st["reads_removed"] == (2 ** moves - 1 if kind == "tips" else moves)      # `moves` moves of S
    cs, kinds = _contigs(e, M, seqs)
    assert cs["branches"] >= 3 and (cx.CIRCLE in kinds) == (kind == "tips") and cx.SINGLE in kinds
    ws, _ = _cut(e, M, wu.Q07)
    assert ws["entries_removed"] == 6 and ws["weak_entries"] == 3
    _contigs(e, M, seqs)
    ts, _ = _clip(e, M, 3, 64)                                  # a second call, of either kind
    assert ts["reads_removed"] == 18 and ts["rounds_run"] == 2
    bs, _ = _pop(e, M, ru.MAX_ARM, 64)
    assert bs["reads_removed"] == 0 and bs["rounds_run"] == 1
    cs, _ = _contigs(e, M, seqs)
    assert cs["branches"] == 0
    # a larger graph, then a smaller one, on the same context
    M2, r2, c2, v2 = _forest("mixed_forest")
    assert M2 > M
    _load(e, M2, r2, c2, v2)
    st, _ = _clip(e, M2, 1, 64) if kind == "tips" else _pop(e, M2, ru.MAX_ARM, 64)
    assert st["rounds_run"] == (B + 3 if kind == "tips" else 4)
    M3, r3, c3, v3 = _tree(B - 1) if kind == "tips" else _nest(B - 1)
    assert M3 < M
    _load(e, M3, r3, c3, v3)
    st, _ = _clip(e, M3, 1, 64) if kind == "tips" else _pop(e, M3, ru.MAX_ARM, 64)
    assert st["rounds_run"] == B
    e.close()


# --- (e) random graphs through each call ---

@pytest.mark.parametrize("seed", ru.TIP_SEEDS)
def test_clip_tips_on_random_graphs(eng, seed):
    M, rows, cols, vals, mx, rounds = ru.random_graph(seed)
    _load(eng, M, rows, cols, vals)
    _clip(eng, M, mx, rounds)


@pytest.mark.parametrize("seed", ru.BUBBLE_SEEDS)
def test_pop_bubbles_on_random_graphs(eng, seed):
    M, rows, cols, vals, mx, rounds = ru.random_graph(seed)
    _load(eng, M, rows, cols, vals)
    _pop(eng, M, mx, rounds)


@pytest.mark.parametrize("seed", ru.WEAK_SEEDS)
def test_cut_weak_overlaps_on_random_S(eng, seed):
    (M, rows, cols, vals), S, q16 = ru.random_weak(seed)
    _load(eng, M, rows, cols, vals, exact=True)
    _cut(eng, M, q16)
    st, _ = _cut(eng, M, q16)                                   # the pass is its own fixed point
    assert st["entries_removed"] == 0


# --- (f) simplify_graph on random graphs ---

def _simplify(e, M, rows, cols, vals, mx, ma, q16=None):
    _load(e, M, rows, cols, vals)
    S = e.export_string_graph()
    if q16 is None:
        want = bu.simplify(M, S["rows"], S["cols"], S["vals"], mx, ma)
        got = e.simplify_graph(mx, ma)
    else:
        want = wu.simplify(M, S["rows"], S["cols"], S["vals"], mx, ma, q16)
        got = e.simplify_graph(mx, ma, min_overlap_ratio=q16 / 65536)
    assert len(got) == len(want[4])                             # the number of passes
    for p, wp in zip(got, want[4]):
        assert len(p) == len(wp)
        for s, ws, keys in zip(p, wp, (tu.STATS, bu.STATS, wu.STATS)):
            for k in keys:
                assert s[k] == ws[k], (k, s, ws)
    _same_S(e.export_string_graph(), want[0], want[1], want[2])
    assert (e.export_read_flags(M) == want[3]).all()
    return got


@pytest.mark.parametrize("seed", ru.SIMPLIFY_SEEDS)
def test_simplify_graph_on_random_graphs(eng, seed):
    M, rows, cols, vals, mx, ma = ru.random_scored(seed)
    assert len(_simplify(eng, M, rows, cols, vals, mx, ma)) in (2, 3)


@pytest.mark.parametrize("seed", ru.SIMPLIFY_WEAK_SEEDS)
def test_simplify_graph_with_a_ratio_on_random_graphs(eng, seed):
    M, rows, cols, vals, mx, ma = ru.random_scored(seed)
    assert len(_simplify(eng, M, rows, cols, vals, mx, ma, wu.Q07)) in (2, 3)


def test_simplify_graph_on_a_forest_whose_tips_need_more_than_a_batch(eng):
    M, rows, cols, vals = _forest("mixed_forest")
    got = _simplify(eng, M, rows, cols, vals, 1, ru.MAX_ARM)
    assert len(got) == 2 and got[0][0]["rounds_run"] == B + 3 and got[0][1]["rounds_run"] == 4 and got[0][1]["reads_removed"] == 6
