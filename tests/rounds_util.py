"""Graphs that keep the round protocol of elba_amd/csrc/sg_rounds.hpp busy for a chosen number of rounds, on tip_util.Graph, and the random
sets the GPU tests of the three cleaning calls draw.  Nothing here runs the library: test_graph_rounds_cpu.py asserts every count stated
below from the restatements (tip_util, bubble_util, weak_util) alone, and test_gpu_graph_rounds.py holds the library against them.

tip_tree          a complete binary tree of depth D hung off a read by its root: with max_tip_reads = 1 one level goes per round, leaves
                  first, for exactly D rounds (a parent of two leaves has degree 3 and two tips: it is not spared)
nested_bubbles    d bubbles one inside the other: with max_arm_reads = 65535 one read goes per round, innermost first, for exactly d rounds
forest            trees and nests of the given depths hung step reads apart on one cycle, under a random relabelling, so that the reads of
                  one structure are spread over the columns of S and every round moves an S of many tiles
moving_rounds     a tree or a nest beside stars of long arms, one of them on a weak overlap: what is left after the rounds still has work
                  for a cut of weak overlaps, a second clip and the contigs, on the buffer S ended in
per_round_nnz     nnz(S) as every round of a restatement finds it
random_graph, random_weak
                  the random graphs of test_tips_cpu.py, test_bubbles_cpu.py and test_weak_cpu.py at up to 3000 reads, with suffixes the
                  reduction keeps at fuzz 0"""
import os
import re

import numpy as np

import contig_util as cu
import tip_util as tu
import weak_util as wu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def const(path, name):
    m = re.search(r"constexpr int %s = (\d+);" % name, open(os.path.join(ROOT, "elba_amd", "csrc", path)).read())
    return int(m.group(1))


SG_BATCH = const("sg_rounds.hpp", "SG_BATCH")                   # rounds queued between two looks at the counters
SG_MAX_ROUNDS = const("sg_rounds.hpp", "SG_MAX_ROUNDS")
SG_TILE = const("sg_rounds.hpp", "SG_TILE")                     # entries one workgroup of k_sg_scatter moves
SG_THREADS = const("sg_rounds.hpp", "SG_THREADS")               # lanes per workgroup of the flat kernels
SCAN_TILE = const("prims.hip", "SCAN_THREADS") * const("prims.hip", "SCAN_ITEMS")     # elements one workgroup of the scan takes
B = SG_BATCH

TREE_DEPTHS = (B - 1, B, B + 1, 2 * B - 1, 2 * B, 2 * B + 1)
NEST_DEPTHS = (B - 1, B, B + 1, 2 * B, 2 * B + 1, SG_MAX_ROUNDS - 1, SG_MAX_ROUNDS, SG_MAX_ROUNDS + 1)
FOREST_ROUNDS = (3, 4, 5, 8, 9, 64)
MAX_ARM = 65535
TIP_MAX = (1, 2, 3, 7, 50)
ROUNDS = (1, 2, 5, 64)
RATIOS_Q16 = (1, 32768, wu.Q07, 65536)                          # 1 / 65536, 0.5, 0.7, 1.0


def tip_tree(g, anchor, D):
    """Hangs a complete binary tree of depth D off `anchor` by its root.  Returns its levels, the root's first: level k has 2^(k-1) reads."""
    levels = [g.arm(anchor, 1)]
    for _ in range(D - 1):
        nxt = []
        for p in levels[-1]:
            nxt += g.arm(p, 1) + g.arm(p, 1)
        levels.append(nxt)
    return levels


def tree_reads_removed(D, rounds):
    """Reads of a tip_tree of depth D that `rounds` rounds at max_tip_reads = 1 take: the deepest min(D, rounds) levels."""
    return 2 ** D - 2 ** max(D - rounds, 0)


def rounds_run(moving, rounds):
    """rounds_run of a call on a graph that loses something in `moving` rounds and then nothing: the round that finds nothing counts."""
    return moving + 1 if rounds > moving else rounds


def nested_bubbles(g, d, tails=(5, 5)):
    """a =(x | y1 y2)= b, wrapped d - 1 times as A - p - lo .. hi - q - B beside A - r - B, with dead-end tails on the outermost anchors.
    Returns (the read that goes in round 1, 2, .., d; the outermost anchors; the last read of the first tail, or None)."""
    a, x, y1, y2, b = g.new(5)
    g.chain([a, x, b]); g.chain([a, y1, y2, b])
    goes, lo, hi = [x], a, b
    for _ in range(d - 1):
        A, p, q, r, Bb = g.new(5)
        g.chain([A, p, lo]); g.chain([hi, q, Bb]); g.chain([A, r, Bb])
        goes.append(r)
        lo, hi = A, Bb
    end = g.arm(lo, tails[0])[-1] if tails[0] else None
    if tails[1]:
        g.arm(hi, tails[1])
    return goes, (lo, hi), end


def tree_on_cycle(D, graph=tu.Graph):
    """A tip_tree of depth D on a 6-cycle: M = 6 + 2^D - 1."""
    g = graph()
    cyc = g.chain(g.new(6), closed=True)
    levels = tip_tree(g, cyc[2], D)
    return g, cyc, levels


def nest(d, graph=tu.Graph):
    """nested_bubbles(d) alone: M = 5 d + 10."""
    g = graph()
    goes, ends, _ = nested_bubbles(g, d)
    return g, goes, ends


def forest(trees, bubbles, cycle_len, step, seed):
    """One cycle of cycle_len reads with a tip_tree per element of `trees` and a nest per element of `bubbles` (hung by the end of its first
    tail), at reads `step` apart.  Returns (graph, perm): perm, drawn from `seed`, renames the reads."""
    g = tu.Graph()
    cyc = g.chain(g.new(cycle_len), closed=True)
    assert step * (len(trees) + len(bubbles)) <= cycle_len
    at = 0
    for D in trees:
        tip_tree(g, cyc[at], D); at += step
    for d in bubbles:
        _, _, end = nested_bubbles(g, d)
        g.link(cyc[at], end); at += step
    return g, np.random.default_rng(seed).permutation(g.n)


def tip_forest():
    """A cycle of 4000 reads with three trees of each depth 1 .. 10, 37 reads apart: M = 10 108, nnz = 20 216."""
    return forest([D for D in range(1, 11) for _ in range(3)], [], 4000, 37, 71)


def bubble_forest():
    """A cycle of 1480 reads with nests of depth 1 .. 12, 37 reads apart: nnz = 4136, 40 above two scan tiles, and the first round takes 48."""
    return forest([], list(range(1, 13)), 1480, 37, 72)


def mixed_forest():
    """Trees of depth 1 .. B + 2 and nests of depth 1 .. 3 on one cycle: a pass of tips at max_tip_reads = 1 needs B + 2 > SG_BATCH rounds."""
    return forest(list(range(1, B + 3)), [1, 2, 3], 300, 23, 73)


def forest_tree_reads_removed(rounds):
    return 3 * sum(tree_reads_removed(D, rounds) for D in range(1, 11))


STAR_ARMS = ((3, 100), (3, 60), (3, 100), (8, 100))              # (reads, score of the overlap with the hub), all on one end of the hub


def moving_rounds(kind, moves, seed):
    """A tree on a 6-cycle (kind "tips") or a nest ("bubbles") that moves S `moves` times, beside three stars of STAR_ARMS, on a
    weak_util.WeakGraph (every overlap scores 100 and a read inside a chain has one on each end) under a random relabelling.  At
    max_tip_reads = 1 a star has no tip; a cut at 0.7 takes its overlap of score 60, and nothing else in the graph; then, at
    max_tip_reads = 3, its two arms of three reads still on the hub are tips beside the arm of eight.  Returns (M, rows, cols, vals) for
    elba_set_overlaps."""
    rng = np.random.default_rng(seed)
    g = tree_on_cycle(moves, wu.WeakGraph)[0] if kind == "tips" else nest(moves, wu.WeakGraph)[0]
    for _ in range(3):
        hub = g.new()[0]
        for n, score in STAR_ARMS:
            ids = g.chain(g.new(n))
            g.link(hub, ids[0], score)
    return g.overlaps(rng, perm=rng.permutation(g.n))


def per_round_nnz(restate, M, rows, cols, vals, mx, rounds):
    """[nnz(S) as round 0 finds it, as round 1 finds it, ..] of restate (tu.clip_tips or bu.pop_bubbles), up to the round that removes
    nothing or `rounds` rounds: one round at a time, each on what the one before left."""
    out = [len(rows)]
    for _ in range(rounds):
        rows, cols, vals, _, st = restate(M, rows, cols, vals, mx, 1)
        if st["reads_removed"] == 0:
            break
        out.append(len(rows))
    return out


def edges_crossed(nnz, tile):
    """The pairs of consecutive rounds between which the number of `tile`-sized tiles that hold entries of S falls."""
    tiles = [(n + tile - 1) // tile for n in nnz]
    return [(r, r + 1) for r in range(len(nnz) - 1) if tiles[r + 1] < tiles[r]]


def random_graph(seed, lo=2, hi=3001):
    """(M, rows, cols, vals, max, rounds): a graph of cu.random_string_graph as the CPU tests draw it, every third one small."""
    rng = np.random.default_rng(seed)
    M = int(rng.integers(lo, 120 if seed % 3 == 0 else hi))
    lens = rng.integers(20, 41, M)
    rows, cols, vals = cu.random_string_graph(rng, M, lens, n_paths=int(rng.integers(1, M // 3 + 2)), p_extra=float(rng.choice([0.05, 0.15, 0.4])))
    vals["suffix"] = rng.integers(5, 10, len(vals)); vals["suffixT"] = rng.integers(5, 10, len(vals))
    return M, rows, cols, vals, int(rng.choice(TIP_MAX)), int(rng.choice(ROUNDS))


def random_weak(seed, hi=3001):
    """((M, rows, cols, vals), S, q16): wu.random_S with p_one_image 0 (every third) or 0.08."""
    rng = np.random.default_rng(seed)
    M = int(rng.integers(2, 120 if seed % 3 == 1 else hi))
    (rows, cols, vals), _ = wu.random_S(rng, M, p_one_image=0.0 if seed % 3 == 0 else 0.08)
    vals["suffix"] = rng.integers(5, 10, len(vals)); vals["suffixT"] = rng.integers(5, 10, len(vals))
    return (M, rows, cols, vals), wu.S_of(rows, cols, vals), RATIOS_Q16[seed % len(RATIOS_Q16)]


TIP_SEEDS = tuple(range(100, 124))
BUBBLE_SEEDS = tuple(range(200, 224))
WEAK_SEEDS = tuple(range(300, 324))
SIMPLIFY_SEEDS = tuple(s for s in range(400, 413) if s != 411)        # (411 has nothing to remove: one pass)
SIMPLIFY_WEAK_SEEDS = tuple(range(500, 512))


def random_scored(seed, hi=1500):
    """random_graph with the scores of wu.random_S, for simplify with a ratio: (M, rows, cols, vals, max_tip, max_arm)."""
    M, rows, cols, vals, mx, _ = random_graph(seed, hi=hi)
    rng = np.random.default_rng(seed + 7)
    vals["score"] = rng.integers(-3, 12, len(vals))
    return M, rows, cols, vals, mx, int(rng.choice(TIP_MAX))
