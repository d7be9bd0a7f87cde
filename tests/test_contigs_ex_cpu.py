"""The restatement of contig generation with circular and single-read contigs (contig_ex_util.py) against two things that do not depend
on it: contig_util.generate_contigs where no extension is asked for, and the genomes themselves where circles are laid out read by read.
No GPU: the device tests (test_gpu_contigs_ex.py) hold contig.hip against this restatement."""
import numpy as np
import pytest

import contig_ex_util as cx
import contig_util as cu


@pytest.mark.parametrize("seed", range(10))
def test_restatement_without_flags_is_the_reference_walk(seed):
    rng = np.random.default_rng(4100 + seed)
    M = int(rng.integers(30, 400))
    seqs = cu.random_reads(rng, M, 1 if seed % 2 else 20, 120)
    lens = [len(s) for s in seqs]
    keys, ovs = _keys_vals(cu.random_string_graph(rng, M, lens, p_extra=float(rng.choice([0.0, 0.05, 0.3]))))
    rows, cols, vals = cu.symmetric(dict(zip(keys, ovs)))
    want = cu.generate_contigs(M, rows, cols, vals, seqs)
    contigs, chains, kinds, read_contig, stats = cx.generate_contigs_ex(M, rows, cols, vals, seqs, 0)
    assert (contigs, chains, read_contig, stats) == want
    assert kinds == [cx.PATH] * len(contigs) and stats["contigs"] > 0


def _keys_vals(upper):
    rows, cols, vals = upper
    return [(int(r), int(c)) for r, c in zip(rows, cols)], list(vals)


def _run(seqs, edges, flags, read_flags=None):
    rows, cols, vals = cu.symmetric(edges)
    return cx.generate_contigs_ex(len(seqs), rows, cols, vals, seqs, flags, read_flags)


def test_forward_step_encoding():
    """The property the layout's edges are derived from: forward reads, Q left of T -> direction 1, directionT 2, suffixT the difference
    of the starts, suffix that of the ends."""
    rng = np.random.default_rng(1)
    g = cx.random_genome(rng, 400)
    for _ in range(20):
        seqs, edges = cx.layout_reads(rng, g, 6, True, np.arange(6))
        for (i, j), o in edges.items():
            si, sj = seqs[i], seqs[j]
            if si in g + g and sj in g + g and j == i + 1:                  # both forward, i left of j
                assert (int(o["direction"]), int(o["directionT"])) == (1, 2)
                ov = len(si) - int(o["suffixT"])                            # i's tail is j's head
                assert ov > 0 and si[int(o["suffixT"]):] == sj[:ov]
                assert int(o["suffix"]) == len(sj) - ov


@pytest.mark.parametrize("n", [4, 5, 50])
@pytest.mark.parametrize("seed", range(3))
def test_a_circle_comes_back_as_a_rotation_of_its_genome(n, seed):
    rng = np.random.default_rng(100 * n + seed)
    seqs, edges, info = cx.genome_graph(rng, [(int(rng.integers(2000, 5001)), n, True)])
    g = info[0][0]
    contigs, chains, kinds, read_contig, st = _run(seqs, edges, cx.CIRCULAR)
    assert kinds == [cx.CIRCLE] and st["cycles"] == 1 and st["contig_reads"] == n
    assert len(contigs[0]) == len(g) and cx.is_rotation(contigs[0], g)
    s = chains[0][0][0]
    assert s == 0 and chains[0][1][0] == min(a + b - s for a, b in edges if s in (a, b))      # from the smallest read towards its smaller neighbour
    assert sorted(r for r, _, _ in chains[0]) == list(range(n)) and read_contig == [0] * n
    assert _run(seqs, edges, 0)[0] == [] and _run(seqs, edges, cx.SINGLETONS)[0] == []        # reads of a cycle are never singletons


@pytest.mark.parametrize("seed", range(4))
def test_two_circles_and_a_linear_genome_in_one_graph(seed):
    rng = np.random.default_rng(900 + seed)
    parts = [(int(rng.integers(2000, 5001)), int(rng.integers(4, 30)), True), (int(rng.integers(2000, 5001)), int(rng.integers(4, 30)), True),
             (int(rng.integers(2000, 5001)), int(rng.integers(2, 30)), False)]
    seqs, edges, info = cx.genome_graph(rng, parts)
    contigs, chains, kinds, read_contig, st = _run(seqs, edges, cx.CIRCULAR | cx.SINGLETONS)
    assert len(contigs) == 3 and st["cycles"] == 2 and sorted(kinds) == [cx.PATH, cx.CIRCLE, cx.CIRCLE]
    for g, ids, circ in info:
        k = read_contig[ids[0]]
        assert all(read_contig[v] == k for v in ids) and kinds[k] == (cx.CIRCLE if circ else cx.PATH)
        assert cx.is_rotation(contigs[k], g) if circ else contigs[k] in (g, cu.revcomp(g))
    starts = [ch[0][0] for ch in chains]
    assert starts == sorted(starts)
    assert _run(seqs, edges, 0)[0] == [contigs[kinds.index(cx.PATH)]]                      # without flags: the path alone


def test_order_kinds_and_flagged_reads_under_both_flags():
    rng = np.random.default_rng(77)
    M = 300
    seqs = cu.random_reads(rng, M, 1, 80)
    seqs[5] = ""; seqs[17] = ""                                          # empty reads are skipped
    lens = [len(s) for s in seqs]
    keys, vals = _keys_vals(cu.random_string_graph(rng, M, lens, n_paths=60, p_extra=0.2))
    edges = dict(zip(keys, vals))
    deg = np.zeros(M, dtype=int)
    for i, j in keys:
        deg[i] += 1; deg[j] += 1
    kept = np.zeros(M, dtype=int)                                        # neighbours that are no branches
    for i, j in keys:
        kept[i] += deg[j] <= 2; kept[j] += deg[i] <= 2
    read_flags = np.zeros(M, dtype=np.uint8)
    lonely = [v for v in range(M) if deg[v] > 2 or kept[v] == 0]         # branches, and reads with no kept neighbour
    assert len(lonely) > 12
    read_flags[lonely[::3]] = 1; read_flags[lonely[1::3]] = 2            # bad, contained
    contigs, chains, kinds, read_contig, st = _run(seqs, edges, cx.CIRCULAR | cx.SINGLETONS, read_flags)
    assert {cx.PATH, cx.CIRCLE, cx.SINGLE} == set(kinds)
    starts = [ch[0][0] for ch in chains]
    assert starts == sorted(starts) and len(set(starts)) == len(starts)
    for ch, k in zip(chains, kinds):
        reads = [r for r, _, _ in ch]
        if k == cx.PATH:
            assert ch[0][0] < ch[-1][0] and len(ch) >= 2
        elif k == cx.CIRCLE:
            assert ch[0][0] == min(reads) and len(ch) >= 4 and ch[1][0] < ch[-1][0]
        else:
            v = ch[0][0]
            assert ch == [(v, len(seqs[v]), 0)] and read_flags[v] == 0 and len(seqs[v]) > 0 and (deg[v] > 2 or kept[v] == 0)
    single = {ch[0][0] for ch, k in zip(chains, kinds) if k == cx.SINGLE}
    assert single == {v for v in range(M) if read_contig[v] >= 0 and kinds[read_contig[v]] == cx.SINGLE}
    assert not single & set(np.nonzero(read_flags)[0].tolist()) and 5 not in single and 17 not in single
    assert single == {v for v in lonely if read_flags[v] == 0 and seqs[v]}
    # every read is in at most one contig, and each flag adds its own kind to the default's contigs without touching them
    base = _run(seqs, edges, 0, read_flags)
    assert [c for c, k in zip(contigs, kinds) if k == cx.PATH] == base[0]
    assert st["contig_reads"] == sum(1 for v in read_contig if v >= 0)
    assert st["cycles"] == base[4]["cycles"] == kinds.count(cx.CIRCLE) and st["components"] == base[4]["components"]
    assert st["used_components"] == base[4]["used_components"] and st["branches"] == base[4]["branches"]


def test_a_bad_closing_prefix_names_the_last_read_and_the_start():
    rng = np.random.default_rng(5)
    seqs, edges, info = cx.genome_graph(rng, [(2000, 7, True)])
    rows, cols, vals = cu.symmetric(edges)
    _, chains, _, _, _ = cx.generate_contigs_ex(7, rows, cols, vals, seqs, cx.CIRCULAR)
    last, s = chains[0][-1][0], chains[0][0][0]
    field = "suffixT" if last < s else "suffix"                          # the closing step last -> s, whichever triangle stores it
    edges[(min(last, s), max(last, s))][field] = len(seqs[last]) + 1
    rows, cols, vals = cu.symmetric(edges)
    with pytest.raises(cu.BadPrefix) as x:
        cx.generate_contigs_ex(7, rows, cols, vals, seqs, cx.CIRCULAR)
    assert x.value.pair == (last, s)
    assert cx.generate_contigs_ex(7, rows, cols, vals, seqs, cx.SINGLETONS)[0] == []   # not walked, not checked
