"""CPU: the layout-shaped overlap generator of tests/string_graph_util.py (reads placed on a genome, planted hubs) and what the scale
tests of tests/test_gpu_string_graph_scale.py rely on.  On small layout graphs the C oracle equals the literal Python restatement in
every field and count, which pins the generator's direction / suffix convention as one the reference's semiring accepts (most entries
ARE transitive there, unlike on graphs with independently drawn fields); the generator's degree report equals a brute-force count; and
the tie graph (suffixes from {0..4}) has the share of exact `suffix + fuzz == best walk` entries that the `>=` of the compare needs."""
import numpy as np
import pytest

import string_graph_util as sg
from oracle import pyoracle as po

TIE_SEED, TIE_M, TIE_COV = 1, 80, 6                       # the tie graph; tests/test_gpu_string_graph_scale.py runs the same one


def tie_graph(seed=TIE_SEED, M=TIE_M, cov=TIE_COV):
    rows, cols, vals = sg.layout_overlaps(np.random.default_rng(seed), M, cov)
    return rows, cols, sg.small_suffixes(np.random.default_rng(seed + 50), vals)


def _oracle_equals_restatement(M, rows, cols, vals, cutoff, fuzz):
    S, flags, st = po.string_graph(M, rows, cols, vals, cutoff=cutoff, fuzz=fuzz)
    want, wflags, wst = sg.python_string_graph(M, rows, cols, vals, cutoff, fuzz)
    assert list(flags) == list(wflags)
    assert [(int(r), int(c)) for r, c in zip(S["rows"], S["cols"])] == [(r, c) for r, c, _ in want]
    for a, (_, _, v) in enumerate(want):
        for f in po.OVERLAP_DTYPE.names:
            assert S["vals"][a][f] == v[f], (a, f)
    for key in ("bad_reads", "edges_passed", "contained_reads", "edges_kept", "nnzN", "marked", "removed", "nnz", "iterations", "products"):
        assert st[key] == wst[key], key
    return st


def _brute_degrees(M, rows, cols, vals, cutoff):
    deg = [0] * M; pas = [0] * M
    for r, c, v in zip(rows, cols, vals):
        deg[r] += 1; deg[c] += 1
        if v["passed"]:
            pas[r] += 1; pas[c] += 1
    bad = [(pas[v] + 1) / (deg[v] + 1.0) <= cutoff for v in range(M)]
    first = [(int(r), int(c), v) for r, c, v in zip(rows, cols, vals) if v["passed"] and not bad[r] and not bad[c]]
    cont = [False] * M
    for r, c, v in first:
        if v["containedQ"]:
            cont[r] = True
        if v["containedT"]:
            cont[c] = True
    kept = [0] * M
    for r, c, v in first:
        if not cont[r] and not cont[c]:
            kept[r] += 1; kept[c] += 1
    return kept, [int(b) | (int(c) << 1) for b, c in zip(bad, cont)]


@pytest.mark.parametrize("seed,hub", [(0, None), (1, None), (2, None), (3, None), (4, 30), (5, 12), (6, 47)])
def test_oracle_equals_the_restatement_on_layout_graphs(seed, hub):
    rng = np.random.default_rng(seed)
    M = int(rng.integers(40, 81))
    cutoff = (0.65, 0.5)[seed % 2]
    kw = dict(p_fail=0.1, p_nodir=0.05, p_contained=0.01 if seed % 3 else 0.0, cutoff=cutoff)
    if hub is None:
        rows, cols, vals = sg.layout_overlaps(rng, M, 6, **kw)
    else:
        rows, cols, vals = sg.layout_with_hub_degrees(seed, M, 6, ((hub, 30),), **kw)
        assert sg.kept_degrees(M, rows, cols, vals, cutoff)[0][hub] == 30
    assert (rows < cols).all() and (np.diff(rows * M + cols) > 0).all()          # upper-triangular, strictly ascending in (row, col)
    st = _oracle_equals_restatement(M, rows, cols, vals, cutoff, 1000)
    # a layout reduces towards a chain: most of what reaches the reduction is transitive
    assert st["marked"] > 0 and st["nnz"] < 0.75 * 2 * st["edges_kept"], st


@pytest.mark.parametrize("fuzz", [0, 1, 2])
def test_tie_graph_has_exact_ties_and_the_oracle_equals_the_restatement(fuzz):
    rows, cols, vals = tie_graph()
    ok = vals["passed"] != 0
    assert set(np.unique(vals["suffix"][ok])) <= set(range(5)) and set(np.unique(vals["suffixT"][ok])) <= set(range(5))
    st = _oracle_equals_restatement(TIE_M, rows, cols, vals, 0.65, fuzz)
    directed, marked, ties = sg.best_walks(TIE_M, rows, cols, vals, 0.65, fuzz)
    assert marked == st["marked"]                          # the counter below looks at the entries the reduction looks at
    assert ties >= 0.10 * directed, (ties, directed)       # `>` in place of `>=` would lose every one of these marks
    assert marked > ties                                   # and the strict side of the compare is there too


@pytest.mark.parametrize("seed", range(6))
def test_degree_report_equals_a_brute_force_count(seed):
    rng = np.random.default_rng(40 + seed)
    M = int(rng.integers(20, 120))
    cutoff = float(rng.choice([0.0, 0.5, 0.65, 0.8]))
    if seed % 2:
        rows, cols, vals = sg.layout_overlaps(rng, M, int(rng.integers(2, 9)), p_fail=0.25, p_nodir=0.05, p_contained=0.02, cutoff=cutoff)
    else:
        rows, cols, vals = sg.random_overlaps(rng, M, density=0.2, p_fail=0.3, p_contained=0.02)
    deg, flags = sg.kept_degrees(M, rows, cols, vals, cutoff)
    bdeg, bflags = _brute_degrees(M, rows, cols, vals, cutoff)
    assert list(deg) == bdeg and list(flags) == bflags
    _, oflags, ost = po.string_graph(M, rows, cols, vals, cutoff=cutoff)
    assert list(oflags) == bflags and ost["edges_kept"] * 2 == sum(bdeg)


def test_hubs_get_the_asked_degree_and_leave_the_rest_alone():
    M, hubs = 3000, ((5, 257), (1500, 300), (2990, 40))
    base = sg.layout_overlaps(np.random.default_rng(9), M, 8)
    rows, cols, vals = sg.layout_with_hub_degrees(9, M, 8, hubs)
    d0, f0 = sg.kept_degrees(M, *base)
    d1, f1 = sg.kept_degrees(M, rows, cols, vals)
    assert [int(d1[h]) for h, _ in hubs] == [d for _, d in hubs]
    assert (f0 == f1).all() and not f1[[h for h, _ in hubs]].any()
    grown = np.flatnonzero(d1 != d0)                        # the hubs and their new partners, one edge each (hubs are no partners)
    assert set(h for h, _ in hubs) <= set(grown) and (d1[grown] >= d0[grown]).all()
    assert len(rows) - len(base[0]) == sum(d - int(d0[h]) for h, d in hubs)
    _, oflags, ost = po.string_graph(M, rows, cols, vals)
    assert (oflags == f1).all() and 2 * ost["edges_kept"] == d1.sum()
    with pytest.raises(ValueError):                         # a read the prunes remove cannot be a hub
        sg.layout_overlaps(np.random.default_rng(9), M, 8, hubs=((int(np.flatnonzero(f0)[0]), 10),))


def test_relabelled_graph_reduces_to_the_relabelled_result():
    """Overlap::Transpose where the new ids change a pair's order: the oracle's S of the relabelled graph is its S mapped."""
    M = 70
    rows, cols, vals = sg.layout_with_hub_degrees(11, M, 6, ((20, 35),), p_nodir=0.05)
    perm = np.random.default_rng(12).permutation(M)
    prow, pcol, pval = sg.relabel(perm, rows, cols, vals)
    assert (prow < pcol).all() and (np.diff(prow * M + pcol) > 0).all() and (prow != rows).any()
    S, flags, st = po.string_graph(M, rows, cols, vals)
    P, pflags, pst = po.string_graph(M, prow, pcol, pval)
    sg.assert_mapped(perm, S, flags, st, P, pflags, pst)
    _oracle_equals_restatement(M, prow, pcol, pval, 0.65, 1000)
