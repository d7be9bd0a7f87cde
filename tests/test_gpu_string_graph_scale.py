"""-m gpu: elba_transitive_reduction where tests/test_gpu_string_graph.py does not reach, on layout-shaped graphs (tests/string_graph_util.py:
reads on a genome, a band of triangles per read reduced to a chain, planted hubs), bit-exact against the CPU oracle as there.

k_tr_mark runs min(M, 32 x CUs) workgroups, each walking rows i = blockIdx.x, += gridDim.x, and stages a row of at most 2048 entries in
LDS 256 entries per step.  Here: more rows than four grids (the row loop, its barrier, LDS staged over the previous row's), hubs of
257 / 512 / 2047 / 2048 / 2049 / 5000 entries on rows one workgroup meets in turn (every staging stride count, the cap from both sides,
staged after unstaged and back), sort keys of 32, 34 and 42 bits, exact ties of the compare, suffixes near 5 * 10^8, one context over
graphs of changing size, and relabelled reads.  Every condition that makes a case what it claims to be (M against the CU count, the
hubs' degrees, the tie share, the overflow bound, edges at both end ids) is asserted from the input and the oracle's output, never
from the GPU's."""
import functools

import numpy as np
import pytest
import torch

import elba_amd
import string_graph_util as sg
from oracle import pyoracle as po
from test_string_graph_layout_cpu import TIE_M, tie_graph

pytestmark = pytest.mark.gpu

CUTOFF, FUZZ = 0.65, 1000
HUB_M = 40000


def _grid():
    return 32 * torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=None)
def _layout(seed, M, cov=8, suffix_scale=1):
    return (M,) + sg.layout_overlaps(np.random.default_rng(seed), M, cov, suffix_scale=suffix_scale)


@functools.lru_cache(maxsize=None)
def _hub_plan(grid):
    """Hub reads and degrees: two residues modulo the grid, so that one workgroup takes an unstaged row (5000), a staged one (2048) and
    an unstaged one (2049) in turn, and another a staged row (2047), an unstaged (2600), and staged rows of two strides (257, 512).
    The ids are the first at or after 100 / 3000 whose reads the prunes keep in the graph without hubs (the generator asks for that)."""
    M = HUB_M
    assert M >= 4 * grid
    deg, flags = sg.kept_degrees(M, *sg.layout_overlaps(np.random.default_rng(3), M, 8), CUTOFF)
    free = (flags == 0) & (deg > 0)
    plan = []
    for first, degrees in ((100, (5000, 2048, 2049)), (3000, (2047, 2600, 257, 512))):
        b = next(b for b in range(first, grid) if all(free[b + t * grid] for t in range(len(degrees))))
        plan += [(b + t * grid, d) for t, d in enumerate(degrees)]
    return tuple(plan)


@functools.lru_cache(maxsize=None)
def _hub_graph(grid):
    return (HUB_M,) + sg.layout_with_hub_degrees(3, HUB_M, 8, _hub_plan(grid), cutoff=CUTOFF)


@functools.lru_cache(maxsize=None)
def _oracle(key, cutoff=CUTOFF, fuzz=FUZZ):
    """po.string_graph of a cached graph (key = the cached builder and its arguments): run once however many tests use the graph."""
    M, rows, cols, vals = key[0](*key[1:])
    return po.string_graph(M, rows, cols, vals, cutoff=cutoff, fuzz=fuzz)


def _run(e, key, cutoff=CUTOFF, fuzz=FUZZ):
    M, rows, cols, vals = key[0](*key[1:])
    e.set_overlaps(M, rows, cols, vals)
    return sg.assert_same_as_oracle(e, M, rows, cols, vals, cutoff, fuzz, want=_oracle(key, cutoff, fuzz))


def _check(M, rows, cols, vals, cutoff=CUTOFF, fuzz=FUZZ):
    e = elba_amd.Engine(17, 2, 8)
    e.set_overlaps(M, rows, cols, vals)
    want = po.string_graph(M, rows, cols, vals, cutoff=cutoff, fuzz=fuzz)
    sg.assert_same_as_oracle(e, M, rows, cols, vals, cutoff, fuzz, want=want)
    e.close()
    return want


def _removed_at(read, M, rows, cols, vals, S, cutoff=CUTOFF):
    """The entries (read, x) the oracle removed as transitive: those that reach the reduction with a direction, less those left in S."""
    keep, _ = sg.kept_edges(M, rows, cols, vals, cutoff)
    directed = int((keep & (rows == read) & (vals["direction"] != -1)).sum() + (keep & (cols == read) & (vals["directionT"] != -1)).sum())
    return directed - int((S["rows"] == read).sum())


@pytest.mark.parametrize("seed,M", [(1, 40000), (2, 300000)])
def test_every_workgroup_takes_several_rows(seed, M):
    assert M >= 4 * _grid()
    key = (_layout, seed, M)
    _, rows, cols, vals = _layout(seed, M)
    deg, _ = sg.kept_degrees(M, rows, cols, vals, CUTOFF)
    assert (deg >= 2).sum() >= M // 2                       # rows that are searched, not skipped
    e = elba_amd.Engine(17, 2, 8)
    _run(e, key)
    e.close()
    st = _oracle(key)[2]
    assert st["marked"] > 0 and st["nnz"] < st["edges_kept"]         # a band reduced towards a chain


def test_staging_strides_and_the_lds_cap_on_rows_of_one_workgroup():
    grid = _grid()
    plan = _hub_plan(grid)
    M, rows, cols, vals = _hub_graph(grid)
    deg, flags = sg.kept_degrees(M, rows, cols, vals, CUTOFF)
    assert sorted(int(deg[h]) for h, _ in plan) == [257, 512, 2047, 2048, 2049, 2600, 5000]
    assert [int(deg[h]) for h, _ in plan] == [d for _, d in plan]
    ids = [h for h, _ in plan]
    assert len(set(h % grid for h in ids[:3])) == 1 and len(set(h % grid for h in ids[3:])) == 1          # met by one workgroup each
    assert [d > 2048 for _, d in plan] == [True, False, True, False, True, False, False]                     # unstaged / staged in turn
    assert min(ids) < grid < max(ids) < M
    e = elba_amd.Engine(17, 2, 8)
    _run(e, (_hub_graph, grid))
    e.close()
    S, oflags, _ = _oracle((_hub_graph, grid))
    for h in ids:
        assert oflags[h] == 0 and flags[h] == 0
        assert _removed_at(h, M, rows, cols, vals, S) > 0, h


@pytest.mark.parametrize("seed,M,cov,bits", [(4, 65535, 8, 32), (4, 65536, 8, 34), (5, (1 << 20) + 1, 4, 42)])
def test_sort_key_width(seed, M, cov, bits):
    mb = 1
    while (1 << mb) < M + 1:
        mb += 1
    assert 2 * mb == bits
    _, rows, cols, vals = _layout(seed, M, cov)
    deg, _ = sg.kept_degrees(M, rows, cols, vals, CUTOFF)
    assert deg[0] > 0 and deg[M - 1] > 0                    # the smallest and the largest id are in keys that the sort orders
    S, _, st = _check(M, rows, cols, vals)
    assert st["marked"] > 0 and (S["rows"] == M - 1).any() and (S["rows"] == 0).any()


@pytest.mark.parametrize("fuzz", [0, 1, 2])
def test_exact_ties_are_marked(fuzz):
    rows, cols, vals = tie_graph()
    directed, marked, ties = sg.best_walks(TIE_M, rows, cols, vals, CUTOFF, fuzz)
    assert ties >= 0.10 * directed and marked > ties
    _, _, st = _check(TIE_M, rows, cols, vals, fuzz=fuzz)
    assert st["marked"] == marked


def test_exact_ties_beyond_the_grid():
    M = 40000
    assert M >= 4 * _grid()
    rows, cols, vals = tie_graph(seed=1, M=M, cov=4)
    directed, marked, ties = sg.best_walks(M, rows, cols, vals, CUTOFF, 1)
    assert ties >= 0.10 * directed and marked > ties
    _, _, st = _check(M, rows, cols, vals, fuzz=1)
    assert st["marked"] == marked


def test_large_suffixes_stay_within_int32():
    M, fuzz = 40000, 1000
    _, rows, cols, vals = _layout(6, M, 8, 50000)
    top = int(max(np.abs(vals["suffix"].astype(np.int64)).max(), np.abs(vals["suffixT"].astype(np.int64)).max()))
    assert 4 * 10**8 <= top and 2 * top + fuzz < 2**31     # about 5e8, and no sum of two plus fuzz overflows on either side
    assert (vals["suffix"] < 0).any() and (vals["suffixT"] < 0).any()
    _, _, st = _check(M, rows, cols, vals, fuzz=fuzz)
    directed = st["removed"] + st["nnz"]
    assert 0.2 * directed < st["marked"] < 0.9 * directed   # jitter x scale is far above fuzz: the compare decides both ways


def test_one_context_over_graphs_of_changing_size():
    """reserve, the memsets sized by the current n and M, and marks / selections left beyond the new size by a larger graph."""
    grid = _grid()
    e = elba_amd.Engine(17, 2, 8)
    big = _run(e, (_layout, 2, 300000))
    small = _run(e, (_layout, 7, 50, 6))
    assert big["marked"] > small["marked"] > 0
    z = np.zeros(0, dtype=po.OVERLAP_DTYPE)
    e.set_overlaps(7, [], [], z)
    sg.assert_same_as_oracle(e, 7, np.zeros(0, np.int64), np.zeros(0, np.int64), z, CUTOFF, FUZZ)
    _run(e, (_hub_graph, grid))
    M, rows, cols, vals = _layout(7, 50, 6)                # the small graph on reads 1000 .. 1049 of a larger set
    e.set_overlaps(M + 2000, rows + 1000, cols + 1000, vals)
    st = e.transitive_reduction(CUTOFF, FUZZ)
    g = e.export_string_graph()
    S, flags, ost = _oracle((_layout, 7, 50, 6))
    for key in sg.COUNTS:
        assert st[key] == ost[key], key
    assert (g["rows"] == S["rows"] + 1000).all() and (g["cols"] == S["cols"] + 1000).all()
    for f in po.OVERLAP_DTYPE.names:
        if f != "pad":
            assert (g["vals"][f] == S["vals"][f]).all(), f
    got = e.export_read_flags(M + 2000)
    assert (got[1000:1050] == flags).all() and not got[:1000].any() and not got[1050:].any()
    _run(e, (_layout, 1, 40000))
    e.close()


def test_relabelled_reads_give_the_relabelled_graph():
    """Hubs and bands at arbitrary rows, pairs stored as their Overlap::Transpose where the new ids change their order."""
    M = 40000
    hubs = ((777, 300), (20111, 2100))
    rows, cols, vals = sg.layout_with_hub_degrees(8, M, 8, hubs, cutoff=CUTOFF)
    perm = np.random.default_rng(13).permutation(M)
    prow, pcol, pval = sg.relabel(perm, rows, cols, vals)
    deg, _ = sg.kept_degrees(M, prow, pcol, pval, CUTOFF)
    assert [int(deg[perm[h]]) for h, _ in hubs] == [d for _, d in hubs]
    S, flags, st = _check(M, rows, cols, vals)
    P, pflags, pst = _check(M, prow, pcol, pval)
    sg.assert_mapped(perm, S, flags, st, P, pflags, pst)
