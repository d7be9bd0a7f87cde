"""-m gpu: the routes through the CSR build of A (csrc/matrix.hip, finish_matrix_from_sorted_csc; its decisions: csrc/csr_plan.hpp), pinned.  Every case of
tests/csr_build_routes.py — sort keys from the k-mer stage's sort path and from its bucket kernels, hints and inline partners on and off, the pair sort,
the sort that leaves the rows to k_unpack_csr_words, dense matrices, positions beyond 16 bits, rebuilds from a consumed hand-off, device and host triples,
a shard's panel, degenerate shapes — must give the format counters, the sizes and the digests of A (both orientations) and of B recorded in
tests/golden/csr_build_routes.json."""
import json
import os

import pytest

import csr_build_routes as routes
import util

pytestmark = pytest.mark.gpu

with open(os.path.join(util.GOLDEN, "csr_build_routes.json")) as _f:
    GOLDEN = json.load(_f)

A_DIGESTS = ("a_colptr", "a_csc", "a_rowptr", "a_csr")


def test_the_fixture_holds_every_case_and_the_routes_the_cases_are_for():
    assert sorted(GOLDEN) == sorted(routes.ALL_CASES)
    g = GOLDEN
    # (a), (b): one-word sort, hints and inline partners — added late on the sort path, written by the bucket kernels (with gather slots) on the other
    for c in ("sort", "msd"):
        assert (g[c]["matrix_csr_words"], g[c]["matrix_hints"], g[c]["matrix_inline"], g[c]["matrix_suffix"]) == (1, 1, 1, 0)
    assert g["sort"]["slots_compact"] == 0 and g["msd"]["slots_compact"] == 1 and g["msd"]["gather_slots"] == 1
    # (c): hints without inline partners; neither
    for c in ("sort_no_inline", "msd_no_inline"):
        assert (g[c]["matrix_hints"], g[c]["matrix_inline"], g[c]["slots_compact"]) == (1, 0, 0)
    for c in ("sort_no_hints", "msd_no_hints"):
        assert (g[c]["matrix_hints"], g[c]["matrix_inline"]) == (0, 0)
    # (d): the pair sort on a matrix that is not dense
    for c in ("sort_csr_pairs", "msd_csr_pairs", "triples_sorted_csr_pairs"):
        assert (g[c]["matrix_csr_words"], g[c]["matrix_suffix"], g[c]["matrix_inline"]) == (0, 0, 0)
    # (e): the same matrix whichever kernel writes the rows
    assert g["sort_tune1"] == g["sort"]
    # every route over the k = 17 reads builds the same columns and the same B
    for c in ("msd", "sort_no_inline", "msd_no_inline", "sort_no_hints", "msd_no_hints", "sort_csr_pairs", "msd_csr_pairs", "triples_msd", "triples_host"):
        assert all(g[c][f] == g["sort"][f] for f in ("a_colptr", "a_csc", "a_rowptr", "b_nnz", "b_csr")), c
    # (f): dense, and kept off the dense path
    assert [g[c]["matrix_suffix"] for c in ("dense", "dense_msd", "dense_msd_pairs_late", "dense_no_suffix")] == [1, 1, 1, 0]
    assert all(g[c]["matrix_csr_words"] == 0 and g[c]["matrix_hints"] == 0 and g[c]["matrix_col_stride"] > 16 for c in ("dense", "dense_msd", "dense_msd_pairs_late"))
    assert all(g[c][f] == g["dense"][f] for c in ("dense_msd", "dense_msd_pairs_late") for f in A_DIGESTS + ("b_csr",))
    assert g["dense_no_suffix"]["b_csr"] == g["dense"]["b_csr"]
    # (g): positions beyond 16 bits
    assert (g["long_positions"]["matrix_pos16"], g["long_positions"]["matrix_inline"]) == (0, 0)
    # (h): a consumed hand-off rebuilds the same matrix (ids of row entries are slots only while the bucket kernels' gather slots stand)
    for c in routes.REBUILD_CASES:
        first, second, third = g[c]
        assert second == third and all(first[f] == second[f] for f in first if f != "slots_compact")
        assert all(second[f] == g["sort"][f] for f in A_DIGESTS + ("b_csr",))
    assert [r["slots_compact"] for r in g["rebuild_msd"]] == [1, 0, 0] and [r["slots_compact"] for r in g["rebuild_sort"]] == [0, 0, 0]
    # (i): device triples through the bucket kernels and through the sorts of the whole matrix (inline partners written by the build itself), host triples
    assert (g["triples_msd"]["triples_path"], g["triples_msd"]["matrix_inline"]) == (1, 1)
    assert (g["triples_sorted"]["triples_path"], g["triples_sorted"]["matrix_inline"], g["triples_sorted"]["matrix_csr_words"]) == (0, 1, 1)
    assert (g["triples_host"]["triples_path"], g["triples_host"]["matrix_inline"]) == (0, 1)
    # (j): a shard's panel: no inline partners unless asked for; dense with a row window
    assert (g["panel"]["matrix_inline"], g["panel_inline"]["matrix_inline"], g["panel_dense"]["matrix_suffix"]) == (0, 1, 1)
    assert "b_csr" in g["panel"] and "b_csr" not in g["panel_inline"]      # (a panel with inline partners is multiplied through the mirror exchange only)
    # (k)
    assert g["no_entries"]["nnz"] == 0 and g["no_entries"]["nrows"] > 0 and g["no_entries"]["ncols"] > 0 and g["one_row"]["nrows"] == 1 and g["one_column"]["ncols"] == 1


@pytest.mark.parametrize("name", routes.ALL_CASES)
def test_counters_sizes_and_digests_equal_the_recorded_ones(name):
    got = routes.run_case(name)
    print(name, got)
    assert got == GOLDEN[name]
