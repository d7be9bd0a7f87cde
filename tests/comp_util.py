"""Connected components (elba_graph_components / elba_partition_components, include/elba_amd.h) restated on the CPU, numpy only: the
rule twice (a literal union-find; a vectorised min-label form with pointer jumping that also reports its rounds), the per-component
tables and stats, the greedy partition as the reference's statements have it (src/ContigGeneration.cpp:126, :184-197) with the two
tie rules of the header, builders of the shapes the GPU tests load, and the hand cases with their claims.

An edge list here is two int64 arrays (u, v) of read ids, one entry per undirected edge, in any orientation and order."""
import numpy as np

TABLES = ("first_read", "reads", "bases", "edges", "branches", "ends")


# ---- the edges of the two graphs ---------------------------------------------------------------------------------------------------
def edges_of_string_graph(g):
    """The undirected edges of an exported S: every pair of reads with an entry, once.  S holds both triangles, but the reduction can keep
    one image of a pair only (it drops an image without a direction alone), so the pairs are taken from both."""
    rows, cols = np.asarray(g["rows"], dtype=np.int64), np.asarray(g["cols"], dtype=np.int64)
    off = rows != cols
    lo, hi = np.minimum(rows, cols)[off], np.maximum(rows, cols)[off]
    if len(lo) == 0:
        return hi, lo
    span = int(hi.max()) + 1
    key = np.unique(hi * span + lo)
    return key // span, key % span


def edges_of_overlaps(rows, cols, vals):
    """The undirected edges of an edge list: the pairs with passed != 0, nothing else."""
    ok = np.asarray(vals["passed"]) != 0
    return np.asarray(rows, dtype=np.int64)[ok], np.asarray(cols, dtype=np.int64)[ok]


# ---- the rule, twice -----------------------------------------------------------------------------------------------------------------
def union_find(M, u, v):
    """label[x] = the smallest read of x's component, by a literal union-find (link the larger root under the smaller, path halving)."""
    parent = list(range(int(M)))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in zip(np.asarray(u).tolist(), np.asarray(v).tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(x) for x in range(int(M))], dtype=np.int64)


def min_label(M, u, v):
    """The same labels by whole-array steps: every edge offers the smaller of its ends' labels to the larger label (which is a root: the
    labels are flat when a hooking step starts), then label = label[label] until flat; repeated until a hooking step changes nothing.
    Returns (labels, rounds): rounds counts every hooking step and every jumping step — the passes a device form of this shape makes."""
    u, v = np.asarray(u, dtype=np.int64), np.asarray(v, dtype=np.int64)
    f = np.arange(int(M), dtype=np.int64)
    rounds = 0
    while True:
        rounds += 1
        fu, fv = f[u], f[v]
        g = f.copy()
        np.minimum.at(g, np.maximum(fu, fv), np.minimum(fu, fv))
        while True:
            rounds += 1
            g2 = g[g]
            if (g2 == g).all():
                break
            g = g2
        if (g == f).all():
            return f, rounds
        f = g


def tables(M, u, v, labels=None, lens=None, base=0):
    """What elba_graph_components returns for the graph: comp_of_read and the six arrays per component, numbered by ascending smallest read."""
    M = int(M)
    u, v = np.asarray(u, dtype=np.int64), np.asarray(v, dtype=np.int64)
    labels = union_find(M, u, v) if labels is None else np.asarray(labels, dtype=np.int64)
    roots = np.flatnonzero(labels == np.arange(M))
    rank = np.full(M, -1, dtype=np.int64)
    rank[roots] = np.arange(len(roots))
    comp = rank[labels]
    n = len(roots)
    deg = np.bincount(u, minlength=M) + np.bincount(v, minlength=M)
    out = dict(comp_of_read=comp.astype(np.int32), first_read=roots + int(base), reads=np.bincount(comp, minlength=n).astype(np.int64))
    out["bases"] = np.zeros(n, dtype=np.int64) if lens is None else _sum_by(comp, np.asarray(lens, dtype=np.int64), n)
    out["edges"] = np.bincount(comp[u], minlength=n).astype(np.int64) if len(u) else np.zeros(n, dtype=np.int64)
    out["branches"] = _sum_by(comp, (deg > 2).astype(np.int64), n)
    out["ends"] = _sum_by(comp, (deg == 1).astype(np.int64), n)
    return out


def _sum_by(comp, w, n):
    s = np.zeros(n, dtype=np.int64)
    np.add.at(s, comp, w)          # (exact 64-bit sums: bincount's weights are doubles)
    return s


def stats(t):
    reads = t["reads"]
    best = int(np.argmax(reads)) if len(reads) else -1          # (argmax: the first of the largest)
    return dict(nreads=int(reads.sum()), edges=int(t["edges"].sum()), components=len(reads), used_components=int((reads >= 2).sum()),
                isolated=int((reads == 1).sum()), largest_reads=int(reads[best]) if best >= 0 else 0, largest_bases=int(t["bases"][best]) if best >= 0 else 0)


def shape(reads, branches, ends):
    if reads == 1:
        return "lone"
    if branches == 0 and ends == 2:
        return "path"
    if branches == 0 and ends == 0 and reads >= 3:
        return "ring"
    return "other"


def same_tables(got, want):
    """None, or the name of the first array that differs."""
    for k in ("comp_of_read",) + TABLES:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        if a.shape != b.shape or not (a.astype(np.int64) == b.astype(np.int64)).all():
            return k
    return None


# ---- the partition ---------------------------------------------------------------------------------------------------------------------
def partition(reads, weight, nparts, min_reads=2):
    """The reference's loop, statement by statement: the (component, weight) tuples of the components with at least min_reads reads,
    sorted by weight descending (ties: the smaller component first), each added to the part std::min_element finds (the first of the
    smallest sums).  Returns (part_of_comp, part_weight)."""
    result = [(c, int(weight[c])) for c in range(len(reads)) if int(reads[c]) >= min_reads]
    result.sort(key=lambda t: (-t[1], t[0]))
    sums = [0] * int(nparts)
    part_of_comp = np.full(len(reads), -1, dtype=np.int32)
    for c, w in result:
        where = sums.index(min(sums))
        sums[where] += w
        part_of_comp[c] = where
    return part_of_comp, np.array(sums, dtype=np.int64)


def partition_of_reads(t, nparts, weight="reads", min_reads=2):
    """(part_of_read, part_weight) for the tables of a graph."""
    poc, pw = partition(t["reads"], t[weight], nparts, min_reads)
    return poc[t["comp_of_read"]] if len(t["comp_of_read"]) else np.zeros(0, np.int32), pw


# ---- shapes ----------------------------------------------------------------------------------------------------------------------------
NUMBERINGS = ("ascending", "descending", "random", "alternating")


def numbering(M, kind, rng=None):
    """ids[p] = the read at position p: 0, 1, 2 ... | M-1, M-2 ... | a permutation | 0, M-1, 1, M-2 ... (low and high ids alternate)."""
    p = np.arange(int(M), dtype=np.int64)
    if kind == "ascending":
        return p
    if kind == "descending":
        return M - 1 - p
    if kind == "random":
        return (rng or np.random.default_rng(0)).permutation(int(M)).astype(np.int64)
    if kind == "alternating":
        return np.where(p % 2 == 0, p // 2, M - 1 - p // 2)
    raise ValueError(kind)


def path(M, kind="ascending", rng=None):
    ids = numbering(M, kind, rng)
    return int(M), ids[:-1], ids[1:]


def ring(M, kind="ascending", rng=None):
    ids = numbering(M, kind, rng)
    return int(M), ids, np.roll(ids, -1)


def star(leaves, hub_first=True):
    """leaves + 1 reads: the hub is read 0, or read M - 1."""
    M = int(leaves) + 1
    leaf = np.arange(1, M, dtype=np.int64) if hub_first else np.arange(0, M - 1, dtype=np.int64)
    return M, np.full(leaves, 0 if hub_first else M - 1, dtype=np.int64), leaf


def binary_tree(depth, kind="ascending", rng=None):
    """2^(depth + 1) - 1 reads; position p hangs under position (p - 1) // 2."""
    M = (1 << (depth + 1)) - 1
    ids = numbering(M, kind, rng)
    p = np.arange(1, M, dtype=np.int64)
    return M, ids[p], ids[(p - 1) // 2]


def caterpillar(spine, kind="alternating", rng=None):
    """A path of `spine` reads, every one with a leg of one read: positions 0 .. spine-1 are the spine, spine + p is the leg of p."""
    M = 2 * int(spine)
    ids = numbering(M, kind, rng)
    p = np.arange(spine, dtype=np.int64)
    return M, np.concatenate([ids[p[:-1]], ids[p]]), np.concatenate([ids[p[1:]], ids[p + spine]])


def isolated_pairs(npairs):
    """3 * npairs reads: the pair (3k, 3k + 2) with the lone read 3k + 1 between its ends."""
    k = np.arange(int(npairs), dtype=np.int64)
    return 3 * int(npairs), 3 * k, 3 * k + 2


def two_giants(n):
    """2n reads: a path over 0 .. n-2 and read 2n-2, a path over n-1 .. 2n-3 and read 2n-1, and the edge (2n-2, 2n-1) that joins them —
    the last of the list in (row, col) order, and the last entry with row > column of an S in (col, row) order."""
    a = np.concatenate([np.arange(0, n - 1), [2 * n - 2]]).astype(np.int64)
    b = np.concatenate([np.arange(n - 1, 2 * n - 2), [2 * n - 1]]).astype(np.int64)
    u = np.concatenate([a[:-1], b[:-1], [2 * n - 2]])
    v = np.concatenate([a[1:], b[1:], [2 * n - 1]])
    return 2 * int(n), u, v


def random_graph(rng, M, nedges):
    """nedges distinct random pairs over M reads (around M / 2 edges the giant component appears)."""
    if M < 2 or nedges <= 0:
        return int(M), np.zeros(0, np.int64), np.zeros(0, np.int64)
    a, b = rng.integers(0, M, size=2 * nedges), rng.integers(0, M, size=2 * nedges)
    keep = a != b
    key = np.unique(np.minimum(a, b)[keep] * M + np.maximum(a, b)[keep])
    key = rng.permutation(key)[:nedges]
    return int(M), key // M, key % M


def sorted_pairs(u, v):
    """(rows, cols) with rows < cols, strictly ascending in (row, col): what elba_set_overlaps takes."""
    u, v = np.asarray(u, dtype=np.int64), np.asarray(v, dtype=np.int64)
    r, c = np.minimum(u, v), np.maximum(u, v)
    assert (r < c).all()
    order = np.lexsort((c, r))
    r, c = r[order], c[order]
    assert len(r) < 2 or ((r[1:] > r[:-1]) | ((r[1:] == r[:-1]) & (c[1:] > c[:-1]))).all(), "a pair twice"
    return r, c


def overlap_records(rng, n, dtype, passed=None):
    """n records for elba_set_overlaps whose pairs the reduction keeps at cutoff 0 and fuzz 0 whatever the graph: all four directions,
    suffix and suffixT in [5, 9] (a two-edge walk is at least 10).  passed: 0 / 1 per record (default all 1)."""
    vals = np.zeros(int(n), dtype=dtype)
    vals["passed"] = 1 if passed is None else passed
    vals["direction"] = rng.integers(0, 4, n); vals["directionT"] = rng.integers(0, 4, n)
    vals["suffix"] = rng.integers(5, 10, n); vals["suffixT"] = rng.integers(5, 10, n)
    return vals


# ---- hand cases ------------------------------------------------------------------------------------------------------------------------
def _case(M, pairs, comp, edges, branches, ends, shapes):
    return dict(M=M, pairs=pairs, comp=comp, edges=edges, branches=branches, ends=ends, shapes=shapes)


def hand_cases():
    """name -> M, pairs and what the rule says of them: the component of every read, and per component its edges, branches, ends and shape."""
    L, P, R, O = "lone", "path", "ring", "other"
    return {
        "no_edge": _case(3, [], [0, 1, 2], [0, 0, 0], [0, 0, 0], [0, 0, 0], [L, L, L]),
        "one_read": _case(1, [], [0], [0], [0], [0], [L]),
        "one_edge": _case(2, [(0, 1)], [0, 0], [1], [0], [2], [P]),
        "one_edge_behind_lone_reads": _case(5, [(3, 4)], [0, 1, 2, 3, 3], [0, 0, 0, 1], [0, 0, 0, 0], [0, 0, 0, 2], [L, L, L, P]),
        "path3_ascending": _case(3, [(0, 1), (1, 2)], [0, 0, 0], [2], [0], [2], [P]),
        "path3_smallest_in_the_middle": _case(3, [(1, 0), (0, 2)], [0, 0, 0], [2], [0], [2], [P]),
        "path3_largest_in_the_middle": _case(3, [(0, 2), (2, 1)], [0, 0, 0], [2], [0], [2], [P]),
        "triangle": _case(3, [(0, 1), (1, 2), (0, 2)], [0, 0, 0], [3], [0], [0], [R]),
        "ring4": _case(4, [(0, 1), (1, 2), (2, 3), (0, 3)], [0, 0, 0, 0], [4], [0], [0], [R]),
        "ring5_shuffled": _case(5, [(0, 3), (3, 1), (1, 4), (4, 2), (2, 0)], [0, 0, 0, 0, 0], [5], [0], [0], [R]),
        "star_hub_first": _case(4, [(0, 1), (0, 2), (0, 3)], [0, 0, 0, 0], [3], [1], [3], [O]),
        "star_hub_last": _case(4, [(3, 0), (3, 1), (3, 2)], [0, 0, 0, 0], [3], [1], [3], [O]),
        "two_pairs": _case(4, [(0, 1), (2, 3)], [0, 0, 1, 1], [1, 1], [0, 0], [2, 2], [P, P]),
        "two_pairs_interleaved": _case(4, [(0, 2), (1, 3)], [0, 1, 0, 1], [1, 1], [0, 0], [2, 2], [P, P]),
        "two_pairs_nested": _case(4, [(0, 3), (1, 2)], [0, 1, 1, 0], [1, 1], [0, 0], [2, 2], [P, P]),
        "pair_round_a_lone_read": _case(3, [(0, 2)], [0, 1, 0], [1, 0], [0, 0], [2, 0], [P, L]),
        "lone_read_first": _case(3, [(1, 2)], [0, 1, 1], [0, 1], [0, 0], [0, 2], [L, P]),
        "y_of_three_arms": _case(7, [(0, 1), (1, 2), (0, 3), (3, 4), (0, 5), (5, 6)], [0] * 7, [6], [1], [3], [O]),
        "h": _case(6, [(0, 2), (1, 2), (2, 3), (3, 4), (3, 5)], [0] * 6, [5], [2], [4], [O]),
        "lollipop": _case(4, [(0, 1), (1, 2), (0, 2), (2, 3)], [0] * 4, [4], [1], [1], [O]),
        "path_beside_ring": _case(7, [(0, 1), (1, 2), (3, 4), (4, 5), (5, 6), (3, 6)], [0, 0, 0, 1, 1, 1, 1], [2, 4], [0, 0], [2, 0], [P, R]),
        "two_paths_joined_by_the_last_edge": _case(6, [(0, 1), (1, 2), (3, 4), (4, 5), (2, 5)], [0] * 6, [5], [0], [2], [P]),
        "k4": _case(4, [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)], [0] * 4, [6], [4], [0], [O]),
        "bowtie": _case(5, [(0, 1), (0, 2), (1, 2), (2, 3), (2, 4), (3, 4)], [0] * 5, [6], [1], [0], [O]),
        "path5_descending": _case(5, [(4, 3), (3, 2), (2, 1), (1, 0)], [0] * 5, [4], [0], [2], [P]),
        "path5_alternating": _case(5, [(0, 4), (4, 1), (1, 3), (3, 2)], [0] * 5, [4], [0], [2], [P]),
        "three_pairs_numbered_by_smallest_read": _case(6, [(5, 1), (4, 2), (3, 0)], [0, 1, 2, 0, 2, 1], [1, 1, 1], [0, 0, 0], [2, 2, 2], [P, P, P]),
        "star_between_lone_reads": _case(6, [(1, 2), (1, 3), (1, 4)], [0, 1, 1, 1, 1, 2], [0, 3, 0], [0, 1, 0], [0, 3, 0], [L, O, L]),
        "caterpillar3": _case(6, [(0, 1), (1, 2), (0, 3), (1, 4), (2, 5)], [0] * 6, [5], [1], [3], [O]),
        "binary_tree_depth2": _case(7, [(0, 1), (0, 2), (1, 3), (1, 4), (2, 5), (2, 6)], [0] * 7, [6], [2], [4], [O]),
        "ring_lone_pair": _case(6, [(0, 1), (1, 2), (0, 2), (4, 5)], [0, 0, 0, 1, 2, 2], [3, 0, 1], [0, 0, 0], [0, 0, 2], [R, L, P]),
        "square_with_diagonal": _case(4, [(0, 1), (1, 2), (2, 3), (0, 3), (0, 2)], [0] * 4, [5], [2], [0], [O]),
    }


def case_edges(case):
    p = np.array(case["pairs"], dtype=np.int64).reshape(-1, 2)
    return case["M"], p[:, 0], p[:, 1]


def check_case(case, t):
    """The claims of a hand case on a result in the layout of tables()."""
    comp = np.asarray(case["comp"])
    n = int(comp.max()) + 1
    assert np.asarray(t["comp_of_read"]).tolist() == comp.tolist()
    assert np.asarray(t["reads"]).tolist() == np.bincount(comp, minlength=n).tolist()
    assert np.asarray(t["first_read"]).tolist() == [int(np.flatnonzero(comp == c)[0]) for c in range(n)]
    for k in ("edges", "branches", "ends"):
        assert np.asarray(t[k]).tolist() == case[k], k
    assert [shape(int(r), int(b), int(e)) for r, b, e in zip(t["reads"], t["branches"], t["ends"])] == case["shapes"]
