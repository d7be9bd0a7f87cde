"""Helpers for the string-graph tests: hand-made Overlap records, random overlap graphs, layout-shaped overlap graphs (reads placed on
a genome: bands of transitive triangles, planted hubs) with a CPU report of every read's degree in the matrix that reaches the
reduction, and a pure-Python restatement of src/main.cpp:305-312 + src/TransitiveReduction.cpp:3-90 with dense dict-of-dict matrices
that follows the reference statement by statement (loop included).  Independent of oracle/elba_oracle.c: it is what pins the C oracle
on random inputs."""
import numpy as np

from oracle import pyoracle as po

INF = 2**31 - 1
COUNTS = ("bad_reads", "edges_passed", "contained_reads", "edges_kept", "products", "marked", "removed", "nnz", "iterations")


def ov(direction, directionT, suffix, suffixT, passed=1, cq=0, ct=0, direction_none=False, **kw):
    o = np.zeros(1, dtype=po.OVERLAP_DTYPE)[0]
    o["direction"] = -1 if direction_none else direction
    o["directionT"] = -1 if direction_none else directionT
    o["suffix"] = suffix; o["suffixT"] = suffixT; o["passed"] = passed; o["containedQ"] = cq; o["containedT"] = ct
    for k, v in kw.items():
        o[k] = v
    return o


def random_overlaps(rng, M, density=0.3, p_fail=0.1, p_contained=0.02, p_nodir=0.03, suffix_range=3000):
    """Upper-triangular pairs in (row, col) order with random Overlap fields — directions, suffixes and flags are drawn independently
    (not from real alignments): every branch of the semiring and of the prunes gets exercised, which real reads rarely do."""
    rows, cols, vals = [], [], []
    for i in range(M):
        for j in range(i + 1, M):
            if rng.random() >= density:
                continue
            o = np.zeros(1, dtype=po.OVERLAP_DTYPE)[0]
            for f in ("begQ", "begT", "endQ", "endT"):
                o[f] = int(rng.integers(0, 20000))
            o["score"] = int(rng.integers(-1, 9000)); o["rc"] = int(rng.integers(0, 2)); o["kind"] = int(rng.integers(0, 5))
            if rng.random() < p_fail:
                o["direction"] = -1; o["directionT"] = -1
            else:
                o["passed"] = 1
                u = rng.random()
                if u < p_contained:
                    o["containedQ"] = 1; o["direction"] = -1; o["directionT"] = -1
                elif u < 2 * p_contained:
                    o["containedT"] = 1; o["direction"] = -1; o["directionT"] = -1
                elif u < 2 * p_contained + p_nodir:
                    o["direction"] = -1; o["directionT"] = int(rng.integers(0, 4))
                else:
                    o["direction"] = int(rng.integers(0, 4)); o["directionT"] = int(rng.integers(-1, 4))
                    o["suffix"] = int(rng.integers(-200, suffix_range)); o["suffixT"] = int(rng.integers(-200, suffix_range))
            rows.append(i); cols.append(j); vals.append(o)
    return np.array(rows, dtype=np.int64), np.array(cols, dtype=np.int64), np.array(vals, dtype=po.OVERLAP_DTYPE) if vals else np.zeros(0, dtype=po.OVERLAP_DTYPE)


def kept_edges(M, rows, cols, vals, cutoff=0.65):
    """Which input pairs reach TransitiveReduction (passed, no bad end, no contained end) and the read flags (bit 0 bad, bit 1 contained):
    find_bad_reads / find_contained_reads of src/main.cpp:553-583 on whole arrays."""
    rows = np.asarray(rows, dtype=np.int64); cols = np.asarray(cols, dtype=np.int64)
    passed = vals["passed"] != 0
    deg = np.bincount(rows, minlength=M) + np.bincount(cols, minlength=M)
    pas = np.bincount(rows[passed], minlength=M) + np.bincount(cols[passed], minlength=M)
    bad = (pas + 1.0) / (deg + 1.0) <= cutoff
    first = passed & ~bad[rows] & ~bad[cols]
    cont = np.zeros(M, dtype=bool)
    cont[rows[first & (vals["containedQ"] != 0)]] = True
    cont[cols[first & (vals["containedT"] != 0)]] = True
    keep = first & ~cont[rows] & ~cont[cols]
    return keep, bad.astype(np.uint8) | (cont.astype(np.uint8) << 1)


def kept_degrees(M, rows, cols, vals, cutoff=0.65):
    """The generator's report: every read's degree in the symmetrised R that reaches the reduction (its row length there), and the flags."""
    keep, flags = kept_edges(M, rows, cols, vals, cutoff)
    rows = np.asarray(rows, dtype=np.int64); cols = np.asarray(cols, dtype=np.int64)
    return np.bincount(rows[keep], minlength=M) + np.bincount(cols[keep], minlength=M), flags


def layout_overlaps(rng, M, cov, L=10000, hubs=(), p_fail=0.08, p_nodir=0.02, p_contained=0.001, jitter=40, suffix_scale=1, cutoff=0.65):
    """Overlaps of M reads of length L laid out on a genome at coverage cov, upper-triangular in (row, col) order.

    Reads get sorted positions (integer gaps, uniform with mean L / cov) and a random strand s; i < j are a pair when pos[j] - pos[i] < L.
    One convention gives every field, so that a two-edge walk through a read between the two ends is a valid product of MinPlusSR:
    the walk to the right leaves i by tail bit 1 - s_i and enters j by head bit s_j (direction = 2 (1 - s_i) + s_j); the walk to the left
    is its mirror image (directionT: the two bits swapped, 2 s_j + (1 - s_i)), and a walk that turns round in the middle read is refused
    (t2 == h1).  suffix and suffixT are suffix_scale * (pos[j] - pos[i] + a jitter of their own in [-jitter, jitter]): the walk
    i -> k -> j sums to the direct distance give or take the jitters, so with fuzz above 3 * jitter * suffix_scale every pair with a read
    between its ends is transitive, and close pairs have negative suffixes.
    p_fail: the pair did not pass (no directions).  p_contained: containedQ or containedT set, nothing else changed.  p_nodir: one of
    direction / directionT / both is -1.

    hubs = ((read, extra), ...) gives that read `extra` more partners anywhere on the genome, fields by the same convention (suffix = the
    scaled distance), always passed and never contained.  So that the hub's degree after the prunes is known beforehand, the hub itself and
    the partners are taken among the reads that the prunes at `cutoff` keep in the graph without hubs (a passed pair more never makes a
    read bad, so flags and every other kept degree stay what they were); a hub that is bad or contained there is a ValueError.  The
    random draws of the graph without hubs come first: the same seed gives the same graph with and without hubs."""
    M = int(M)
    gap_hi = max(2, 2 * L // cov)
    pos = np.cumsum(rng.integers(1, gap_hi, size=M, dtype=np.int64))
    strand = rng.integers(0, 2, size=M, dtype=np.int64)
    rr, cc = [], []
    for k in range(1, M):
        near = np.flatnonzero(pos[k:] - pos[:-k] < L)
        if len(near) == 0:
            break
        rr.append(near); cc.append(near + k)
    rows = np.concatenate(rr) if rr else np.zeros(0, np.int64)
    cols = np.concatenate(cc) if cc else np.zeros(0, np.int64)
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    n = len(rows)
    u_fail, u_cont, u_nodir = rng.random(n), rng.random(n), rng.random(n)
    jit = rng.integers(-jitter, jitter + 1, size=(2, n), dtype=np.int64)
    filler = rng.integers(0, L, size=(6, n), dtype=np.int64)

    def fields(rows, cols, jit, filler, u_nodir):
        v = np.zeros(len(rows), dtype=po.OVERLAP_DTYPE)
        dist = pos[cols] - pos[rows]
        sfx = suffix_scale * (dist + jit[0]); sfxT = suffix_scale * (dist + jit[1])
        assert len(rows) == 0 or max(np.abs(sfx).max(), np.abs(sfxT).max()) < 2**31, "suffixes must fit an int32"
        v["suffix"] = sfx; v["suffixT"] = sfxT
        v["direction"] = 2 * (1 - strand[rows]) + strand[cols]
        v["directionT"] = 2 * strand[cols] + (1 - strand[rows])
        which = (u_nodir / max(p_nodir, 1e-300) * 3).astype(np.int64)          # 0, 1, 2 below p_nodir
        v["direction"][(u_nodir < p_nodir) & (which != 1)] = -1
        v["directionT"][(u_nodir < p_nodir) & (which != 0)] = -1
        v["passed"] = 1
        v["rc"] = strand[rows] ^ strand[cols]
        v["begQ"] = filler[0]; v["endQ"] = filler[0] + filler[1]; v["begT"] = filler[2]; v["endT"] = filler[2] + filler[3]
        v["score"] = filler[4]; v["kind"] = filler[5] % 5
        return v

    vals = fields(rows, cols, jit, filler, u_nodir)
    failed = u_fail < p_fail
    for f in ("direction", "directionT"):
        vals[f][failed] = -1
    for f in ("passed", "suffix", "suffixT"):
        vals[f][failed] = 0
    vals["containedQ"][~failed & (u_cont < p_contained)] = 1
    vals["containedT"][~failed & (u_cont >= p_contained) & (u_cont < 2 * p_contained)] = 1
    if not hubs:
        return rows, cols, vals
    deg, flags = kept_degrees(M, rows, cols, vals, cutoff)
    hub_ids = [int(h) for h, _ in hubs]
    free = (flags == 0) & (deg > 0)
    if not all(free[h] for h in hub_ids):
        raise ValueError("layout_overlaps: a hub read is bad, contained or without edges in the graph without hubs")
    free[hub_ids] = False
    xr, xc = [], []
    for h, extra in hubs:
        cand = free.copy()
        cand[cols[rows == h]] = False; cand[rows[cols == h]] = False
        cand = np.flatnonzero(cand)
        partners = rng.choice(cand, size=int(extra), replace=False)
        xr.append(np.minimum(partners, h)); xc.append(np.maximum(partners, h))
    xr = np.concatenate(xr); xc = np.concatenate(xc)
    m = len(xr)
    xv = fields(xr, xc, rng.integers(-jitter, jitter + 1, size=(2, m), dtype=np.int64), rng.integers(0, L, size=(6, m), dtype=np.int64), rng.random(m))
    rows = np.concatenate([rows, xr]); cols = np.concatenate([cols, xc]); vals = np.concatenate([vals, xv])
    order = np.lexsort((cols, rows))
    return rows[order], cols[order], vals[order]


def layout_with_hub_degrees(seed, M, cov, hub_degrees, cutoff=0.65, **kw):
    """layout_overlaps with hubs whose degree after the prunes is exactly hub_degrees = ((read, degree), ...): the graph without hubs
    is generated first from the same seed to see what each hub has already."""
    rows, cols, vals = layout_overlaps(np.random.default_rng(seed), M, cov, cutoff=cutoff, **kw)
    deg, _ = kept_degrees(M, rows, cols, vals, cutoff)
    hubs = tuple((int(h), int(d) - int(deg[h])) for h, d in hub_degrees)
    return layout_overlaps(np.random.default_rng(seed), M, cov, hubs=hubs, cutoff=cutoff, **kw)


def small_suffixes(rng, vals, hi=5):
    """The tie graph: suffix and suffixT of every passed pair redrawn from {0 .. hi-1}, so that suffix + fuzz == the best walk is common."""
    vals = vals.copy()
    ok = vals["passed"] != 0
    vals["suffix"][ok] = rng.integers(0, hi, size=int(ok.sum())); vals["suffixT"][ok] = rng.integers(0, hi, size=int(ok.sum()))
    return vals


def relabel(perm, rows, cols, vals):
    """The same graph with read v renamed perm[v]: pairs whose ends change order are stored as their Overlap::Transpose; (row, col) order."""
    perm = np.asarray(perm, dtype=np.int64)
    r, c = perm[np.asarray(rows, dtype=np.int64)], perm[np.asarray(cols, dtype=np.int64)]
    flip = r > c
    v = vals.copy()
    for a, b in (("begQ", "begT"), ("endQ", "endT"), ("suffix", "suffixT"), ("direction", "directionT"), ("containedQ", "containedT")):
        v[a][flip] = vals[b][flip]; v[b][flip] = vals[a][flip]
    r, c = np.where(flip, c, r), np.where(flip, r, c)
    order = np.lexsort((c, r))
    return r[order], c[order], v[order]


def assert_mapped(perm, S, flags, st, P, pflags, pst):
    """P (po.string_graph of the relabelled graph) is S (of the original) with read v renamed perm[v], in P's own (col, row) order."""
    perm = np.asarray(perm, dtype=np.int64)
    assert pst == st and (pflags[perm] == flags).all()
    r, c = perm[S["rows"]], perm[S["cols"]]
    order = np.lexsort((r, c))
    assert P["n"] == S["n"] and (P["rows"] == r[order]).all() and (P["cols"] == c[order]).all()
    for f in po.OVERLAP_DTYPE.names:
        if f != "pad":
            assert (P["vals"][f] == S["vals"][f][order]).all(), f


def best_walks(M, rows, cols, vals, cutoff, fuzz):
    """For every directed entry of the symmetrised R that reaches the reduction, the smallest valid two-edge walk that lands in the slot
    of its direction (None when there is none), by plain dictionaries.  Returns (directed entries, with a walk and suffix + fuzz >= it,
    with suffix + fuzz == it): the second is the reduction's `marked`, the third counts the exact ties."""
    keep, _ = kept_edges(M, rows, cols, vals, cutoff)
    adj = {}
    for a in np.flatnonzero(keep):
        i, j, v = int(rows[a]), int(cols[a]), vals[a]
        adj.setdefault(i, {})[j] = (int(v["direction"]), int(v["suffix"]))
        adj.setdefault(j, {})[i] = (int(v["directionT"]), int(v["suffixT"]))
    directed = marked = ties = 0
    for i, ri in adj.items():
        for j, (d, s) in ri.items():
            if d == -1:
                continue
            directed += 1
            best = None
            rj = adj[j]
            for k, (d1, s1) in ri.items():
                if d1 == -1 or k not in rj:
                    continue
                d2, s2 = adj[k][j]
                if d2 == -1 or ((d2 >> 1) & 1) == (d1 & 1) or 2 * ((d1 >> 1) & 1) + (d2 & 1) != d:
                    continue
                best = s1 + s2 if best is None else min(best, s1 + s2)
            if best is not None and s + fuzz >= best:
                marked += 1
                ties += s + fuzz == best
    return directed, marked, ties


def assert_same_as_oracle(e, nreads, rows, cols, vals, cutoff=0.65, fuzz=1000, want=None):
    """Run the reduction on the engine and hold it against po.string_graph bit for bit: the entries of S in the reference's output order,
    every field, the read flags and the nine counts.  `want` is po.string_graph's result for the same arguments when the caller has it."""
    st = e.transitive_reduction(cutoff, fuzz)
    g = e.export_string_graph()
    S, flags, ost = want if want is not None else po.string_graph(nreads, rows, cols, vals, cutoff=cutoff, fuzz=fuzz)
    for key in COUNTS:
        assert st[key] == ost[key], (key, st, ost)
    assert st["nreads"] == nreads and st["nedges"] == len(rows)
    assert g["n"] == S["n"] and (g["rows"] == S["rows"]).all() and (g["cols"] == S["cols"]).all()
    for f in po.OVERLAP_DTYPE.names:
        if f != "pad":
            assert (g["vals"][f] == S["vals"][f]).all(), f
    assert (e.export_read_flags(nreads) == flags).all()
    return st


def transpose(o):
    """Overlap::Transpose, include/Overlap.hpp:43-69."""
    t = o.copy()
    t["begQ"], t["begT"] = o["begT"], o["begQ"]
    t["endQ"], t["endT"] = o["endT"], o["endQ"]
    t["suffix"], t["suffixT"] = o["suffixT"], o["suffix"]
    t["direction"], t["directionT"] = o["directionT"], o["direction"]
    t["containedQ"], t["containedT"] = o["containedT"], o["containedQ"]
    return t


def _multiply(e1, e2):
    """MinPlusSR::multiply (include/TransitiveReduction.hpp:88-104) on (direction, suffix, paths) triples."""
    out = [INF] * 4
    if e1[0] == -1 or e2[0] == -1:
        return out
    t1, h1, t2, h2 = (e1[0] >> 1) & 1, e1[0] & 1, (e2[0] >> 1) & 1, e2[0] & 1
    if t2 == h1:
        return out
    out[2 * t1 + h2] = e1[1] + e2[1]
    return out


def python_string_graph(M, rows, cols, vals, cutoff, fuzz):
    rows = [int(r) for r in rows]; cols = [int(c) for c in cols]
    # find_bad_reads (src/main.cpp:553-571)
    deg = [0] * M; pas = [0] * M
    for r, c, v in zip(rows, cols, vals):
        deg[r] += 1; deg[c] += 1
        if v["passed"]:
            pas[r] += 1; pas[c] += 1
    bad = [(pas[v] + 1) / (float(deg[v]) + 1) <= cutoff for v in range(M)]
    R = {(r, c): v for r, c, v in zip(rows, cols, vals) if v["passed"] and not bad[r] and not bad[c]}
    st = dict(bad_reads=sum(bad), edges_passed=len(R))
    # find_contained_reads (:573-583)
    cont = [False] * M
    for (r, c), v in R.items():
        if v["containedQ"]:
            cont[r] = True
        if v["containedT"]:
            cont[c] = True
    R = {(r, c): v for (r, c), v in R.items() if not cont[r] and not cont[c]}
    st.update(contained_reads=sum(cont), edges_kept=len(R))
    flags = [int(b) | (int(c) << 1) for b, c in zip(bad, cont)]
    # TransitiveReduction
    for (r, c), v in list(R.items()):
        R[(c, r)] = transpose(v)
    Rm = {key: (int(v["direction"]), int(v["suffix"])) for key, v in R.items()}
    rowsof = {}
    for (r, c) in Rm:
        rowsof.setdefault(r, []).append(c)
    P = dict(Rm)
    T = set()
    iters = 0
    first = None
    while True:
        prev = len(T)
        N = {}
        products = 0
        for (i, k), e1 in P.items():
            for j in rowsof.get(k, ()):
                prod = _multiply(e1, Rm[(k, j)])
                products += 1
                cur = N.get((i, j))
                N[(i, j)] = prod if cur is None else [min(a, b) for a, b in zip(cur, prod)]
        N = {key: p for key, p in N.items() if any(x < INF for x in p)}
        Ipat = set()
        for key, (d, s) in Rm.items():
            if key in N and d != -1 and s + fuzz >= N[key][d]:
                Ipat.add(key)
        if first is None:
            first = dict(products=products, nnzN=len(N), marked=len(Ipat))
        Ipat |= {(c, r) for (r, c) in Ipat}
        T |= Ipat
        P = {key: (-1, 0) for key in N}                 # entries of N come out of Overlap(): direction -1, suffix 0
        iters += 1
        if len(T) == prev:
            break
    S = [(r, c, v) for (r, c), v in R.items() if (r, c) not in T and v["direction"] != -1]
    S.sort(key=lambda t: (t[1], t[0]))
    st.update(first)
    st.update(removed=len(T), nnz=len(S), iterations=iters)
    return S, flags, st
