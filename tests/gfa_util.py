"""The assembly graph (elba_export_assembly_links; the rule is stated in include/elba_amd.h) restated twice in Python, a tiny GFA 1 parser,
hand cases with their claims, and a ground-truth generator.  The two restatements share nothing with elba_amd/csrc/graph_links.hip nor with
each other: links_walk is a literal walk over the edges with dicts and reads, for the pair u < v, the entry stored in column u (row v) and
transposes it as the contig walk does; links_tables is vectorised numpy over end tables and reads the entry of the upper triangle (row u,
column v) as it is.  On an S that holds Overlap::Transpose images of its entries (every S the tests build) the two are the same steps.

Both take the same `inp` dict (inputs_of_export / inputs_of_restatement): M, base, rows, cols, vals (S, export order), chain_off,
chain_read, chain_strand, kinds, read_contig, lens (bases per read), seq_off (bases per contig), and return (records, stats): records as
a LINK array sorted by (from_read, to_read), stats as the dict of elba_graph_stats without its time."""
import numpy as np

import contig_ex_util as cx
import contig_util as cu
from oracle import pyoracle as po

LINK = np.dtype([("from", "<u4"), ("to", "<u4"), ("from_read", "<u4"), ("to_read", "<u4"), ("overlap", "<i4"), ("from_rev", "u1"), ("to_rev", "u1"),
                 ("flags", "u1"), ("reserved", "u1")])
STATS = ("segments", "candidates", "links", "closures", "twisted", "unplaced", "clamped", "asymmetric")
CLOSURE = 1


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def inputs_of_export(g, got, read_contig, lens, base=0):
    """From Engine.export_string_graph(), Engine.export_contigs(), Engine.export_read_contigs(M) and the read lengths."""
    return dict(M=len(lens), base=base, rows=np.asarray(g["rows"]), cols=np.asarray(g["cols"]), vals=g["vals"], chain_off=np.asarray(got["chain_off"], dtype=np.int64),
                chain_read=np.asarray(got["chain_read"], dtype=np.int64), chain_strand=np.asarray(got["chain_strand"], dtype=np.uint8),
                kinds=np.asarray(got["kinds"], dtype=np.uint8), read_contig=np.asarray(read_contig, dtype=np.int64), lens=np.asarray(lens, dtype=np.int64),
                seq_off=np.asarray(got["seq_off"], dtype=np.int64))


def inputs_of_restatement(M, rows, cols, vals, seqs, flags, read_flags=None):
    """S (both triangles, export order) and reads -> the contigs of contig_ex_util.generate_contigs_ex -> (inp, contigs)."""
    contigs, chains, kinds, read_contig, _ = cx.generate_contigs_ex(M, rows, cols, vals, seqs, flags, read_flags)
    flat = [el for ch in chains for el in ch]
    inp = dict(M=M, base=0, rows=np.asarray(rows), cols=np.asarray(cols), vals=vals,
               chain_off=np.concatenate([[0], np.cumsum([len(c) for c in chains])]).astype(np.int64),
               chain_read=np.array([r for r, _, _ in flat], dtype=np.int64), chain_strand=np.array([s for _, _, s in flat], dtype=np.uint8),
               kinds=np.array(kinds, dtype=np.uint8), read_contig=np.array(read_contig, dtype=np.int64), lens=np.array([len(s) for s in seqs], dtype=np.int64),
               seq_off=np.concatenate([[0], np.cumsum([len(c) for c in contigs])]).astype(np.int64))
    return inp, contigs


def _records(recs):
    out = np.zeros(len(recs), dtype=LINK)
    for i, r in enumerate(sorted(recs, key=lambda r: (r[2], r[3]))):
        out[i] = tuple(r) + (0,)
    return out


# ---- restatement 1: a walk over the edges ------------------------------------------------------------------------------------------
def links_walk(inp):
    base = inp["base"]
    column = {}                                                  # column[u][v] = the entry stored at (row v, column u)
    for r, c, o in zip(inp["rows"], inp["cols"], inp["vals"]):
        column.setdefault(int(c) - base, {})[int(r) - base] = o
    chains = [[(int(inp["chain_read"][e]) - base, int(inp["chain_strand"][e])) for e in range(int(a), int(b))] for a, b in zip(inp["chain_off"][:-1], inp["chain_off"][1:])]
    where = {}                                                   # read -> (contig, place in its chain, strand bit)
    for k, ch in enumerate(chains):
        for i, (r, s) in enumerate(ch):
            where[r] = (k, i, s)
    seglen = [int(b - a) for a, b in zip(inp["seq_off"][:-1], inp["seq_off"][1:])]
    st = dict.fromkeys(STATS, 0)
    st["segments"] = len(chains)
    recs = []
    for k, ch in enumerate(chains):
        if int(inp["kinds"][k]) == cx.CIRCLE:
            s = ch[0][0] + base
            recs.append((k, k, s, s, 0, 0, 0, CLOSURE))
            st["closures"] += 1
    for u in sorted(column):
        for v in sorted(column[u]):
            if v <= u or (len(column[u]) <= 2 and len(column.get(v, {})) <= 2):
                continue
            st["candidates"] += 1
            if u not in where or v not in where:
                st["unplaced"] += 1
                continue
            t = cu.transpose(column[u][v])                       # S(u, v), what the contig walk reads at u
            d, p_uv, d_back, p_vu = int(t["direction"]) & 3, int(t["suffixT"]), int(t["directionT"]) & 3, int(t["suffix"])
            u_reversed, v_as_stored = bool(d & 2), bool(d & 1)
            (ku, iu, su), (kv, iv, sv) = where[u], where[v]
            nu, nv = len(chains[ku]), len(chains[kv])
            # leaving side
            if nu == 1:
                from_rev = int(u_reversed)
            elif iu == nu - 1 and u_reversed == bool(su):        # last, leaves in the orientation it has in the chain
                from_rev = 0
            elif iu == 0 and u_reversed != bool(su):             # first, leaves in the other orientation
                from_rev = 1
            else:
                st["twisted"] += 1
                continue
            # entering side
            v_in_chain_orientation = v_as_stored == (sv == 0)
            if iv == 0 and v_in_chain_orientation:
                to_rev = 0
            elif iv == nv - 1 and not v_in_chain_orientation:
                to_rev = 1
            else:
                st["twisted"] += 1
                continue
            raw = min(int(inp["lens"][u]) - p_uv, int(inp["lens"][v]) - p_vu)
            ov = max(0, min(raw, seglen[ku], seglen[kv]))
            st["clamped"] += ov != raw
            # the reverse complement of the step leaves v flipped from how it was entered and enters u flipped from how it was left
            st["asymmetric"] += not (bool(d_back & 2) == v_as_stored and bool(d_back & 1) == u_reversed)
            st["links"] += 1
            recs.append((ku, kv, u + base, v + base, ov, from_rev, to_rev, 0))
    return _records(recs), st


# ---- restatement 2: end tables, vectorised -----------------------------------------------------------------------------------------
def links_tables(inp):
    M, base = inp["M"], inp["base"]
    rows, cols, vals = inp["rows"] - base, inp["cols"] - base, inp["vals"]
    deg = np.bincount(cols, minlength=M) if len(cols) else np.zeros(M, dtype=np.int64)
    co, cr = inp["chain_off"], inp["chain_read"] - base
    first, last, strand = np.zeros(M, dtype=bool), np.zeros(M, dtype=bool), np.zeros(M, dtype=np.int64)
    if len(co) > 1:
        first[cr[co[:-1]]] = True; last[cr[co[1:] - 1]] = True
        strand[cr] = inp["chain_strand"]
    rc = inp["read_contig"]
    seglen = np.diff(inp["seq_off"])
    up = rows < cols
    u, v, o = rows[up], cols[up], vals[up]
    cand = (deg[u] > 2) | (deg[v] > 2)
    u, v, o = u[cand], v[cand], o[cand]
    placed = (rc[u] >= 0) & (rc[v] >= 0)
    d, back = o["direction"].astype(np.int64) & 3, o["directionT"].astype(np.int64) & 3
    urev, vrev = d >> 1, 1 - (d & 1)
    f_plus = last[u] & (urev == strand[u]); f_minus = first[u] & (urev != strand[u])
    t_plus = first[v] & (vrev == strand[v]); t_minus = last[v] & (vrev != strand[v])
    ok = placed & (f_plus | f_minus) & (t_plus | t_minus)
    st = dict(segments=len(seglen), candidates=int(cand.sum()), links=int(ok.sum()), closures=int((inp["kinds"] == cx.CIRCLE).sum()),
              twisted=int((placed & ~ok).sum()), unplaced=int((~placed).sum()))
    u, v, o, d, back = u[ok], v[ok], o[ok], d[ok], back[ok]
    raw = np.minimum(inp["lens"][u] - o["suffixT"].astype(np.int64), inp["lens"][v] - o["suffix"].astype(np.int64))
    ov = np.clip(raw, 0, np.minimum(seglen[rc[u]], seglen[rc[v]])) if len(u) else raw
    st["clamped"] = int((ov != raw).sum())
    st["asymmetric"] = int((back != (((d & 1) << 1) | (d >> 1))).sum())
    circ = np.nonzero(inp["kinds"] == cx.CIRCLE)[0]
    out = np.zeros(len(u) + len(circ), dtype=LINK)
    n = len(u)
    out["from"][:n] = rc[u]; out["to"][:n] = rc[v]; out["from_read"][:n] = u + base; out["to_read"][:n] = v + base; out["overlap"][:n] = ov
    out["from_rev"][:n] = ~f_plus[ok]; out["to_rev"][:n] = ~t_plus[ok]
    out["from"][n:] = circ; out["to"][n:] = circ; out["flags"][n:] = CLOSURE
    if len(circ):
        out["from_read"][n:] = inp["chain_read"][co[circ]]; out["to_read"][n:] = inp["chain_read"][co[circ]]
    return out[np.lexsort((out["to_read"], out["from_read"]))], st


def same_records(a, b):
    return len(a) == len(b) and a.tobytes() == b.tobytes()


# ---- the sequence property ---------------------------------------------------------------------------------------------------------
def oriented(contigs, k, rev):
    return cu.revcomp(contigs[k]) if rev else contigs[k]


def sequence_property_failures(contigs, recs):
    """The edge links whose oriented from-segment does not end with the `overlap` bases the oriented to-segment begins with."""
    bad = []
    for r in recs:
        if int(r["flags"]) & CLOSURE:
            continue
        a, b, n = oriented(contigs, int(r["from"]), int(r["from_rev"])), oriented(contigs, int(r["to"]), int(r["to_rev"])), int(r["overlap"])
        if n > min(len(a), len(b)) or a[len(a) - n:] != b[:n]:
            bad.append(tuple(r))
    return bad


# ---- GFA 1 -------------------------------------------------------------------------------------------------------------------------
def parse_gfa(path):
    """(version, segments [(name, sequence, {tag: value})], links [(from, '+'/'-', to, '+'/'-', overlap in bases)])."""
    version, segs, links = None, [], []
    with open(path, "rb") as f:
        data = f.read()
    assert data.endswith(b"\n")
    for line in data.decode("ascii").split("\n")[:-1]:
        t = line.split("\t")
        if t[0] == "H":
            assert version is None and t[1].startswith("VN:Z:")
            version = t[1][5:]
        elif t[0] == "S":
            tags = {}
            for x in t[3:]:
                name, typ, val = x.split(":", 2)
                tags[name] = int(val) if typ == "i" else val
            segs.append((t[1], t[2], tags))
        elif t[0] == "L":
            assert len(t) == 6 and t[2] in "+-" and t[4] in "+-" and t[5].endswith("M")
            links.append((t[1], t[2], t[3], t[4], int(t[5][:-1])))
        else:
            raise AssertionError("unknown GFA line %r" % line)
    return version, segs, links


def gfa_components(segs, links):
    parent = {name: name for name, _, _ in segs}

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, _, b, _, _ in links:
        parent[find(a)] = find(b)
    return len({find(x) for x in parent})


# ---- hand cases --------------------------------------------------------------------------------------------------------------------
def swap(d):
    return ((d & 1) << 1) | (d >> 1)


def E(d, p_qt=60, p_tq=60, dT=None):
    """The entry at (Q, T), Q < T: the step Q -> T has direction d and prefix p_qt, the step T -> Q direction dT (default: the reverse
    complement of Q -> T) and prefix p_tq."""
    o = np.zeros(1, dtype=po.OVERLAP_DTYPE)[0]
    o["passed"] = 1
    o["direction"], o["directionT"] = d, swap(d) if dT is None else dT
    o["suffixT"], o["suffix"] = p_qt, p_tq
    return o


def _case(M, edges, claims, flags=3, lens=None, read_flags=None):
    return dict(M=M, edges=edges, claims=claims, flags=flags, lens=[100] * M if lens is None else lens, read_flags=read_flags)


def _star(d01=1, d02=1, d03=1, **kw):
    """Branch read 0 with the three lone reads 1, 2, 3."""
    return {(0, 1): E(d01, **kw), (0, 2): E(d02), (0, 3): E(d03)}


def _rec(recs, u, v):
    hit = recs[(recs["from_read"] == u) & (recs["to_read"] == v)]
    assert len(hit) == 1, (u, v, recs)
    return hit[0]


def hand_cases():
    """name -> dict(M, edges {(i, j): entry}, flags, lens, read_flags, claims(records, stats, read_contig)).  Reads have 100 bases and every
    step takes a prefix of 60 (an overlap of 40) unless the case says otherwise."""
    cases = {}
    # a Y: the paths 0-1, 2-3, 4-5 end at the branch read 6.  Under the code d of the steps x -> 6 the chains are laid so that their last
    # reads leave as they are in the chain (step 0 -> 1 enters 1 reversed iff d & 2): three links contig -> the branch's own segment,
    # from '+', to '-' iff the branch is not entered as stored
    for d in range(4):
        inner = 1 - (d >> 1)                                    # the step 0 -> 1 enters 1 as stored iff 1 then leaves unreversed
        edges = {(0, 1): E(inner), (2, 3): E(inner), (4, 5): E(inner), (1, 6): E(d), (3, 6): E(d), (5, 6): E(d)}

        def claims(recs, st, rc, d=d):
            assert st["candidates"] == st["links"] == 3 and st["twisted"] == st["unplaced"] == st["clamped"] == st["asymmetric"] == st["closures"] == 0
            assert st["segments"] == 4 and recs["from_read"].tolist() == [1, 3, 5] and recs["to_read"].tolist() == [6, 6, 6]
            assert recs["from"].tolist() == [rc[1], rc[3], rc[5]] and (recs["to"] == rc[6]).all() and len({rc[1], rc[3], rc[5], rc[6]}) == 4
            assert (recs["from_rev"] == 0).all() and (recs["to_rev"] == 1 - (d & 1)).all() and (recs["overlap"] == 40).all()
        cases["y_code_%d" % d] = _case(7, edges, claims)
    # the same Y with chains that carry their last read the other way: the edge then hangs on the inner side of the last read
    edges = {(0, 1): E(1), (2, 3): E(1), (4, 5): E(1), (1, 6): E(2), (3, 6): E(1), (5, 6): E(1)}

    def claims(recs, st, rc):
        assert st["candidates"] == 3 and st["twisted"] == 1 and st["links"] == 2 and recs["from_read"].tolist() == [3, 5]
    cases["twisted_end"] = _case(7, edges, claims)
    # two branch reads joined: 6 (arms 0-1, 2-3) and 7 (arms 4-5 and, past the diagonal, 8-9): the joint is a link between two one-read
    # segments, and 7 -> 8 enters a chain at its first read
    edges = {(0, 1): E(1), (2, 3): E(1), (4, 5): E(1), (8, 9): E(1), (1, 6): E(1), (3, 6): E(1), (6, 7): E(1), (5, 7): E(1), (7, 8): E(1)}

    def claims(recs, st, rc):
        assert st["candidates"] == st["links"] == 5 and st["segments"] == 6
        assert list(zip(recs["from_read"].tolist(), recs["to_read"].tolist())) == [(1, 6), (3, 6), (5, 7), (6, 7), (7, 8)]
        j = _rec(recs, 6, 7)
        assert (j["from"], j["to"], j["from_rev"], j["to_rev"]) == (rc[6], rc[7], 0, 0)
        k = _rec(recs, 7, 8)
        assert (k["from"], k["to"], k["from_rev"], k["to_rev"]) == (rc[7], rc[8], 0, 0) and rc[8] == rc[9]
    cases["two_branches_joined"] = _case(10, edges, claims)
    # the same joint entered against the chain 8-9: 8 is first but is entered reversed while the chain holds it as stored
    edges = dict(edges); edges[(7, 8)] = E(0)

    def claims(recs, st, rc):
        assert st["twisted"] == 1 and st["links"] == 4
    cases["two_branches_joined_twisted_entry"] = _case(10, edges, claims)
    # a path end and a lone read whose only neighbours are branches: path 0-1 ends at branch 5 (1, 2, 3); the lone read 2 sits between
    # the branches 5 and 6 (2, 4, 7); 3, 4 and 7 are lone as well
    edges = {(0, 1): E(1), (1, 5): E(1), (2, 5): E(1), (3, 5): E(1), (2, 6): E(1), (4, 6): E(1), (6, 7): E(1)}

    def claims(recs, st, rc):
        assert st["candidates"] == st["links"] == 6 and st["unplaced"] == 0 and (np.asarray(rc) >= 0).all() and st["segments"] == 7
        assert sorted(recs["to"][recs["from_read"] == 2].tolist()) == sorted([rc[5], rc[6]])
    cases["path_end_and_lone_read"] = _case(8, edges, claims)
    # a one-read chain left reversed: the branch read 0 leaves towards 2 reverse-complemented and enters it against its stored form,
    # and leaves towards 3 reverse-complemented and enters it as stored
    def claims(recs, st, rc):
        a, b, c = _rec(recs, 0, 1), _rec(recs, 0, 2), _rec(recs, 0, 3)
        assert (a["from_rev"], a["to_rev"]) == (0, 0) and (b["from_rev"], b["to_rev"]) == (1, 1) and (c["from_rev"], c["to_rev"]) == (1, 0)
        assert st["links"] == 3 and st["twisted"] == 0
    cases["one_read_chain_left_reversed"] = _case(4, _star(d02=2, d03=3), claims)
    # an asymmetric loaded edge: 1 -> 0 claims to leave 1 unreversed although 0 -> 1 entered it as stored ... and to enter 0 reversed
    def claims(recs, st, rc):
        assert st["links"] == 3 and st["asymmetric"] == 1
    cases["asymmetric_edge"] = _case(4, _star(dT=0), claims)
    # prefixes beyond the read: a negative overlap becomes 0
    def claims(recs, st, rc):
        assert st["clamped"] == 1 and _rec(recs, 0, 1)["overlap"] == 0 and _rec(recs, 0, 2)["overlap"] == 40
    cases["negative_overlap"] = _case(4, _star(p_qt=150), claims)
    # negative prefixes: an overlap longer than both reads stops at the shorter segment
    def claims(recs, st, rc):
        assert st["clamped"] == 1 and _rec(recs, 0, 1)["overlap"] == 70
    cases["overlap_beyond_a_segment"] = _case(4, _star(p_qt=-30, p_tq=-30), claims, lens=[100, 70, 100, 100])
    # ... and without any bad prefix: the chain 0 -> 1 takes 5 bases of read 0 and the 10 of read 1, so its contig has 15 bases, fewer
    # than the 40 that read 0 shares with the branch 2 on its other side
    edges = {(0, 1): E(1, 5, 5), (0, 2): E(2), (2, 3): E(1), (2, 4): E(1)}

    def claims(recs, st, rc):
        r = _rec(recs, 0, 2)
        assert (r["from_rev"], r["to_rev"], r["overlap"]) == (1, 1, 15) and st["clamped"] == 1 and st["links"] == 3
    cases["overlap_longer_than_a_short_contig"] = _case(5, edges, claims, lens=[100, 10, 100, 100, 100])
    # a circular contig beside a branch, under every flag combination.  Reads of a cycle touch no candidate and a flagged or empty read
    # has no entry or no contig under any flags, so `unplaced` can differ between flags only through the branch and lone reads: it is
    # 3 without ELBA_CONTIG_SINGLETONS and 0 with it
    ring = {(0, 1): E(1), (1, 2): E(1), (2, 3): E(1), (0, 3): E(2)}
    ring.update({(4, 5): E(1), (4, 6): E(1), (4, 7): E(1)})
    for flags in range(4):
        def claims(recs, st, rc, flags=flags):
            assert st["candidates"] == 3 and st["closures"] == (flags & 1) and st["unplaced"] == (0 if flags & 2 else 3) and st["links"] == (3 if flags & 2 else 0)
            assert st["segments"] == (flags & 1) + (4 if flags & 2 else 0)
            if flags & 1:
                c = recs[0]
                assert (c["from"], c["to"], c["from_read"], c["to_read"], c["overlap"], c["from_rev"], c["to_rev"], c["flags"]) == (rc[0], rc[0], 0, 0, 0, 0, 0, 1)
                assert (recs["flags"][1:] == 0).all()
        cases["circle_beside_a_branch_flags_%d" % flags] = _case(8, ring, claims, flags=flags)
    return cases


def case_graph(case):
    """(rows, cols, vals) of a hand case's S, both triangles, export order; and reads of the case's lengths."""
    rng = np.random.default_rng(7)
    seqs = [cx.random_genome(rng, n) for n in case["lens"]]
    return cu.symmetric(case["edges"]), seqs


def clipped_case():
    """A graph after clip_tips: branch 0 holds the lone read 1 and the arms 2-3-4 and 5-6-7; tips of one read are clipped, so read 1
    leaves S with flag 4, 0 falls to degree 2 and the whole graph is one path.  No candidate is left, the flagged read is in no contig."""
    import tip_util as tu
    edges = {(0, 1): E(1), (0, 2): E(1), (2, 3): E(1), (3, 4): E(1), (0, 5): E(1), (5, 6): E(1), (6, 7): E(1)}
    rows, cols, vals = cu.symmetric(edges)
    r2, c2, v2, flags, _ = tu.clip_tips(8, rows, cols, vals, 1, 1)
    return (rows, cols, vals), (np.asarray(r2), np.asarray(c2), v2), flags


# ---- ground truth ------------------------------------------------------------------------------------------------------------------
def truth_graph(rng, glen, n, skips, ids=None, rc=None, drop_middle=False, at_ends=False):
    """A linear genome of glen bases at error 0, cut into n reads laid out as contig_ex_util.layout_reads lays them (read i overlaps
    read i + 1 and ends before read i + 2 begins), except that for i in `skips` read i reaches into read i + 2 as well: the true skip
    edge i <-> i + 2, which makes i and i + 2 branches.  rc marks the reads stored reverse-complemented (default: a random half), read
    i of the layout gets the id ids[i] (default: a random permutation).  Every edge comes from the layout alone: for the step x -> y,
    direction = 2 * (x is emitted reverse-complemented) + (y is emitted as stored); with the layout the prefix is the difference of
    the starts, against it the difference of the ends.
    drop_middle: the true edge (i + 1, i + 2) is left out at every skip, so the graph has no triangle and a transitive reduction at
    fuzz 0 keeps every entry (the full graph's skip edges are transitive by construction: prefixes along the genome add up exactly).
    Read i is still a branch (i - 1, i + 1, i + 2), so i >= 1 then; i + 2 is one when i + 2 is in `skips` too.
    A skip needs a read before i and, unless the middle edge is dropped, one behind i + 2: at the genome's ends only one of the three
    reads gets a third neighbour and the skip edge hangs on the inner side of a path end (at_ends allows that: a twisted edge).
    Returns (genome, seqs by id, edges {(a, b): entry} with a < b, ids, rc)."""
    assert n >= 4 and all(0 <= i and i + 2 <= n - 1 for i in skips)
    assert at_ends or all(1 <= i and i + 2 <= (n - 1 if drop_middle else n - 2) for i in skips)
    genome = cx.random_genome(rng, glen)
    gaps = 8 + rng.multinomial(glen - 8 * n, np.ones(n) / n)    # start-to-start distances (the last: to the genome's end), each >= 8
    p = np.concatenate([[0], np.cumsum(gaps)]).astype(np.int64)  # p[n] = glen
    ov = [int(rng.integers(2, gaps[i + 1])) for i in range(n - 1)]               # read i reaches ov[i] bases into read i + 1, not into i + 2
    e = [int(p[i + 1]) + ov[i] for i in range(n - 1)] + [glen]
    for i in sorted(skips):
        e[i] = int(p[i + 2]) + int(rng.integers(1, ov[i + 1]))      # into read i + 2, ending before read i + 1 ends
    assert all(e[i] < e[i + 1] for i in range(n - 1)) and all(e[i] > p[i + 1] for i in range(n - 1))
    ids = rng.permutation(n) if ids is None else np.asarray(ids)
    if rc is None:
        rc = np.zeros(n, dtype=bool)
        rc[rng.permutation(n)[:n // 2]] = True
    seqs = {}
    for i in range(n):
        s = genome[int(p[i]):e[i]]
        seqs[int(ids[i])] = cu.revcomp(s) if rc[i] else s
    pairs = [(i, i + 1) for i in range(n - 1) if not (drop_middle and i - 1 in skips)] + [(i, i + 2) for i in sorted(skips)]
    edges = {}
    for i, j in pairs:
        assert e[i] > p[j]                                       # they do overlap
        fwd = (2 * int(rc[i]) + (1 - int(rc[j])), int(p[j] - p[i]))              # the step i -> j, with the layout
        back = (2 * (1 - int(rc[j])) + int(rc[i]), e[j] - e[i])                  # the step j -> i, against it
        x, y = int(ids[i]), int(ids[j])
        q2t, t2q = (fwd, back) if x < y else (back, fwd)
        edges[(min(x, y), max(x, y))] = E(q2t[0], q2t[1], t2q[1], dT=t2q[0])
    return genome, [seqs[v] for v in range(n)], edges, ids, rc
