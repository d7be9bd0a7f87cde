"""A pure-Python restatement of GenerateContigs on one rank (src/ContigGeneration.cpp:18-51,110,376-457), statement by statement, with
dict-of-dict matrices and union-find in place of CombBLAS's CC (LACC): component labels never reach the output, only the partition does.
Its input is S as triples in the export order (columns ascending, rows ascending within a column; the value at (r, c) is S(r, c), the
Overlap whose Q read is r) and the read sequences.  Shares nothing with elba_amd/csrc/contig.hip, in the spirit of string_graph_util.py.
Also: a generator of valid random string graphs."""
import numpy as np

from oracle import pyoracle as po

_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def comp(c):
    return _COMP.get(c, "\0")                               # comp(), :327-337


def revcomp(s):
    return "".join(comp(c) for c in s)[::-1]


class BadPrefix(ValueError):
    pass


def _find(parent, x):
    while parent[x] != x:
        parent[x] = parent[parent[x]]
        x = parent[x]
    return x


def generate_contigs(nreads, rows, cols, vals, seqs, base=0):
    """Returns (contigs, chains, read_contig, stats).  rows / cols are ids of S (base + local index); seqs[v] is the read of local index v.
    chains[i] = [(read id, prefix, strand), ...]; read_contig[v] = contig index or -1."""
    # S as a dict-of-dict matrix: S[r][c] = S(r, c)
    S = {}
    for r, c, o in zip(rows, cols, vals):
        S.setdefault(int(r) - base, {})[int(c) - base] = o
    # GetRead2Contigs (:18-52): degrees = row reduction of the bool copy; branches = degrees > 2; A.PruneFull(branches, branches); CC(A)
    degrees = [len(S.get(v, {})) for v in range(nreads)]
    branches = {v for v in range(nreads) if degrees[v] > 2}
    A = {r: {c: 1 for c in row if c not in branches} for r, row in S.items() if r not in branches}
    parent = list(range(nreads))
    for r, row in A.items():
        for c in row:
            a, b = _find(parent, r), _find(parent, c)
            if a != b:
                parent[max(a, b)] = min(a, b)
    assignments = [_find(parent, v) for v in range(nreads)]
    numcontigs = len(set(assignments))
    # GetContigSizes (:110): only components of >= 2 reads are used; GetLocalProcAssignments: every other read gets processor -1
    sizes = {}
    for a in assignments:
        sizes[a] = sizes.get(a, 0) + 1
    proc = [0 if sizes[assignments[v]] >= 2 else -1 for v in range(nreads)]
    # InducedSubgraphs2Procs + Transpose + GetCSC (:376-378): local ids ascending global id; column cur lists rows r with S(cur, r)
    local_contig_read_ids = [v for v in range(nreads) if proc[v] == 0]
    loc = {v: i for i, v in enumerate(local_contig_read_ids)}
    n = len(local_contig_read_ids)
    jc, ir, num = [0], [], []
    for cur in local_contig_read_ids:
        for r in sorted(S.get(cur, {})):
            if r in loc:
                ir.append(loc[r]); num.append(S[cur][r])
        jc.append(len(ir))
    contigs, chains = [], []
    read_contig = [-1] * nreads
    # the walk (:402-457)
    visited = [False] * n
    used_roots = set()
    for v in range(n):
        if jc[v + 1] - jc[v] != 1 or v in used_roots:
            continue
        chain = []
        lastdir = None
        cur = v
        while True:
            visited[cur] = True
            nxt, end = jc[cur], jc[cur + 1]
            while nxt < end and visited[ir[nxt]]:
                nxt += 1
            if nxt >= end:
                break
            o = num[nxt]
            strand = (int(o["direction"]) >> 1) & 1
            chain.append((local_contig_read_ids[cur], int(o["suffixT"]), bool(strand)))
            lastdir = int(o["direction"])
            cur = ir[nxt]
        readlen = len(seqs[local_contig_read_ids[cur]])
        chain.append((local_contig_read_ids[cur], readlen, bool(1 - (lastdir & 1))))
        contig = ""
        for readid, prefix, strand in chain:
            s = seqs[readid]
            if prefix < 0 or prefix > len(s):          # undefined in the reference (std::string(begin, begin + prefix)); an error here
                raise BadPrefix("read %d: prefix %d outside [0, %d]" % (readid + base, prefix, len(s)))
            if strand:
                s = revcomp(s)
            contig += s[:prefix]
        for readid, _, _ in chain:
            read_contig[readid] = len(contigs)
        contigs.append(contig)
        chains.append([(readid + base, prefix, int(strand)) for readid, prefix, strand in chain])
        used_roots.add(cur)
    # counts: used components that emitted nothing are cycles (no read of degree 1)
    used = {assignments[v] for v in range(nreads) if proc[v] == 0}
    stats = dict(nreads=nreads, branches=len(branches), components=numcontigs, used_components=len(used), contigs=len(contigs),
                 cycles=len(used) - len(contigs), contig_reads=sum(len(c) for c in chains), bases=sum(len(c) for c in contigs),
                 longest=max((len(c) for c in contigs), default=0))
    return contigs, chains, read_contig, stats


def export_of(g):
    """(rows, cols, vals) of an Engine.export_string_graph() dict."""
    return g["rows"], g["cols"], g["vals"]


def seqs_of(packed, off, lens):
    """ASCII reads from the 2-bit layout (first base in bits 7-6)."""
    out = []
    for o, L in zip(off, lens):
        o, L = int(o), int(L)
        b = np.asarray(packed[o:o + (L + 3) // 4], dtype=np.uint8)
        codes = np.stack([(b >> 6) & 3, (b >> 4) & 3, (b >> 2) & 3, b & 3], axis=1).reshape(-1)[:L]
        out.append(np.frombuffer(b"ACGT", dtype=np.uint8)[codes].tobytes().decode("ascii"))
    return out


def pack(seqs):
    """(packed, byte_off, lens) of ASCII reads (A, C, G, T)."""
    code = {"A": 0, "C": 1, "G": 2, "T": 3}
    buf, off, lens = bytearray(), [], []
    for s in seqs:
        off.append(len(buf)); lens.append(len(s))
        b = bytearray((len(s) + 3) // 4)
        for i, ch in enumerate(s):
            b[i // 4] |= code[ch] << (6 - 2 * (i % 4))
        buf += b
    buf += bytes(16)
    return np.frombuffer(bytes(buf), dtype=np.uint8).copy(), np.array(off, dtype=np.uint64), np.array(lens, dtype=np.uint32)


def random_reads(rng, n, lo=20, hi=200):
    return ["".join("ACGT"[x] for x in rng.integers(0, 4, int(rng.integers(lo, hi + 1)))) for _ in range(n)]


def edge(rng, lenQ, lenT, direction=None, directionT=None):
    """A valid upper-triangle entry (Q = the row read): a direction pair from all four, 0 <= suffixT <= len(Q), 0 <= suffix <= len(T)."""
    o = np.zeros(1, dtype=po.OVERLAP_DTYPE)[0]
    o["passed"] = 1
    o["direction"] = int(rng.integers(0, 4)) if direction is None else direction
    o["directionT"] = int(rng.integers(0, 4)) if directionT is None else directionT
    o["suffixT"] = int(rng.integers(0, lenQ + 1)); o["suffix"] = int(rng.integers(0, lenT + 1))
    return o


def upper(edges):
    """{(i, j): overlap} with i < j -> (rows, cols, vals) ascending in (row, col), the order elba_set_overlaps wants."""
    keys = sorted(edges)
    rows = np.array([k[0] for k in keys], dtype=np.int64); cols = np.array([k[1] for k in keys], dtype=np.int64)
    vals = np.array([edges[k] for k in keys], dtype=po.OVERLAP_DTYPE) if keys else np.zeros(0, dtype=po.OVERLAP_DTYPE)
    return rows, cols, vals


def random_string_graph(rng, M, lens, n_paths=None, p_extra=0.3):
    """A valid random string graph without triangles (so that the transitive reduction at cutoff 0 keeps every entry): reads laid out on
    random paths and cycles under shuffled ids, plus random extra edges (hubs, branches) that close no triangle."""
    perm = rng.permutation(M)
    edges, adj = {}, [set() for _ in range(M)]

    def add(u, v):
        if u == v or v in adj[u] or adj[u] & adj[v]:          # no multi-edges, no triangles
            return
        i, j = min(u, v), max(u, v)
        edges[(i, j)] = edge(rng, int(lens[i]), int(lens[j]))
        adj[u].add(v); adj[v].add(u)

    cuts = sorted(rng.choice(np.arange(1, M), size=min(M - 1, n_paths or max(1, M // 8)), replace=False).tolist()) if M > 1 else []
    for a, b in zip([0] + cuts, cuts + [M]):
        seg = perm[a:b]
        for x, y in zip(seg[:-1], seg[1:]):
            add(int(x), int(y))
        if len(seg) >= 4 and rng.random() < 0.25:
            add(int(seg[-1]), int(seg[0]))                    # a cycle
    for _ in range(int(p_extra * M)):
        add(int(rng.integers(0, M)), int(rng.integers(0, M)))
    return upper(edges)


def transpose(o):
    """Overlap::Transpose (include/Overlap.hpp:42-69)."""
    t = o.copy()
    for a, b in (("begQ", "begT"), ("endQ", "endT"), ("suffix", "suffixT"), ("direction", "directionT"), ("containedQ", "containedT")):
        t[a], t[b] = o[b], o[a]
    return t


def symmetric(edges):
    """S from {(i, j): S(i, j)} (i < j): both triangles, S(j, i) = Overlap::Transpose(S(i, j)), in the export order (columns ascending,
    rows ascending within a column)."""
    ent = {}
    for (i, j), o in edges.items():
        ent[(i, j)] = o; ent[(j, i)] = transpose(o)
    keys = sorted(ent, key=lambda k: (k[1], k[0]))
    rows = np.array([k[0] for k in keys], dtype=np.int64); cols = np.array([k[1] for k in keys], dtype=np.int64)
    vals = np.array([ent[k] for k in keys], dtype=po.OVERLAP_DTYPE) if keys else np.zeros(0, dtype=po.OVERLAP_DTYPE)
    return rows, cols, vals


def random_packed(rng, n, lo=20, hi=60):
    """n random reads straight into the 2-bit layout (fast for large n): (packed, byte_off, lens)."""
    lens = rng.integers(lo, hi + 1, n).astype(np.uint32)
    nb = (lens.astype(np.int64) + 3) // 4
    off = np.zeros(n, dtype=np.uint64)
    off[1:] = np.cumsum(nb)[:-1].astype(np.uint64)
    packed = rng.integers(0, 256, int(nb.sum()) + 16).astype(np.uint8)
    packed[-16:] = 0
    return packed, off, lens
