"""A pure-Python restatement of contig generation with its two extensions (elba_generate_contigs_ex): path contigs by the reference's walk
(src/ContigGeneration.cpp:402-457), cycles walked from their smallest read towards its smaller neighbour with the closing prefix, single
reads, and the merge by start read.  Dict-based; shares nothing with elba_amd/csrc/contig.hip nor with contig_util.generate_contigs (only
its helpers are imported).  Also: circular and linear genomes cut into reads, with the string-graph edges derived from the layout."""
import numpy as np

import contig_util as cu

CIRCULAR, SINGLETONS = 1, 2
PATH, CIRCLE, SINGLE = 0, 1, 2


def generate_contigs_ex(nreads, rows, cols, vals, seqs, flags=0, read_flags=None, base=0):
    """Returns (contigs, chains, kinds, read_contig, stats).  S as in contig_util.generate_contigs; read_flags[v] != 0 marks a bad or a
    contained read (never a singleton).  A prefix outside [0, len] raises contig_util.BadPrefix whose .pair is the smallest (read, next)."""
    S = {}
    for r, c, o in zip(rows, cols, vals):
        S.setdefault(int(r) - base, {})[int(c) - base] = o          # S[cur][next] = S(cur, next), the entry the walk reads at cur
    branch = {v for v in range(nreads) if len(S.get(v, {})) > 2}
    nb = {v: ([] if v in branch else sorted(c for c in S.get(v, {}) if c not in branch)) for v in range(nreads)}
    found = []                                                  # (start read, kind, [(read, next or None)])
    seen = set()
    # paths: the walk starts at every read with one kept neighbour that no earlier walk ended in, ascending
    for v in range(nreads):
        if len(nb[v]) != 1 or v in seen:
            continue
        steps, prev, cur = [], None, v
        while True:
            seen.add(cur)
            nxt = [w for w in nb[cur] if w != prev]
            if not nxt:
                steps.append((cur, None))
                break
            steps.append((cur, nxt[0]))
            prev, cur = cur, nxt[0]
        found.append((v, PATH, steps))
    # what is left with two kept neighbours lies on cycles
    ncycles = 0
    for s in range(nreads):
        if len(nb[s]) != 2 or s in seen:
            continue
        ncycles += 1
        steps, prev, cur, nxt = [], None, s, min(nb[s])
        while True:
            seen.add(cur)
            steps.append((cur, nxt))
            prev, cur = cur, nxt
            if cur == s:
                break
            nxt = [w for w in nb[cur] if w != prev][0]
        if flags & CIRCULAR:
            found.append((s, CIRCLE, steps))
    isolated = sum(1 for v in range(nreads) if v not in branch and not nb[v])
    if flags & SINGLETONS:
        for v in range(nreads):
            if not nb[v] and len(seqs[v]) > 0 and (read_flags is None or int(read_flags[v]) == 0):
                found.append((v, SINGLE, [(v, None)]))
    found.sort(key=lambda t: t[0])
    contigs, chains, kinds, read_contig, bad = [], [], [], [-1] * nreads, []
    for start, kind, steps in found:
        chain = []
        for i, (cur, nxt) in enumerate(steps):
            if nxt is not None:
                o = S[cur][nxt]
                prefix, strand = int(o["suffixT"]), (int(o["direction"]) >> 1) & 1
                if prefix < 0 or prefix > len(seqs[cur]):
                    bad.append((cur + base, nxt + base))
                    prefix = 0
            elif kind == SINGLE:
                prefix, strand = len(seqs[cur]), 0
            else:
                lastdir = int(S[steps[i - 1][0]][cur]["direction"])
                prefix, strand = len(seqs[cur]), 1 - (lastdir & 1)
            chain.append((cur + base, prefix, strand))
            read_contig[cur] = len(contigs)
        contigs.append("".join((cu.revcomp(seqs[r - base]) if st else seqs[r - base])[:p] for r, p, st in chain))
        chains.append(chain); kinds.append(kind)
    if bad:
        e = cu.BadPrefix("prefix outside the read at (read, next) = %r" % (min(bad),))
        e.pair = min(bad)
        raise e
    npaths = sum(1 for k in kinds if k == PATH)
    stats = dict(nreads=nreads, branches=len(branch), components=len(branch) + isolated + npaths + ncycles, used_components=npaths + ncycles,
                 contigs=len(contigs), cycles=ncycles, contig_reads=sum(len(c) for c in chains), bases=sum(len(c) for c in contigs),
                 longest=max((len(c) for c in contigs), default=0))
    return contigs, chains, kinds, read_contig, stats


def random_genome(rng, n):
    return "".join("ACGT"[x] for x in rng.integers(0, 4, n))


def layout_reads(rng, genome, n, circular, ids):
    """Cuts `genome` into n reads that cover it, each overlapping only its neighbours in the layout (the last one the first, round the
    origin, when circular; n >= 4 then), reverse-complements a random half and gives read i of the layout the id ids[i].
    Returns ({id: sequence}, {(i, j): overlap} with i < j).

    The edges come from the layout alone.  For a step of the walk from x to y, direction = 2 * (x is emitted reverse-complemented) +
    (y is emitted as stored) and the prefix is what x contributes before y begins: walking with the layout, x is reversed iff it was
    stored reverse-complemented and the prefix is the difference of the starts; walking against it everything flips and the prefix is
    the difference of the ends.  The entry at (Q, T) holds the step Q -> T in direction / suffixT and, by Overlap::Transpose, the step
    T -> Q in directionT / suffix.  (Forward reads, Q left of T: direction 1, directionT 2.)"""
    glen = len(genome)
    gaps = 8 + rng.multinomial(glen - 8 * n, np.ones(n) / n)   # start-to-start distances, each >= 8
    p = np.concatenate([[0], np.cumsum(gaps)]).astype(np.int64)  # p[n] = glen: the first read again, one turn on
    if circular:
        off = int(rng.integers(0, glen))
        src = genome + genome + genome
        ov = [int(rng.integers(1, gaps[(i + 1) % n])) for i in range(n)]          # reaches into the next read, not into the one after
        e = [int(p[i + 1]) + ov[i] for i in range(n)]
    else:
        off, src = 0, genome
        ov = [int(rng.integers(1, gaps[i + 1])) for i in range(n - 1)]
        e = [int(p[i + 1]) + ov[i] for i in range(n - 1)] + [glen]
    rc = np.zeros(n, dtype=bool)
    rc[rng.permutation(n)[:n // 2]] = True
    seqs = {}
    for i in range(n):
        s = src[off + int(p[i]):off + e[i]]
        seqs[int(ids[i])] = cu.revcomp(s) if rc[i] else s
    edges = {}
    for i in range(n if circular else n - 1):
        j = (i + 1) % n
        pj, ej = (int(p[i + 1]), e[j] + (glen if j == 0 else 0))                   # the right-hand read in the coordinates of the left one
        fwd = (2 * int(rc[i]) + (1 - int(rc[j])), pj - int(p[i]))                  # the step i -> j, with the layout
        back = (2 * (1 - int(rc[j])) + int(rc[i]), ej - e[i])                      # the step j -> i, against it
        x, y = int(ids[i]), int(ids[j])
        q2t, t2q = (fwd, back) if x < y else (back, fwd)
        o = cu.edge(rng, 1, 1, q2t[0], t2q[0])
        o["suffixT"], o["suffix"] = q2t[1], t2q[1]
        edges[(min(x, y), max(x, y))] = o
    return seqs, edges


def is_rotation(contig, genome):
    """contig is a rotation of the circular genome or of its reverse complement."""
    return len(contig) == len(genome) and (contig in genome + genome or contig in cu.revcomp(genome) * 2)


def genome_graph(rng, parts):
    """parts: [(genome length, reads, circular)].  One graph under a random permutation of all ids.  Returns (seqs list, edges dict,
    [(genome, ids of its reads, circular)])."""
    M = sum(n for _, n, _ in parts)
    perm = rng.permutation(M)
    seqs, edges, info, at = {}, {}, [], 0
    for glen, n, circ in parts:
        g = random_genome(rng, glen)
        ids = perm[at:at + n]; at += n
        s, e = layout_reads(rng, g, n, circ, ids)
        seqs.update(s); edges.update(e)
        info.append((g, sorted(int(x) for x in ids), circ))
    return [seqs[v] for v in range(M)], edges, info
