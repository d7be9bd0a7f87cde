"""Text formats of the reference around the path — host-side, for interop with the reference's own tools:

* SharedSeeds as the reference prints it: operator<< `{(q0,t0),(q1,t1),n}` (include/SharedSeeds.hpp:75-88; min(numshared, 2) seeds) and
  IOHandlerBrief `numstored<TAB>numshared` (:66-73) — the value column of B.mtx (ELBALogger::log_seed_matrix, src/ELBALogger.cpp:22-35,
  CombBLAS ParallelWriteMM with one-based indices).
* the `row col q0 t0 q1 t1` dump that the reference's test.py reads (test.py:42-52: two header lines, zero-based read indices), and
  test.py's check itself (:53-65): every stored seed must be the same k-mer in both reads, forward or reverse complement.
* Overlap as the reference prints it (include/Overlap.hpp:78-83) and the PAF lines of parallel_write_paf (src/main.cpp:514-551),
  including its `maplen` expression as written there (`end_T - end_T`, i.e. max(endQ - begQ, 0)).

CombBLAS's ParallelWriteMM itself is not in the reference tree (un-vendored): its header line is restated from the MatrixMarket
convention (`%%MatrixMarket matrix coordinate real general`, then `nrows ncols nnz`), entries column by column as the DCSC stores them.
"""
import numpy as np

_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def seed_str(v):
    """SharedSeeds operator<< (include/SharedSeeds.hpp:75-88)."""
    n = int(v["numshared"])
    stored = min(2, n)
    parts = []
    if stored >= 1:
        parts.append("(%d,%d)," % (int(v["q0"]), int(v["t0"])))
    if stored >= 2:
        parts.append("(%d,%d)," % (int(v["q1"]), int(v["t1"])))
    return "{" + "".join(parts) + "%d}" % n


def seed_brief_str(v):
    """SharedSeeds::IOHandlerBrief (include/SharedSeeds.hpp:66-73)."""
    n = int(v["numshared"])
    return "%d\t%d" % (min(2, n), n)


def write_seed_matrix_mm(path, dcsc, nrows, handler=seed_str):
    """B.mtx as ELBALogger::log_seed_matrix writes it (one-based indices; entries in DCSC order: column by column, rows ascending)."""
    with open(path, "w") as f:
        f.write("%%MatrixMarket matrix coordinate real general\n")
        f.write("%d %d %d\n" % (nrows, nrows, dcsc["nnz"]))
        for c in range(dcsc["nzc"]):
            col = int(dcsc["jc"][c]) + 1
            for e in range(int(dcsc["cp"][c]), int(dcsc["cp"][c + 1])):
                f.write("%d\t%d\t%s\n" % (int(dcsc["ir"][e]) + 1, col, handler(dcsc["numx"][e])))


def write_testpy_dump(path, csr):
    """The file test.py opens as B.mtx (test.py:42-52): two header lines, then `row col q0 t0 q1 t1`, zero-based."""
    rows = np.repeat(np.arange(csr["M"]), np.diff(csr["rowptr"]))
    with open(path, "w") as f:
        f.write("%%MatrixMarket matrix coordinate integer general\n%d %d %d\n" % (csr["M"], csr["M"], csr["Y"]))
        for e in range(csr["Y"]):
            v = csr["val"][e]
            f.write("%d %d %d %d %d %d\n" % (rows[e], int(csr["col"][e]), int(v["q0"]), int(v["t0"]), int(v["q1"]), int(v["t1"])))


def check_seed_dump(path, seqs, k):
    """test.py:53-67 — returns (correct, incorrect)."""
    correct = incorrect = 0
    with open(path) as f:
        next(f); next(f)
        for line in f:
            t = tuple(int(v) for v in line.split())
            iq, it = t[0], t[1]
            if iq == it:
                continue
            sq, st = seqs[iq], seqs[it]
            for bq, bt in ((t[2], t[3]), (t[4], t[5])):
                a, b = sq[bq:bq + k], st[bt:bt + k]
                if a != b and a != b.translate(_COMP)[::-1]:
                    incorrect += 1
                else:
                    correct += 1
    return correct, incorrect


def overlap_str(o, lenQ, lenT):
    """Overlap operator<< (include/Overlap.hpp:78-83)."""
    return "%d\t%d\t%d\t%s\t%d\t%d\t%d\t%d\t%d\t%d" % (lenQ, int(o["begQ"]), int(o["endQ"]), "-" if o["rc"] else "+", lenT, int(o["begT"]), int(o["endT"]),
                                                     int(o["score"]), int(o["direction"]), int(o["suffix"]))


def paf_line(o, nameQ, nameT, lenQ, lenT):
    """One line of parallel_write_paf (src/main.cpp:536-540)."""
    maplen = max(int(o["endQ"]) - int(o["begQ"]), int(o["endT"]) - int(o["endT"]))      # as written in the reference (:536)
    return "%s\t%d\t%d\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t255\t%d" % (nameQ, lenQ, int(o["begQ"]), int(o["endQ"]), "-" if o["rc"] else "+", nameT, lenT,
                                                                 int(o["begT"]), int(o["endT"]), int(o["score"]), maplen, int(o["passed"]))


def write_paf(path, overlaps, names, lens, dcsc_order=False):
    """dcsc_order: walk the triples as parallel_write_paf walks the local DCSC (columns ascending, rows ascending within a column)
    instead of in the order given."""
    idx = range(overlaps["n"])
    if dcsc_order:
        idx = np.lexsort((overlaps["rows"], overlaps["cols"])).tolist()
    with open(path, "w") as f:
        for a in idx:
            i, j = int(overlaps["rows"][a]), int(overlaps["cols"][a])
            f.write(paf_line(overlaps["vals"][a], names[i], names[j], int(lens[i]), int(lens[j])) + "\n")


def contig_components(comp_of_read, chain_off, chain_read, id_base=0):
    """One component id per contig from Engine.graph_components()["comp_of_read"] and the chains of Engine.export_contigs(): a contig's
    component is that of its first chain read (chain_read holds the ids the graph exports show: read + id_base)."""
    n = len(chain_off) - 1
    return np.array([int(comp_of_read[int(chain_read[int(chain_off[i])]) - int(id_base)]) for i in range(n)], dtype=np.int64)


def write_contigs_fasta(path, seqs, first=0, kinds=None, components=None):
    """<prefix>.contigs.fa as parallel_write_contigs writes it (src/main.cpp:496-499): `>contig<i>` then the sequence, i counted from `first`
    (the rank's offset from MPI_Exscan; 0 on one rank).  With `kinds` (one per contig, Engine.export_contigs()["kinds"]) the header of a
    circular contig (kind 1) is `>contig<i> circular`; every other line is the same.  With `components` (one component id per contig,
    contig_components) the header also ends in ` component=<id>`; without it every byte is as before."""
    if kinds is not None and len(kinds) != len(seqs):
        raise ValueError("write_contigs_fasta: one kind per contig")
    if components is not None and len(components) != len(seqs):
        raise ValueError("write_contigs_fasta: one component per contig")
    with open(path, "wb") as f:
        for i, s in enumerate(seqs):
            f.write(b">contig%d%s%s\n" % (i + first, b" circular" if kinds is not None and int(kinds[i]) == 1 else b"",
                                         b" component=%d" % int(components[i]) if components is not None else b""))
            f.write(s.encode("ascii") if isinstance(s, str) else bytes(s))
            f.write(b"\n")


def placement_interval(p, length, contig_len, circular):
    """(query begin, query end, target begin, target end) of one placed record of Engine.place_reads(): the credited part of the read in
    FORWARD read coordinates and where it lies on the contig.  On a path or single-read contig the target interval is [max(start, 0),
    min(start + len, L)), empty (begin = end, at the nearer contig end) for a read flagged outside.  On a circular contig it is min(len, L)
    bases from start mod L, and the end of a wrapped read runs past L by the bases that wrap."""
    start, l, L = int(p["start"]), int(length), int(contig_len)
    if circular:
        cred = min(l, L)
        tb = start % L if L > 0 else 0
        te, ob, oe = tb + cred, 0, cred
    else:
        tb = min(max(start, 0), L)
        te = max(tb, min(start + l, L))
        ob, oe = min(max(tb - start, 0), l), min(max(te - start, 0), l)
    return (l - oe, l - ob, tb, te) if int(p["strand"]) else (ob, oe, tb, te)


def write_placements_paf(path, placements, names, lens, contig_lens, kinds=None):
    """A reads-to-contigs PAF from Engine.place_reads() (its dict, or its "reads" array): one line per placed read (chain or anchored), by
    ascending read — name, length, the credited interval in forward read coordinates, strand, `contig<i>`, its length, the target interval
    (placement_interval), then in the style of paf_line the anchor pair's score (0 for chain reads), the block length (target end - begin)
    and 255.  `kinds` (Engine.export_contigs()["kinds"]) says which contigs are circular.  Without it none may be: the records do not
    carry their contig's kind, so a record with the wrapped flag raises instead of being written as if it lay on a path."""
    reads = placements["reads"] if isinstance(placements, dict) else placements
    if not (len(reads) == len(names) == len(lens)):
        raise ValueError("write_placements_paf: one record, one name and one length per read")
    if kinds is not None and len(kinds) != len(contig_lens):
        raise ValueError("write_placements_paf: one kind per contig")
    with open(path, "w") as f:
        for r, p in enumerate(reads):
            if not int(p["kind"]):
                continue
            k = int(p["contig"])
            if not 0 <= k < len(contig_lens):
                raise ValueError("write_placements_paf: read %d names contig %d of %d" % (r, k, len(contig_lens)))
            if kinds is None and int(p["flags"]) & 4:
                raise ValueError("write_placements_paf: read %d is wrapped, so contig %d is circular: give the contigs' kinds" % (r, k))
            qb, qe, tb, te = placement_interval(p, lens[r], contig_lens[k], kinds is not None and int(kinds[k]) == 1)
            f.write("%s\t%d\t%d\t%d\t%s\tcontig%d\t%d\t%d\t%d\t%d\t%d\t255\n" % (names[r], int(lens[r]), qb, qe, "-" if int(p["strand"]) else "+", k, int(contig_lens[k]),
                                                                                    tb, te, int(p["score"]), te - tb))


def write_gfa(path, seqs, kinds, links, chains=None, depth=None, component=None):
    """The assembly graph as GFA 1: `H\tVN:Z:1.0`, one `S\tcontig<i>\t<seq>\tLN:i:<len>` per contig (the names of write_contigs_fasta;
    with `chains`, the chain_off of Engine.export_contigs() or one chain per contig, also `\tRC:i:<reads>`), and one
    `L\tcontig<a>\t+|-\tcontig<b>\t+|-\t<overlap>M` per record of Engine.assembly_links(), in their order, the closure records of circular
    contigs (a link from the contig's end to its own start, 0M) included.  `kinds` is checked against the closures: one per circular contig.
    With `depth`, the credited_bases of Engine.place_reads() (one per contig), every S line also ends in `\tDP:f:<credited bases / length>`
    with two decimals (0.00 for a contig of no bases); without it every byte is as before.  With `component`, one component id per contig
    (contig_components over Engine.graph_components()), every S line ends in `\tcc:i:<id>`; without it every byte is as before."""
    n = len(seqs)
    if component is not None and len(component) != n:
        raise ValueError("write_gfa: one component per contig")
    if kinds is not None and len(kinds) != n:
        raise ValueError("write_gfa: one kind per contig")
    if chains is not None and len(chains) not in (n, n + 1):
        raise ValueError("write_gfa: chains is chain_off (n + 1 offsets) or one chain per contig")
    if depth is not None and len(depth) != n:
        raise ValueError("write_gfa: one depth (credited bases) per contig")
    closed = sorted(int(r["from"]) for r in links if int(r["flags"]) & 1)
    if kinds is not None and closed != [i for i in range(n) if int(kinds[i]) == 1]:
        raise ValueError("write_gfa: the closure records are not those of the circular contigs")
    with open(path, "wb") as f:
        f.write(b"H\tVN:Z:1.0\n")
        for i, s in enumerate(seqs):
            b = s.encode("ascii") if isinstance(s, str) else bytes(s)
            f.write(b"S\tcontig%d\t%s\tLN:i:%d" % (i, b, len(b)))
            if chains is not None:
                f.write(b"\tRC:i:%d" % (int(chains[i + 1]) - int(chains[i]) if len(chains) == n + 1 else len(chains[i])))
            if depth is not None:
                f.write(b"\tDP:f:%.2f" % (int(depth[i]) / len(b) if len(b) else 0.0))
            if component is not None:
                f.write(b"\tcc:i:%d" % int(component[i]))
            f.write(b"\n")
        for r in links:
            if int(r["from"]) >= n or int(r["to"]) >= n:
                raise ValueError("write_gfa: a link names contig %d of %d" % (max(int(r["from"]), int(r["to"])), n))
            f.write(b"L\tcontig%d\t%s\tcontig%d\t%s\t%dM\n" % (int(r["from"]), b"-" if int(r["from_rev"]) else b"+", int(r["to"]), b"-" if int(r["to_rev"]) else b"+",
                                                                int(r["overlap"])))
