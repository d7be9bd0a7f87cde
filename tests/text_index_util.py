"""The grammar of elba_set_reads_text (include/elba_amd.h) restated twice on the CPU — a literal loop over bytes and
lines, and a vectorised numpy form built like the device's passes (newline ranks, header flags, closed forms per record) — with a FASTQ
writer and a table of hand cases whose records are written out by hand.  tests/test_text_index_cpu.py holds the two forms against each
other, against fasta.write_fai and against the table; tests/test_gpu_text_ingest.py holds the device against them."""
import numpy as np

from elba_amd.fasta import FAI_DTYPE

# kinds of a violation (the low three bits of the library's error word; on one offset the smaller kind is reported)
CR, FIRST, SHAPE, FQ_LINES, FQ_AT, FQ_PLUS, FQ_QUAL, LONG = range(8)
KIND_NAMES = ("CR", "FIRST", "SHAPE", "FQ_LINES", "FQ_AT", "FQ_PLUS", "FQ_QUAL", "LONG")
MAX_LEN = 0x7FFFFFF0
NAME_ENDS = (0x20, 0x09, 0x0B, 0x0C)      # space, tab, VT, FF ('\n' ends the line, '\r' is rejected): where bytes.split() cuts


class TextError(Exception):
    def __init__(self, kind, offset):
        Exception.__init__(self, "%s at file offset %d" % (KIND_NAMES[kind], offset))
        self.kind, self.offset = kind, offset


def _format(data, fmt, file_off):
    if fmt != "auto":
        return fmt
    if len(data) == 0 or data[0] == 0x3E:
        return "fasta"
    if data[0] == 0x40:
        return "fastq"
    raise TextError(CR if data[0] == 0x0D else FIRST, file_off)


def _result(fmt, nlines, recs, name_pos, name_len):
    return dict(format=fmt, lines=nlines, recs=np.array(recs, dtype=FAI_DTYPE).reshape(-1), name_pos=np.array(name_pos, dtype=np.uint64).reshape(-1),
                name_len=np.array(name_len, dtype=np.uint32).reshape(-1))


def _raise_smallest(errs):
    if errs:
        off, kind = min(errs)
        raise TextError(kind, off)


# ---- form 1: a literal loop --------------------------------------------------------------------------------------------------------------
def index_loop(data, fmt="auto", file_off=0):
    data = bytes(data)
    n = len(data)
    fmt = _format(data, fmt, file_off)
    errs = []
    lines, s = [], 0      # (start, end): the line's bytes without its newline
    for i in range(n):
        if data[i] == 0x0D:
            errs.append((file_off + i, CR))
        if data[i] == 0x0A:
            lines.append((s, i)); s = i + 1
    if n and data[-1] != 0x0A:
        lines.append((s, n))

    def name_of(a, b):
        p = min(a + 1, b)
        q = p
        while q < b and data[q] not in NAME_ENDS:
            q += 1
        return file_off + p, q - p

    recs, name_pos, name_len = [], [], []
    if fmt == "fasta":
        groups = []      # [header line, sequence lines]
        for li, (a, b) in enumerate(lines):
            if b > a and data[a] == 0x3E:
                groups.append([li, []])
            elif not groups:
                if li == 0:
                    errs.append((file_off, FIRST))
            else:
                groups[-1][1].append(li)
        for h, seq in groups:
            ha, hb = lines[h]
            pos = min(hb + 1, n)
            ll = [lines[j][1] - lines[j][0] for j in seq]
            length, bases = sum(ll), (ll[0] if ll else 0)
            for t, j in enumerate(seq):      # the local rule: l <= bases and (l == bases or the successor is empty or it is the last line)
                ok = ll[t] <= bases and (ll[t] == bases or t + 1 == len(seq) or ll[t + 1] == 0)
                if not ok:
                    errs.append((file_off + lines[j][0], SHAPE))
            if length >= MAX_LEN:
                errs.append((file_off + ha, LONG))
            recs.append((length, file_off + pos, 1 if length == 0 else bases))
            p, l = name_of(ha, hb)
            name_pos.append(p); name_len.append(l)
    else:
        nrec = len(lines) // 4
        if len(lines) % 4:
            errs.append((file_off + lines[4 * nrec][0], FQ_LINES))
        for r in range(nrec):
            (a0, b0), (a1, b1), (a2, b2), (a3, b3) = lines[4 * r:4 * r + 4]
            if not (b0 > a0 and data[a0] == 0x40):
                errs.append((file_off + a0, FQ_AT))
            if not (b2 > a2 and data[a2] == 0x2B):
                errs.append((file_off + a2, FQ_PLUS))
            if b3 - a3 != b1 - a1:
                errs.append((file_off + a0, FQ_QUAL))
            if b1 - a1 >= MAX_LEN:
                errs.append((file_off + a0, LONG))
            recs.append((b1 - a1, file_off + a1, max(b1 - a1, 1)))
            p, l = name_of(a0, b0)
            name_pos.append(p); name_len.append(l)
    _raise_smallest(errs)
    return _result(fmt, len(lines), recs, name_pos, name_len)


def shape_holds(ll):
    """the line lengths read bases, .., bases, t, 0, .., 0 with 0 <= t <= bases — the definition the local rule is equivalent to"""
    if not ll:
        return True
    bases, k = ll[0], 0
    while k < len(ll) and ll[k] == bases:
        k += 1
    rest = ll[k:]
    return not rest or (rest[0] <= bases and all(x == 0 for x in rest[1:]))


def local_rule_holds(ll):
    bases = ll[0] if ll else 0
    return all(ll[t] <= bases and (ll[t] == bases or t + 1 == len(ll) or ll[t + 1] == 0) for t in range(len(ll)))


# ---- form 2: vectorised, shaped like the device's passes ---------------------------------------------------------------------------------
def index_numpy(data, fmt="auto", file_off=0):
    data = bytes(data)
    a = np.frombuffer(data, dtype=np.uint8)
    n = a.size
    fmt = _format(data, fmt, file_off)
    errs = []
    cr = np.flatnonzero(a == 0x0D)
    if cr.size:
        errs.append((file_off + int(cr[0]), CR))
    nlpos = np.flatnonzero(a == 0x0A).astype(np.int64)
    final_nl = bool(n and a[-1] == 0x0A)
    nlines = int(nlpos.size) + (1 if n and not final_nl else 0)
    ls = np.zeros(nlines + 1, dtype=np.int64)      # line i is [ls[i], ls[i + 1] - 1)
    ls[1:nlpos.size + 1] = nlpos + 1
    if n and not final_nl:
        ls[nlines] = n + 1
    L = ls[1:] - 1 - ls[:-1]
    first = a[ls[:nlines]] if nlines else np.zeros(0, np.uint8)      # (an empty line's "first byte" is its newline)
    wspos = np.flatnonzero(np.isin(a, NAME_ENDS)).astype(np.int64)

    def names_of(h):
        e = np.minimum(ls[h + 1] - 1, n)
        p = np.minimum(ls[h] + 1, e)
        k = np.searchsorted(wspos, p)
        cand = wspos[np.minimum(k, max(wspos.size - 1, 0))] if wspos.size else np.full(p.shape, n, np.int64)
        q = np.where((k < wspos.size) & (cand < e), cand, e)
        return (file_off + p).astype(np.uint64), (q - p).astype(np.uint32)

    if fmt == "fasta":
        hdr = first == 0x3E
        rol = np.cumsum(hdr) - hdr      # headers before line i
        rec_line = np.append(np.flatnonzero(hdr), nlines).astype(np.int64)
        nrec = rec_line.size - 1
        if nlines and not hdr[0]:
            errs.append((file_off, FIRST))
        i = np.flatnonzero(~hdr & (rol > 0))
        if i.size:
            h, nxt = rec_line[rol[i] - 1], rec_line[rol[i]]
            bases = L[h + 1]
            succ = L[np.minimum(i + 1, nlines - 1)]
            bad = ~((L[i] <= bases) & ((L[i] == bases) | (i + 1 == nxt) | (succ == 0)))
            if bad.any():
                errs.append((file_off + int(ls[i[bad][0]]), SHAPE))
        h, nxt = rec_line[:-1], rec_line[1:]
        pos = np.minimum(ls[h + 1], n) if nrec else np.zeros(0, np.int64)
        end = np.minimum(ls[nxt], n) if nrec else np.zeros(0, np.int64)
        nseq = nxt - h - 1
        length = end - pos - (nseq - ((nxt == nlines) & (not final_nl) & (nseq > 0)))
        bases = np.where(nseq > 0, L[np.minimum(h + 1, max(nlines - 1, 0))], 0) if nrec else np.zeros(0, np.int64)
        bases = np.where(length == 0, 1, bases)
        hl = h
    else:
        nrec = nlines // 4
        if nlines % 4:
            errs.append((file_off + int(ls[4 * nrec]), FQ_LINES))
        hl = 4 * np.arange(nrec, dtype=np.int64)
        length, pos = L[hl + 1], ls[hl + 1]
        for bad, at, kind in ((first[hl] != 0x40, ls[hl], FQ_AT), (first[hl + 2] != 0x2B, ls[hl + 2], FQ_PLUS), (L[hl + 3] != length, ls[hl], FQ_QUAL)):
            if bad.any():
                errs.append((file_off + int(at[bad][0]), kind))
        bases = np.maximum(length, 1)
    if nrec and (length >= MAX_LEN).any():
        errs.append((file_off + int(ls[hl[length >= MAX_LEN][0]]), LONG))
    _raise_smallest(errs)
    recs = np.zeros(nrec, dtype=FAI_DTYPE)
    recs["len"], recs["pos"], recs["bases"] = length, pos + file_off, bases
    name_pos, name_len = names_of(hl) if nrec else (np.zeros(0, np.uint64), np.zeros(0, np.uint32))
    return dict(format=fmt, lines=nlines, recs=recs, name_pos=name_pos, name_len=name_len)


def same_index(x, y):
    return (x["format"] == y["format"] and x["lines"] == y["lines"] and x["recs"].shape == y["recs"].shape and all((x["recs"][f] == y["recs"][f]).all() for f in ("len", "pos", "bases"))
            and (x["name_pos"] == y["name_pos"]).all() and (x["name_len"] == y["name_len"]).all())


def error_of(fn, data, fmt="auto", file_off=0):
    """(kind, offset) of the rejection, None when the text is accepted"""
    try:
        fn(data, fmt, file_off)
    except TextError as e:
        return e.kind, e.offset
    return None


def names_of(data, idx, file_off=0):
    data = bytes(data)
    return [data[int(p) - file_off:int(p) - file_off + int(l)].decode() for p, l in zip(idx["name_pos"], idx["name_len"])]


def sequences_of(data, idx, file_off=0):
    """the bases of every record, placed as the reference places them: base b at pos + b + b / bases"""
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    out = []
    for r in idx["recs"]:
        b = np.arange(int(r["len"]), dtype=np.int64)
        out.append(a[int(r["pos"]) - file_off + b + b // int(r["bases"])].tobytes())
    return out


# ---- writers ------------------------------------------------------------------------------------------------------------------------------
def fastq_bytes(seqs, names=None, quals=None, final_newline=True):
    """four lines per read; quals[i] (default 'I' * len) may begin with '@', '+' or '>'"""
    out = bytearray()
    for i, s in enumerate(seqs):
        name = names[i] if names is not None else b"read%d some description" % i
        q = quals[i] if quals is not None else b"I" * len(s)
        out += b"@" + name + b"\n" + s + b"\n+\n" + q + b"\n"
    if not final_newline and out:
        del out[-1]
    return bytes(out)


def fasta_bytes(seqs, width=0, names=None, final_newline=True):
    out = bytearray()
    for i, s in enumerate(seqs):
        out += b">" + (names[i] if names is not None else b"read%d some description" % i) + b"\n"
        if width <= 0 or not s:
            out += s + b"\n"
        else:
            for a in range(0, len(s), width):
                out += s[a:a + width] + b"\n"
    if not final_newline and out:
        del out[-1]
    return bytes(out)


def random_seqs(rng, lengths, alphabet=b"ACGTacgtNnXR"):
    al = np.frombuffer(alphabet, dtype=np.uint8)
    return [al[rng.integers(0, len(al) if i % 3 == 0 else min(8, len(al)), int(n))].tobytes() for i, n in enumerate(lengths)]


# ---- hand cases: (label, text, fmt, [(len, pos, bases)], [names]) — every number written by hand ----------------------------------------
GOOD_CASES = [
    ("empty chunk", b"", "auto", [], []),
    ("header without newline", b">r", "auto", [(0, 2, 1)], ["r"]),
    ("lone >", b">", "auto", [(0, 1, 1)], [""]),
    ("one read", b">r1\nACGT\n", "auto", [(4, 4, 4)], ["r1"]),
    ("no final newline", b">r1\nACGT", "auto", [(4, 4, 4)], ["r1"]),
    ("wrapped", b">r1 d\nACGT\nACGT\nAC\n>r2\nGG\n", "auto", [(10, 6, 4), (2, 23, 2)], ["r1", "r2"]),
    ("wrapped, exact multiple, no final newline", b">a\nAC\nGT", "auto", [(4, 3, 2)], ["a"]),
    ("header as last line", b">a\nAC\n>b\n", "auto", [(2, 3, 2), (0, 9, 1)], ["a", "b"]),
    ("header as last line, no newline", b">a\nAC\n>b", "auto", [(2, 3, 2), (0, 8, 1)], ["a", "b"]),
    ("empty reads first, last and adjacent", b">a\n\n>b\n>c\nA\n>d\n\n>e\n", "auto", [(0, 3, 1), (0, 7, 1), (1, 10, 1), (0, 15, 1), (0, 19, 1)], ["a", "b", "c", "d", "e"]),
    ("trailing blank lines", b">a\nACG\nA\n\n\n>b\nT\n\n", "auto", [(4, 3, 3), (1, 14, 1)], ["a", "b"]),
    ("names ended by space, tab and line end", b">n1 x y\nA\n>n2\tz\nC\n>n3\nG\n", "auto", [(1, 8, 1), (1, 16, 1), (1, 22, 1)], ["n1", "n2", "n3"]),
    ("empty name before a space", b"> x\nA\n", "auto", [(1, 4, 1)], [""]),
    ("> inside a header and inside a sequence line", b">a>b c\nAC>T\nA>\n", "auto", [(6, 7, 4)], ["a>b"]),
    ("fastq", b"@q1 d\nACGT\n+\nIIII\n", "auto", [(4, 6, 4)], ["q1"]),
    ("fastq, no final newline", b"@q1\nACGT\n+q1\nIIII", "auto", [(4, 4, 4)], ["q1"]),
    ("fastq, quality lines that begin with @ + >", b"@a\nAC\n+\n@I\n@b\nGT\n+\n+I\n@c\nTT\n+\n>I\n", "auto", [(2, 3, 2), (2, 14, 2), (2, 25, 2)], ["a", "b", "c"]),
    ("fastq, empty reads first and last", b"@a\n\n+\n\n@b\nA\n+\nI\n@c\n\n+\n\n", "auto", [(0, 3, 1), (1, 10, 1), (0, 19, 1)], ["a", "b", "c"]),
    ("explicit fastq, empty", b"", "fastq", [], []),
]

# (label, text, fmt, kind, offset)
BAD_CASES = [
    ("a CR", b">a\nAC\r\nGT\n", "auto", CR, 5),
    ("a CR in a header", b">a\r\nAC\n", "auto", CR, 2),
    ("first byte neither > nor @", b"ACGT\n>a\nA\n", "auto", FIRST, 0),
    ("first byte not > in explicit FASTA", b"@a\nA\n+\nI\n", "fasta", FIRST, 0),
    ("first byte a CR", b"\r>a\nA\n", "auto", CR, 0),
    ("short middle line", b">a\nACGT\nAC\nACGT\n", "auto", SHAPE, 8),
    ("last line longer than bases", b">a\nAC\nACG\n", "auto", SHAPE, 6),
    ("blank middle line", b">a\nAC\n\nAC\n", "auto", SHAPE, 6),
    ("blank first line", b">a\n\nAC\n", "auto", SHAPE, 4),
    ("second record breaks the shape", b">a\nAC\nA\n>b\nA\nAC\n", "auto", SHAPE, 13),
    ("fastq 4n+1 lines", b"@a\nA\n+\nI\n@b\n", "auto", FQ_LINES, 9),
    ("fastq 4n+2 lines", b"@a\nA\n+\nI\n@b\nA\n", "auto", FQ_LINES, 9),
    ("fastq 4n+3 lines", b"@a\nA\n+\nI\n@b\nA\n+\n", "auto", FQ_LINES, 9),
    ("fastq 4n+3 lines, no final newline", b"@a\nA\n+\nI\n@b\nA\n+", "auto", FQ_LINES, 9),
    ("missing +", b"@a\nA\n-\nI\n", "auto", FQ_PLUS, 5),
    ("missing @", b"@a\nA\n+\nI\nb\nA\n+\nI\n", "auto", FQ_AT, 9),
    ("missing @ in explicit FASTQ", b">a\nA\n+\nI\n", "fastq", FQ_AT, 0),
    ("quality one byte short", b"@a\nAC\n+\nI\n", "auto", FQ_QUAL, 0),
    ("quality one byte long", b"@a\nAC\n+\nIII\n@b\nA\n+\nI\n", "auto", FQ_QUAL, 0),
    ("quality one byte long, second record", b"@a\nA\n+\nI\n@b\nA\n+\nII\n", "auto", FQ_QUAL, 9),
    ("wrapped fastq", b"@a\nAC\nGT\n+\nII\nII\n", "auto", FQ_QUAL, 0),      # (its fourth line, the "+", has not the length of its second)
    ("an empty last quality line cannot lose its newline", b"@a\nA\n+\nI\n@b\n\n+\n", "auto", FQ_LINES, 9),
    ("two violations, the earlier one named", b">a\nAC\n\nAC\n>b\nA\r\n", "auto", SHAPE, 6),
    ("a CR before a shape violation", b">a\r\nAC\n\nAC\n", "auto", CR, 2),
]


# ---- the device against the restatement (the -m gpu files share these) -----------------------------------------------------------------------
FMT = {"fasta": 1, "fastq": 2}


def device_exported(e, n, packed_bytes):
    recs, npos, nlen = e.export_read_index_raw()
    packed, off, ln = e.export_reads(n, packed_bytes)
    return recs, npos, nlen, packed, off, ln


def same_export(a, b):
    return all(x.shape == y.shape and (x == y).all() for x, y in zip(a, b))


def device_check(e, data, fmt="auto", file_off=0, gid=0, want=None, loop=False):
    """one call against the restatement (the vectorised form; with loop also the literal one) and the oracle's encoder"""
    from oracle import pyoracle as po
    data = bytes(data)
    want = want or index_numpy(data, fmt, file_off)
    if loop:
        assert same_index(index_loop(data, fmt, file_off), want)
    st = e.set_reads_text(data, file_off, fmt, gid)
    n = len(want["recs"])
    assert st["nreads"] == n and st["lines"] == want["lines"] and st["format"] == FMT[want["format"]] and st["chunk_bytes"] == len(data)
    recs, npos, nlen = e.export_read_index_raw()
    for f in ("len", "pos", "bases"):
        bad = np.flatnonzero(recs[f] != want["recs"][f])
        assert bad.size == 0, (f, int(bad[0]), int(recs[f][bad[0]]), int(want["recs"][f][bad[0]]))
    assert (npos == want["name_pos"]).all() and (nlen == want["name_len"]).all()
    seqs = sequences_of(data, want, file_off)
    wp, woff, wlen = po.pack_reads(seqs)
    assert st["bases"] == int(wlen.sum()) and st["packed_bytes"] == int(((wlen.astype(np.int64) + 3) // 4).sum())
    got, goff, glen = e.export_reads(n, st["packed_bytes"])
    assert (goff == woff).all() and (glen == wlen).all()
    assert (got[:st["packed_bytes"]] == wp[:st["packed_bytes"]]).all() and not got[st["packed_bytes"]:].any()
    names, recs2 = e.export_read_index()
    assert names == names_of(data, want, file_off) and (recs2 == recs).all()
    return st, seqs


def device_rejected(e, data, fmt="auto", file_off=0, loop=True):
    """(kind, offset) the library names, checked against both forms of the restatement (loop=False: a text too long for the literal
    form, which the CPU tests hold against the vectorised one at a small size), and the record of the message"""
    import re

    import pytest

    import elba_amd
    with pytest.raises(elba_amd.ElbaError) as x:
        e.set_reads_text(bytes(data), file_off, fmt)
    assert x.value.status == 1, x.value
    m = re.search(r"\(kind (\d+)\) in record (-?\d+) at file offset (\d+)", str(x.value))
    assert m, str(x.value)
    got = (int(m.group(1)), int(m.group(3)))
    assert got == error_of(index_numpy, data, fmt, file_off)
    if loop:
        assert got == error_of(index_loop, data, fmt, file_off)
    return got, int(m.group(2))
