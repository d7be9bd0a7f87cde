"""A numpy restatement of elba_trim_reads (trim.hip): the pieces of every read from pileup_util's intervals and runs, the packed source
unpacked to one base per element, sliced, and packed again with zero padding bits.  Shares nothing with elba_amd/csrc/trim.hip.  Also: a
brute-force version on ASCII strings (the CPU tests hold the two equal) and a copy of test_gpu_pileup.py's planted-chimera generator."""
import numpy as np

import contig_util as cu
import pileup_util as pu

STATS = ("nreads_in", "pieces", "reads_dropped", "reads_split", "reads_unchanged", "bases_in", "bases_out", "packed_bytes", "longest")

# test_gpu_pileup.py's settings for the planted chimeras (see the comment above CHIM there)
CHIM = dict(mode=1, margin=50, min_depth=2, min_run=300, trim_len=2500)
CHIM_ALIGN = dict(mat=1, mis=-3, gap=-3, dropoff=15)
CLEAN_SPLIT_ALLOWED = 2


def pieces_of(lens, p, depth, off, mode, min_len, min_depth, min_run):
    """(src_read, src_beg, src_end) in (read, beg) order from pileup_util.pileup's outputs: mode 0 the trimmed interval, mode 1 the long runs."""
    src, beg, end = [], [], []
    for v in range(len(lens)):
        if mode == 0:
            iv = [(int(p["trim_beg"][v]), int(p["trim_end"][v]))] if p["trim_beg"][v] >= 0 else []
        else:
            s, e = pu._runs(depth[off[v]:off[v + 1]], min_depth)
            iv = [(int(a), int(b)) for a, b in zip(s, e) if b - a >= min_run]
        for a, b in iv:
            if b - a >= min_len:
                src.append(v); beg.append(a); end.append(b)
    return np.array(src, np.int64), np.array(beg, np.int32), np.array(end, np.int32)


def unpack_bases(packed):
    """One 2-bit code per element: base i of the buffer is bits 7-6, 5-4, 3-2, 1-0 of byte i // 4 (src/DnaSeq.cpp:17)."""
    b = np.asarray(packed, dtype=np.uint8)
    return np.stack([(b >> 6) & 3, (b >> 4) & 3, (b >> 2) & 3, b & 3], axis=1).reshape(-1)


def cut(packed, byte_off, src, beg, end):
    """The pieces in DnaBuffer layout: (packed with 16 guard bytes, byte_off u64, len u32)."""
    ln = (end.astype(np.int64) - beg).astype(np.int64)
    nb = (ln + 3) // 4
    boff = np.concatenate([[0], np.cumsum(nb)]).astype(np.int64)
    total = int(boff[-1])
    out = np.zeros(4 * total, dtype=np.uint8)
    if len(src):
        bases = unpack_bases(packed)
        first = 4 * np.asarray(byte_off, dtype=np.int64)[src] + beg                  # the piece's first base in the source buffer
        within = np.arange(int(ln.sum()), dtype=np.int64) - np.repeat(np.cumsum(ln) - ln, ln)
        out[np.repeat(4 * boff[:-1], ln) + within] = bases[np.repeat(first, ln) + within]
    q = out.reshape(-1, 4)
    by = ((q[:, 0] << 6) | (q[:, 1] << 4) | (q[:, 2] << 2) | q[:, 3]).astype(np.uint8)
    return np.concatenate([by, np.zeros(16, np.uint8)]), boff[:-1].astype(np.uint64), ln.astype(np.uint32)


def trim_of(packed, byte_off, lens, pile, pileup_cfg, mode=0, min_len=1):
    """trim() on a pileup computed before: pile = pileup_util.pileup(lens, rows, cols, vals, **pileup_cfg)."""
    lens = np.asarray(lens, dtype=np.int64)
    p, _, depth, off = pile
    src, beg, end = pieces_of(lens, p, depth, off, mode, min_len, pileup_cfg.get("min_depth", 1), pileup_cfg.get("min_run", 1))
    out, boff, ln = cut(packed, byte_off, src, beg, end)
    per_read = np.bincount(src, minlength=len(lens))
    whole = np.zeros(len(lens), dtype=bool)
    whole[src[(beg == 0) & (end == lens[src])]] = True
    st = dict(nreads_in=len(lens), pieces=len(src), reads_dropped=int((per_read == 0).sum()), reads_split=int((per_read >= 2).sum()),
              reads_unchanged=int(((per_read == 1) & whole).sum()), bases_in=int(lens.sum()), bases_out=int(ln.sum()), packed_bytes=len(out) - 16,
              longest=int(ln.max()) if len(ln) else 0)
    return dict(n=len(src), src_read=src, src_beg=beg, src_end=end, byte_off=boff, len=ln, packed=out, flags=p["flags"]), st


def trim(packed, byte_off, lens, rows, cols, vals, pileup_cfg, mode=0, min_len=1):
    """Everything elba_trim_reads computes after elba_read_pileup(**pileup_cfg): dict of the map, byte_off, len, packed, and the stats."""
    lens = np.asarray(lens, dtype=np.int64)
    return trim_of(packed, byte_off, lens, pu.pileup(lens, rows, cols, vals, **pileup_cfg), pileup_cfg, mode, min_len)


def overlaps_for(M, intervals):
    """A pair list (strictly ascending, row < col, score 1) that credits exactly the given (read, beg, end) intervals: the k-th interval of
    read r rides on the pair {r, (r + 1 + k) mod M}, on the side r has in it; the other side stays (0, 0) unless its read uses it."""
    from elba_amd.capi import OVERLAP_DTYPE
    slot, k = {}, {}
    for r, b, e in intervals:
        j = k.get(r, 0); k[r] = j + 1
        assert j < M - 1, "more intervals on one read than it has partners"
        t = (r + 1 + j) % M
        key = (min(r, t), max(r, t))
        side = 0 if r < t else 1
        assert (key, side) not in slot
        slot[(key, side)] = (b, e)
    keys = sorted({ks[0] for ks in slot})
    vals = np.zeros(len(keys), OVERLAP_DTYPE)
    vals["score"] = 1
    for a, key in enumerate(keys):
        vals["begQ"][a], vals["endQ"][a] = slot.get((key, 0), (0, 0))
        vals["begT"][a], vals["endT"][a] = slot.get((key, 1), (0, 0))
    return np.array([x[0] for x in keys], np.int64), np.array([x[1] for x in keys], np.int64), vals


def brute_force(seqs, rows, cols, vals, pileup_cfg, mode, min_len):
    """The same on ASCII strings with plain loops: per-base depth lists, runs by a scan, the trimmed interval by the reference's literal loop
    (pileup_util.trimmed_interval_literal), pieces as substrings.  Returns (list of (read, beg, end), list of piece strings)."""
    mg, md, mr = pileup_cfg.get("margin", 0), pileup_cfg.get("min_depth", 1), pileup_cfg.get("min_run", 1)
    depth = [[0] * len(s) for s in seqs]
    for r, c, o in zip(rows, cols, vals):
        if not (o["passed"] != 0 if pileup_cfg.get("mode", 0) == 0 else o["score"] > 0):
            continue
        for who, b, e in ((int(r), int(o["begQ"]), int(o["endQ"])), (int(c), int(o["begT"]), int(o["endT"]))):
            for i in range(b + mg, e - mg):
                depth[who][i] += 1
    out, strs = [], []
    for v, s in enumerate(seqs):
        iv = []
        if mode == 0:
            a, b = pu.trimmed_interval_literal(depth[v], md, pileup_cfg.get("trim_len", 2500))
            if a >= 0:
                iv.append((a, b))
        else:
            start = -1
            for i in range(len(s) + 1):
                if i < len(s) and depth[v][i] >= md:
                    start = i if start < 0 else start
                elif start >= 0:
                    if i - start >= mr:
                        iv.append((start, i))
                    start = -1
        for a, b in iv:
            if b - a >= min_len:
                out.append((v, a, b)); strs.append(s[a:b])
    return out, strs


def chimera_reads(synth_reads, seed=51, glen=150_000, nchim=12):
    """test_gpu_pileup._chimera_reads restated: error-free reads of a random genome plus nchim planted chimeras, the first half of one read
    joined to the second half of a read from at least glen / 4 away.  synth_reads = elba_amd.synth_reads.  Returns (seqs, n0, genome)."""
    packed, off, lens, info = synth_reads(seed, glen, 12, 3000, 500, error_rate=0.0, min_len=1500)
    seqs = cu.seqs_of(packed, off, lens)
    pos = info["genome_pos"]
    n0 = len(seqs)
    rng = np.random.default_rng(seed)
    chim, used = [], set()
    while len(chim) < nchim:
        i, j = (int(x) for x in rng.integers(0, n0, 2))
        if i in used or j in used or abs(int(pos[i]) - int(pos[j])) < glen // 4:
            continue
        used |= {i, j}
        chim.append(seqs[i][:len(seqs[i]) // 2] + seqs[j][len(seqs[j]) // 2:])
    glen_used = int(max(int(pos[v]) + len(seqs[v]) for v in range(n0)))
    g = ["N"] * glen_used
    for v, s in enumerate(seqs):
        fwd = cu.revcomp(s) if info["strand"][v] else s
        g[int(pos[v]):int(pos[v]) + len(fwd)] = fwd
    return seqs + chim, n0, "".join(g)
