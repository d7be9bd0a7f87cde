"""The x-drop stage restated in plain Python/numpy, and the planted-seed case generator.

`xdrop_aligner`, `classify_alignment` and `extend_overlap` follow the reference's src/XDropAligner.cpp and src/Overlap.cpp statement by
statement on ASCII reads; they share no code with oracle/elba_oracle.c or elba_amd/csrc/align.hip.  Scores are Python integers; where
the reference computes in `int` the value is checked to stay inside 32 bits (`_i32`), so a case that would depend on signed overflow
stops here instead of being compared.  One antidiagonal is one numpy expression.

`planted(cases, k)` turns a list of (query, target, seedQ, seedT) into reads and triples of A such that B(2c, 2c+1) carries exactly
that seed as seeds[0]: the aligner under test is then driven with chosen seeds, not with the ones a k-mer stage happens to find.
"""
import numpy as np

INT_MIN = -(1 << 31)
INT_MAX = (1 << 31) - 1
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def _i32(v):
    assert INT_MIN <= v <= INT_MAX, ("the reference's int arithmetic would overflow here", v)
    return v


def _cdiv(a, b):
    """C's integer division (truncation towards zero)."""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def revcomp(s):
    return s.translate(_COMP)[::-1]


class ExtInfo:
    """What one direction did: DP cells, antidiagonals, the widest stored antidiagonal (top_max - off3 + 1), the largest number of cells
    of one antidiagonal that beat `best` (and their number on the last antidiagonal where any did), whether mis / gap were replaced by min_err, and whether the extension was degenerate."""
    __slots__ = ("cells", "ads", "widest", "max_beats", "last_beats", "clamped", "ran", "col", "row", "score")

    def __init__(self):
        self.cells = 0; self.ads = 0; self.widest = 0; self.max_beats = 0; self.last_beats = 0; self.clamped = False; self.ran = False
        self.col = 0; self.row = 0; self.score = 0


def _extend_seed_one_direction(Q, T, extleft, xs, mat, mis, gap, dropoff, info, clamp=True):
    """src/XDropAligner.cpp:46-206.  Q: query codes (uint8 array), T: the target ORIENTED as the seed is (reverse-complemented when rc), so
    that T[posT] is `rc ? seqT.revcomp_at(posT) : seqT.regular_at(posT)`.  xs = [begQ, endQ, begT, endT], updated in place.
    clamp=False leaves out the reference's min_err_score clamp of mis and gap, in unbounded integers (no 32-bit checks: the clamp is what
    keeps the reference inside them); it exists for the test that shows the clamp decides results."""
    lenQ, lenT = len(Q), len(T)
    lenQ_ext = xs[0] if extleft else lenQ - xs[1]
    lenT_ext = xs[2] if extleft else lenT - xs[3]
    cols, rows = lenQ_ext + 1, lenT_ext + 1
    if rows == 1 or cols == 1:
        return 0
    info.ran = True
    ln = 2 * max(cols, rows)
    min_err_score = _cdiv(INT_MIN, ln)
    info.clamped = gap < min_err_score or mis < min_err_score
    if clamp:
        gap = max(gap, min_err_score)
        mis = max(mis, min_err_score)
    i32 = _i32 if clamp else (lambda v: v)
    undef = i32(i32(INT_MIN - gap) - mis)
    min_col, max_col = 1, 2
    offset1 = offset2 = offset3 = 0
    ad1 = np.zeros(0, dtype=np.int64)
    ad2 = np.array([0], dtype=np.int64)
    best_ext_col = best_ext_row = best_ext_score = 0
    g1 = undef if -gap > dropoff else gap
    ad3 = np.array([g1, g1], dtype=np.int64)
    ad_no, best = 1, 0
    offsetQ, offsetT = xs[1], xs[3]
    while min_col < max_col:
        ad_no += 1
        ad1, ad2 = ad2, ad3
        offset1, offset2, offset3 = offset2, offset3, min_col - 1
        ad3 = np.empty(max_col + 1 - offset3, dtype=np.int64)
        info.ads += 1
        info.widest = max(info.widest, len(ad3))
        ad3[0] = ad3[max_col - offset3] = undef
        if i32(ad_no * gap) > i32(best - dropoff):
            if offset3 == 0:
                ad3[0] = ad_no * gap
            if ad_no - max_col == 0:
                ad3[max_col - offset3] = ad_no * gap
        ad_best = ad_no * gap
        n = max_col - min_col
        if n > 0:
            info.cells += n
            c = np.arange(min_col, max_col)
            if extleft:
                qb = Q[cols - 1 - max_col + 1:cols - 1 - min_col + 1][::-1]                     # posQ = cols - 1 - col
                p0 = rows - 1 + min_col - ad_no                                                 # posT = rows - 1 + col - ad_no
                tb = T[p0:p0 + n]
            else:
                qb = Q[min_col - 1 + offsetQ:max_col - 1 + offsetQ]                             # posQ = col - 1 + offsetQ
                p1 = ad_no - min_col - 1 + offsetT                                              # posT = ad_no - col - 1 + offsetT
                tb = T[p1 - n + 1:p1 + 1][::-1]
            assert (p0 if extleft else p1 - n + 1) >= 0 and cols - max_col >= 0
            assert len(qb) == n and len(tb) == n, "a base outside its read"
            i2, i1 = c - offset2, c - offset1
            assert i2[0] - 1 >= 0 and i2[-1] < len(ad2) and i1[0] - 1 >= 0 and i1[-1] - 1 < len(ad1), "a cell outside its antidiagonal"
            temp = np.maximum(ad2[i2 - 1], ad2[i2]) + gap
            temp2 = ad1[i1 - 1] + np.where(qb == tb, mat, mis)
            assert not clamp or (min(int(temp.min()), int(temp2.min())) >= INT_MIN and max(int(temp.max()), int(temp2.max())) <= INT_MAX)
            temp = np.maximum(temp, temp2)
            keep = temp >= best - dropoff
            ad3[1:1 + n] = np.where(keep, temp, undef)
            if keep.any():
                ad_best = max(ad_best, int(temp[keep].max()))
            beat = np.nonzero(temp > best)[0]
            if len(beat):
                info.max_beats = max(info.max_beats, len(beat))
                info.last_beats = len(beat)
                best_ext_col = int(c[beat[-1]])                                                 # ascending columns: the last one stays
                best_ext_row = ad_no - best_ext_col
                best_ext_score = int(ad3[best_ext_col - offset3])
                assert best_ext_score == int(temp[beat[-1]])
        best = max(best, ad_best)
        while (min_col - offset3 < len(ad3) and ad3[min_col - offset3] == undef and
               0 <= min_col - offset2 - 1 < len(ad2) and ad2[min_col - offset2 - 1] == undef):
            min_col += 1
        while max_col - offset3 > 0 and ad3[max_col - offset3 - 1] == undef and ad2[max_col - offset2 - 1] == undef:
            max_col -= 1
        max_col += 1
        min_col = max(min_col, ad_no + 2 - rows)
        max_col = min(max_col, cols)
    # (the ext_col / ext_row / ext_score tail of the reference, :158-189, changes nothing that leaves the function)
    if best_ext_score != undef:
        if extleft:
            xs[2] -= best_ext_row; xs[0] -= best_ext_col
        else:
            xs[3] += best_ext_row; xs[1] += best_ext_col
    info.col, info.row, info.score = best_ext_col, best_ext_row, best_ext_score
    return best_ext_score


def _codes(s):
    return np.frombuffer(s, dtype=np.uint8)


def xdrop_aligner(q, t, begQ, begT, k, mat, mis, gap, dropoff, clamp=True):
    """src/XDropAligner.cpp:232-282 on ASCII reads.  Returns (ret, result, infos): result = dict of XSeed's fields (its defaults, include/
    XDropAligner.hpp, when the seed is rejected: all zero, score -1), infos = (left ExtInfo, right ExtInfo)."""
    res = dict(begQ=0, endQ=0, begT=0, endT=0, score=-1, rc=0)
    infos = (ExtInfo(), ExtInfo())
    lenQ, lenT = len(q), len(t)
    if begQ < 0 or begQ + k > lenQ:
        return -1, res, infos
    if begT < 0 or begT + k > lenT:
        return -1, res, infos
    if begQ == 0 and begT == 0:
        return -1, res, infos
    rc = q[begQ + (k >> 1)] != t[begT + (k >> 1)]
    tr = revcomp(t) if rc else t                       # tr[i] = rc ? seqT.revcomp_at(i) : seqT.regular_at(i)
    for i in range(k):
        if q[begQ + i] != (tr[lenT - begT - k + i] if rc else t[begT + i]):
            return -1, res, infos
    xbegT = lenT - begT - k if rc else begT
    seed = [begQ, begQ + k, xbegT, xbegT + k]
    Q, T = _codes(q), _codes(tr)
    left = list(seed)
    lscore = _extend_seed_one_direction(Q, T, True, left, mat, mis, gap, dropoff, infos[0], clamp)
    right = list(seed)
    rscore = _extend_seed_one_direction(Q, T, False, right, mat, mis, gap, dropoff, infos[1], clamp)
    score = lscore + rscore + mat * k
    assert not clamp or (_i32(lscore + rscore) is not None and _i32(score) is not None)
    begQ_ext, begT_ext, endQ_ext, endT_ext = left[0], left[2], right[1], right[3]
    res = dict(begQ=begQ_ext, endQ=endQ_ext, begT=(lenT - endT_ext) if rc else begT_ext, endT=(lenT - begT_ext) if rc else endT_ext,
               score=score, rc=int(rc))
    return score, res, infos


def classify_alignment(ai, lenQ, lenT):
    """src/XDropAligner.cpp:7-44 -> OverlapClass (0 BAD_ALIGNMENT, 1 FIRST_CONTAINED, 2 SECOND_CONTAINED, 3 FIRST_TO_SECOND, 4 SECOND_TO_FIRST)."""
    if ai["score"] <= 0:
        return 0
    begTr = lenT - ai["endT"] if ai["rc"] else ai["begT"]
    endTr = lenT - ai["begT"] if ai["rc"] else ai["endT"]
    maplen = _cdiv((ai["endT"] - ai["begT"]) + (ai["endQ"] - ai["begQ"]), 2)
    overhang = min(ai["begQ"], begTr) + min(lenQ - ai["endQ"], lenT - endTr)
    overlap = maplen + overhang
    my_thr = np.float32((1.0 - 0.1) * (0.99 * overlap))                 # float my_thr = (1.0 - DELTACHERNOFF) * (0.99 * overlap)
    if ai["begQ"] <= begTr and lenQ - ai["endQ"] <= lenT - endTr:
        return 1
    if ai["begQ"] >= begTr and lenQ - ai["endQ"] >= lenT - endTr:
        return 2
    if np.float32(ai["score"]) < my_thr or overlap < 500:               # int < float: the int is converted to float
        return 0
    if ai["begQ"] > begTr:
        return 3
    return 4


OVERLAP_FIELDS = ("begQ", "begT", "endQ", "endT", "score", "suffix", "suffixT", "direction", "directionT", "rc", "passed", "containedQ", "containedT", "kind")


def extend_overlap(q, t, seedQ, seedT, k, mat, mis, gap, dropoff, clamp=True):
    """Overlap::Overlap + Overlap::extend_overlap (src/Overlap.cpp:4-10, :20-73) -> (dict of OVERLAP_FIELDS, ret, infos)."""
    ret, r, infos = xdrop_aligner(q, t, seedQ, seedT, k, mat, mis, gap, dropoff, clamp)
    lenQ, lenT = len(q), len(t)
    kind = classify_alignment(r, lenQ, lenT)
    o = dict(score=r["score"], suffix=0, suffixT=0, direction=-1, directionT=-1, rc=r["rc"], passed=0, containedQ=0, containedT=0, kind=kind,
             begQ=r["begQ"], begT=r["begT"], endQ=r["endQ"], endT=r["endT"])
    rc = r["rc"]
    begQr, endQr = r["begQ"], r["endQ"]
    begTr = lenT - r["endT"] if rc else r["begT"]
    endTr = lenT - r["begT"] if rc else r["endT"]
    if kind != 0:
        o["passed"] = 1
        if kind == 1:
            o["containedQ"] = 1
        elif kind == 2:
            o["containedT"] = 1
        elif kind == 3:
            o["direction"] = 0 if rc else 1
            o["directionT"] = 0 if rc else 2
            o["suffix"] = (lenT - endTr) - (lenQ - endQr)
            o["suffixT"] = begQr - begTr
        else:
            o["direction"] = 3 if rc else 2
            o["directionT"] = 3 if rc else 1
            o["suffix"] = begTr - begQr
            o["suffixT"] = (lenQ - endQr) - (lenT - endTr)
    return o, ret, infos


# ---- planted seeds ---------------------------------------------------------------------------------------------------------------
class Case:
    """One pair: query, target (ASCII bytes), the planted seed (signed: a negative position is stored as its uint32 image), numshared of
    B's entry, and free-form notes the family's own checks use."""

    def __init__(self, name, q, t, q0, t0, numshared=2, **notes):
        self.name, self.q, self.t, self.q0, self.t0, self.numshared, self.notes = name, bytes(q), bytes(t), int(q0), int(t0), int(numshared), notes


def pack_ascii(seqs, tail=16):
    """ASCII reads (ACGT only) -> (packed u8, byte offsets u64, lengths u32) in the reference's DnaBuffer layout: four bases per byte, the
    first in the two highest bits, A C G T = 0 1 2 3, every read starting on a byte; `tail` zero bytes follow the last read."""
    lens = np.array([len(s) for s in seqs], dtype=np.uint32)
    nb = (lens.astype(np.int64) + 3) // 4
    off = np.zeros(len(seqs), dtype=np.uint64)
    if len(seqs):
        off[1:] = np.cumsum(nb)[:-1]
    buf = np.zeros(int(nb.sum()) + tail, dtype=np.uint8)
    lut = np.full(256, 255, dtype=np.uint8)
    for i, ch in enumerate(b"ACGT"):
        lut[ch] = i
    for i, s in enumerate(seqs):
        c = lut[np.frombuffer(s, dtype=np.uint8)]
        assert (c < 4).all()
        pad = np.zeros(int(nb[i]) * 4, dtype=np.uint8)
        pad[:len(c)] = c
        p = pad.reshape(-1, 4)
        buf[int(off[i]):int(off[i]) + int(nb[i])] = (p[:, 0] << 6) | (p[:, 1] << 4) | (p[:, 2] << 2) | p[:, 3]
    return buf, off, lens


def planted(cases, k, ids=None):
    """-> (packed, off, lens, M, N, rows, cols, vals): case c becomes reads 2c (query) and 2c + 1 (target) and `numshared` columns of A that
    hold exactly these two reads; the column with the smallest id carries the seed, so B(2c, 2c+1).seeds[0] = (q0, t0) and B(2c+1, 2c) its
    mirror image.  The other columns' positions are fillers (1, 2): they are seeds[1] at most and never aligned.  No position is checked
    against a read's length by either side (elba_set_kmer_matrix, orc_set_triples): that is the point.
    ids: another numbering, ids[c] = (query's read id, target's read id) with query < target (the aligner takes the smaller id as query)."""
    n = len(cases)
    for cs in cases:          # what is out of range overshoots its read by at most k bases (both sides reject it before reading a base)
        assert max(cs.q0 + k - len(cs.q), cs.t0 + k - len(cs.t), -cs.q0, -cs.t0) <= k, cs.name
    if ids is None:
        ids = [(2 * c, 2 * c + 1) for c in range(n)]
    assert sorted(i for p in ids for i in p) == list(range(2 * n)) and all(a < b for a, b in ids)
    seqs, rows, cols, vals = [None] * (2 * n), [], [], []
    ncol = 0
    for (a, b), cs in zip(ids, cases):
        seqs[a], seqs[b] = cs.q, cs.t
        assert cs.numshared >= 2, "B drops entries with one shared k-mer"
        for s in range(cs.numshared):
            rows += [a, b]; cols += [ncol, ncol]
            vals += [(cs.q0 if s == 0 else 1) & 0xFFFFFFFF, (cs.t0 if s == 0 else 2) & 0xFFFFFFFF]
            ncol += 1
    packed, off, lens = pack_ascii(seqs)
    return (packed, off, lens, len(seqs), ncol, np.array(rows, dtype=np.int64), np.array(cols, dtype=np.int64), np.array(vals, dtype=np.uint32))


def scattered_ids(n, seed):
    """A random numbering of n pairs' reads in which query < target: pairs straddle any partition of the reads, with both parities of i + j."""
    p = np.random.default_rng(seed).permutation(2 * n)
    return [(int(min(p[2 * c], p[2 * c + 1])), int(max(p[2 * c], p[2 * c + 1]))) for c in range(n)]


def extensions_run(cs, k):
    """How many of the pair's two extensions run at all (0 for a rejected seed; a direction with no bases left in either read does not)."""
    q, t, q0, t0 = cs.q, cs.t, cs.q0, cs.t0
    if q0 < 0 or q0 + k > len(q) or t0 < 0 or t0 + k > len(t) or (q0 == 0 and t0 == 0):
        return 0
    rc = q[q0 + (k >> 1)] != t[t0 + (k >> 1)]
    if q[q0:q0 + k] != (revcomp(t[t0:t0 + k]) if rc else t[t0:t0 + k]):
        return 0
    tl, tr = (len(t) - t0 - k, t0) if rc else (t0, len(t) - t0 - k)
    return int(q0 > 0 and tl > 0) + int(len(q) - q0 - k > 0 and tr > 0)


def orientations(cs):
    """The case as it is, with the target reverse-complemented, with query and target exchanged, and both."""
    k = cs.notes["k"]
    if cs.notes.get("fixed"):
        return [cs, Case(cs.name + "/swap", cs.t, cs.q, cs.t0, cs.q0, cs.numshared, **dict(cs.notes, swapped=True))]
    tr, t0r = revcomp(cs.t), len(cs.t) - cs.t0 - k
    qr, q0r = revcomp(cs.q), len(cs.q) - cs.q0 - k
    return [cs,
            Case(cs.name + "/rc", cs.q, tr, cs.q0, t0r, cs.numshared, **cs.notes),
            Case(cs.name + "/swap", cs.t, cs.q, cs.t0, cs.q0, cs.numshared, **dict(cs.notes, swapped=True)),
            Case(cs.name + "/swap+rc", cs.t, qr, cs.t0, q0r, cs.numshared, **dict(cs.notes, swapped=True))]


# ---- sequences ---------------------------------------------------------------------------------------------------------------------
def rand_seq(rng, n):
    return bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(n))].tolist())


def mutate(rng, s, err):
    """substitutions, insertions and deletions, a third each, at rate `err` per base"""
    if err <= 0:
        return s
    out = bytearray()
    r = rng.random(len(s)); kind = rng.integers(0, 3, len(s)); nb = rng.integers(0, 4, len(s))
    for i, ch in enumerate(s):
        if r[i] >= err:
            out.append(ch)
        elif kind[i] == 0:
            out.append(b"ACGT"[(b"ACGT".index(ch) + 1 + nb[i] % 3) % 4])
        elif kind[i] == 1:
            out.append(ch); out.append(b"ACGT"[nb[i]])
    return bytes(out)


def related(rng, name, k, ql, qr, tl, tr, err, **notes):
    """Two reads of one locus around a shared k-mer: the query has ql bases left of the seed and qr right of it, the target tl and tr; the
    target's flanks are the query's with errors at rate `err` (padded with unrelated bases where the target is longer)."""
    m = max(ql, qr, tl, tr)
    L, R, kmer = rand_seq(rng, 2 * m + 64), rand_seq(rng, 2 * m + 64), rand_seq(rng, k)
    Lt, Rt = rand_seq(rng, m + 64) + mutate(rng, L, err), mutate(rng, R, err) + rand_seq(rng, m + 64)
    q = L[len(L) - ql:] + kmer + R[:qr]
    t = Lt[len(Lt) - tl:] + kmer + Rt[:tr]
    return Case(name, q, t, ql, tl, k=k, **notes)


def unrelated(rng, name, k, ql, qr, tl, tr, **notes):
    """Two random reads that share nothing but the planted k-mer."""
    kmer = rand_seq(rng, k)
    return Case(name, rand_seq(rng, ql) + kmer + rand_seq(rng, qr), rand_seq(rng, tl) + kmer + rand_seq(rng, tr), ql, tl, k=k, **notes)


# ---- the families ---------------------------------------------------------------------------------------------------------------
P_DEFAULT = (1, -1, -1, 15)


def fam_rejected(k=17):
    """Every seed here is refused by xdrop_aligner's prologue; out-of-range positions overshoot the read by at most k bases."""
    rng = np.random.default_rng(7001)
    base = related(rng, "ok", k, 120, 150, 90, 200, 0.03)
    q, t, q0, t0 = base.q, base.t, base.q0, base.t0
    lq, lt = len(q), len(t)
    same = rand_seq(rng, 300)
    cs = [Case("q-past-end-by-1", q, t, lq - k + 1, t0), Case("q-past-end-by-k", q, t, lq, t0),
          Case("t-past-end-by-1", q, t, q0, lt - k + 1), Case("t-past-end-by-k", q, t, q0, lt),
          Case("both-past-end", q, t, lq - k + 3, lt - k + 2),
          Case("q-negative-1", q, t, -1, t0), Case("q-negative-k", q, t, -k, t0), Case("t-negative-1", q, t, q0, -1), Case("t-negative-k", q, t, q0, -k),
          # (the rule is about the stored positions, so these come as written and exchanged, not through orientations())
          Case("zero-zero-identical-reads", same, same, 0, 0, fixed=True), Case("zero-zero-shared-prefix", same[:200], same[:k] + rand_seq(rng, 100), 0, 0, fixed=True),
          Case("zero-zero-reverse-complement-prefix", same[:220], revcomp(same[:k]) + rand_seq(rng, 130), 0, 0, fixed=True),
          Case("not-shared-shift-q", q, t, q0 + 1, t0), Case("not-shared-shift-t", q, t, q0, t0 - 1),
          Case("last-base-differs", q[:q0 + k - 1] + bytes([b"ACGT"[(b"ACGT".index(q[q0 + k - 1]) + 1) % 4]]) + q[q0 + k:], t, q0, t0),
          Case("first-base-differs", bytes(q[:q0]) + bytes([b"ACGT"[(b"ACGT".index(q[q0]) + 2) % 4]]) + q[q0 + 1:], t, q0, t0),
          # the middle base decides the orientation: with only that base changed the seed is tried as a reverse complement and fails
          Case("middle-base-differs", q[:q0 + k // 2] + bytes([b"ACGT"[(b"ACGT".index(q[q0 + k // 2]) + 1) % 4]]) + q[q0 + k // 2 + 1:], t, q0, t0),
          Case("query-shorter-than-k", q[:k - 1], t, 0, t0), Case("target-shorter-than-k", q, t[:k - 2], q0, 1),
          Case("query-one-base", b"A", t, 0, t0), Case("seed-at-last-valid-plus-0-other-past", q, t, lq - k, lt - k + 1)]
    for c in cs:
        c.notes["k"] = k
    out = []
    for c in cs:
        out += orientations(c)
    return out


def fam_edges(k=17):
    """Seeds at the corners and edges of the two reads (one or both directions degenerate), reads of length k and k + 1, 1-base extensions."""
    rng = np.random.default_rng(7002)
    cs = []
    for name, ql, qr, tl, tr in [("q-starts-at-seed", 0, 200, 60, 220), ("t-starts-at-seed", 70, 200, 0, 180), ("q-ends-at-seed", 150, 0, 170, 90),
                                 ("t-ends-at-seed", 150, 80, 170, 0), ("both-end-at-seed", 150, 0, 120, 0), ("q-starts-t-ends", 0, 200, 180, 0),
                                 ("q-ends-t-starts", 200, 0, 0, 180), ("query-is-the-seed", 0, 0, 90, 100), ("target-is-the-seed", 100, 80, 0, 0),
                                 ("query-of-k-at-target-end", 0, 0, 150, 0), ("query-k+1-left", 1, 0, 90, 100), ("query-k+1-right", 0, 1, 90, 100),
                                 ("both-k+1-left", 1, 0, 1, 0), ("both-k+1-right", 0, 1, 1, 1), ("one-base-each-way", 1, 1, 1, 1),
                                 ("one-column-many-rows", 1, 1, 200, 200), ("two-columns-many-rows", 2, 2, 300, 250), ("second-base", 1, 250, 1, 260),
                                 ("q-second-t-first", 1, 250, 0, 260), ("last-but-one", 250, 1, 240, 1)]:
        cs.append(related(rng, name, k, ql, qr, tl, tr, 0.04))
    cs.append(Case("with-a-read-shorter-than-k", cs[0].q[:k - 3], cs[0].t, 0, 5, k=k))
    out = []
    for c in cs:
        out += orientations(c)
    return out


def fam_ratio(k=17):
    """Length ratio 1 : 100 with the seed near either end: the row / column clamps move min_col and max_col."""
    rng = np.random.default_rng(7003)
    cs = []
    for name, ql, qr, tl, tr in [("short-in-long-front", 6, 37, 30, 5900), ("short-in-long-back", 37, 6, 5900, 30), ("short-in-long-middle", 20, 23, 3000, 2950),
                                 ("short-front-long-back", 6, 37, 5900, 30), ("short-back-long-front", 37, 6, 30, 5900), ("short-at-long-start", 3, 40, 2, 5950)]:
        cs.append(related(rng, name, k, ql, qr, tl, tr, 0.05))
    cs.append(unrelated(rng, "unrelated-short-in-long", k, 25, 18, 2500, 3400))
    out = []
    for c in cs:
        out += orientations(c)
    return out


RATIO_PARAMS = [P_DEFAULT, (1, -1, -1, 100), (1, -1, -1, 20000)]


def _repeat(unit, n, phase=0):
    s = unit * (n // len(unit) + 3)
    return s[phase:phase + n]


def _first_match(q, t, q0, k, start=0):
    t0 = t.find(q[q0:q0 + k], start)
    assert t0 >= 0
    return t0


def _interrupt(s, at, n, foreign):
    return s[:at] + foreign * n + s[at + n:]


def fam_ties(k=17):
    """Homopolymers, 2- and 3-base tandem repeats at different phases, a repeat unit embedded in random flanks: antidiagonals on which many
    cells are equal.  Said plainly: the homopolymer and the 2- and 3-base tandem cases do NOT have two cells beating `best` on one
    antidiagonal (ties=False; they are kept for their many equal cells and their trimming); only the cases marked ties=True do, and
    tests/test_xdrop_planted_cpu.py asserts it for exactly those.  On a pure repeat only the seed's diagonal ever beats `best`; where the target has a short foreign block (3 bases, or 9
    in a 3-base repeat: mismatches on the seed's diagonal against gaps around it, at equal cost under +1/-1/-1, see below) two diagonals recover
    together and the 'last column that beats best' is decided among them: the cases where that happens carry ties=True."""
    # the block: m mismatches on the seed's diagonal cost m over 2m antidiagonals; g gaps around it cost g over g antidiagonals and leave
    # (2m - g) / 2 matches to catch up: equal scores on the same antidiagonal when g = 4m / 3, and g must be a multiple of the period:
    # m = 3, g = 4 for period 4.  With periods 1, 2 and 3 a shorter shift (some gaps, some mismatches) is cheaper than both and leads alone.
    rng = np.random.default_rng(7004)
    cs = [Case("homopolymer", b"A" * 300, b"A" * 420, 50, 120, ties=False), Case("homopolymer-seed-late", b"C" * 260, b"C" * 200, 230, 100, ties=False),
          Case("homopolymer-vs-interrupted-once", b"G" * 300, b"G" * 150 + b"T" + b"G" * 200, 40, 60, ties=False),
          Case("homopolymer-interrupted", b"A" * 300, _interrupt(_interrupt(b"A" * 420, 80, 3, b"C"), 190, 3, b"G"), 50, 120, ties=False)]
    for unit, nq, nt, pq, pt, q0, blk, foreign in [(b"AT", 300, 380, 0, 1, 60, 3, b"G"), (b"AC", 250, 250, 1, 0, 11, 3, b"T"), (b"ACG", 330, 300, 0, 1, 100, 9, b"T"),
                                                   (b"ACG", 300, 400, 2, 0, 31, 9, b"T"), (b"AAC", 301, 299, 1, 2, 150, 9, b"G"), (b"AG", 120, 700, 0, 0, 50, 3, b"C")]:
        q, t = _repeat(unit, nq, pq), _repeat(unit, nt, pt)
        t0 = _first_match(q, t, q0, k, start=nt // 3)
        cs.append(Case("tandem-%s-%d-%d" % (unit.decode(), pq, pt), q, t, q0, t0, ties=False))
        ti = t
        if t0 + k + 30 + blk < nt and q0 + k + 45 < nq:
            ti = _interrupt(ti, t0 + k + 30, blk, foreign)
        if t0 > 45 and q0 > 45:
            ti = _interrupt(ti, t0 - 36, blk, foreign)
        assert ti != t
        cs.append(Case("tandem-%s-%d-%d-interrupted" % (unit.decode(), pq, pt), q, ti, q0, t0, ties=False))          # one diagonal leads alone: see above
    # periods 4 and 8, where no cheaper in-phase shift exists: block lengths found with this module's restatement (cells beating best >= 2)
    for unit, nq, nt, pq, pt, q0, blk, foreign in [(b"AACG", 300, 420, 0, 1, 60, 3, b"T"), (b"AAAC", 300, 380, 2, 1, 100, 7, b"G"), (b"ACGT", 260, 300, 1, 3, 80, 12, b"A"),
                                                   (b"AACCGGTT", 400, 420, 1, 3, 120, 9, b"A")]:
        q, t = _repeat(unit, nq, pq), _repeat(unit, nt, pt)
        t0 = _first_match(q, t, q0, k, start=nt // 3)
        ti = _interrupt(_interrupt(t, t0 + k + 30, blk, foreign), t0 - 50, blk, foreign)
        cs.append(Case("tandem-%s-interrupted" % unit.decode(), q, ti, q0, t0, ties=True))
        # ... and with the target cut so that the two tied diagonals reach their last cells on the same antidiagonal: the extension's END is
        # decided among ties (d: target bases beyond the query's end, found with the restatement: last_beats >= 2)
        for d in dict(AACG=(2,), AAAC=(6,), ACGT=(2, 10)).get(unit.decode(), ()):
            cs.append(Case("tandem-%s-tied-at-end-%d" % (unit.decode(), d), q, ti[:t0 + nq - q0 + d], q0, t0, ties=True, tied_end=True))
    for unit, n, ties in [(b"AT", 140, True), (b"ACG", 150, True), (b"A", 90, False)]:
        core = _repeat(unit, n)
        fl = [rand_seq(rng, 150) for _ in range(3)]
        q = fl[0] + core + fl[1]
        t = mutate(rng, fl[0], 0.03)[-120:] + _repeat(unit, n + 12) + fl[2]
        q0 = 150 + 20
        cs.append(Case("embedded-%s" % unit.decode(), q, t, q0, _first_match(q, t, q0, k, start=125), ties=ties))
    for c in cs:
        c.notes["k"] = k
    out = []
    for c in cs:
        out += orientations(c)
    return out


TIES_PARAMS = [P_DEFAULT, (1, -1, -1, 100), (2, -3, -2, 7), (1, -2, -3, 30)]


INDEL_SCORES = (1, -2, -2)          # unrelated sequence loses under these, so an extension that cannot pay for the gap ends at the indel
                                    # (under +1/-1/-1 it wanders on through unrelated bases: random DNA gains score there)


def indel_bridge_x(n):
    """An x-drop that bridges a gap of n bases under INDEL_SCORES (and lets the extension go on past it)."""
    return 2 * n + n // 5 + 20


INDEL_SIZES = (50, 200, 1000)


def fam_indel(k=17):
    """One insertion of 50, 200 or 1 000 bases in one of the reads, right or left of the seed, in otherwise identical reads: the band shifts by
    that many columns (or rows) while staying narrow, if the x-drop lets the extension cross it."""
    rng = np.random.default_rng(7005)
    cs = []
    for n in INDEL_SIZES:
        near, far = 150, 2 * n + 300              # identical bases between seed and indel, and beyond it (enough to win the gap back)
        a, b, c, kmer, ins = rand_seq(rng, 100), rand_seq(rng, near), rand_seq(rng, far), rand_seq(rng, k), rand_seq(rng, n)
        cs.append(Case("ins-%d-right-in-target" % n, a + kmer + b + c, a + kmer + b + ins + c, 100, 100, k=k, indel=n, side="right", at=100 + k + near, full=100 + k + near + far))
        cs.append(Case("ins-%d-left-in-target" % n, c + b + kmer + a, c + ins + b + kmer + a, far + near, far + n + near, k=k, indel=n, side="left", at=far, full=0))
    out = []
    for c in cs:
        out += orientations(c)
    return out


INDEL_PARAMS = [INDEL_SCORES + (15,)] + [INDEL_SCORES + (indel_bridge_x(n),) for n in INDEL_SIZES] + [P_DEFAULT]

# Band-width ladder.  Found by running this module's restatement (tests/xdrop_util.py: ladder_search) over unrelated random read pairs
# under +1/-1/-1 with the x-drop as the dial: (rng seed of the pair, x-drop) whose widest stored antidiagonal, over the pair's two
# extensions, is exactly the rung.  LADDER is checked against the restatement by tests/test_xdrop_planted_cpu.py.
LADDER_RUNGS = (63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513)
LADDER = {63: (9104, 10), 64: (9102, 11), 65: (9102, 12), 127: (9101, 21), 128: (9101, 22), 129: (9104, 17),
          255: (9102, 69), 256: (9100, 69), 257: (9101, 67), 511: (9100, 293), 512: (9100, 295), 513: (9100, 296),
          500: (9101, 289), 517: (9100, 301)}          # rung -> (pair seed, x-drop)
# two more rungs, found the same way: the pairs at 511 ... 513 have their OTHER extension at 508 ... 510 columns, inside the 512-column tier's
# grey zone (506 ... 512); these two have both extensions clear of every tier's (491 / 500 and 513 / 517 columns)
LADDER_CLEAR = (500, 517)
LADDER_FLANK = 800   # bases on each side of the seed, in both reads


def ladder_pair(seed, k=17):
    rng = np.random.default_rng(int(seed))
    return unrelated(rng, "ladder-pair-%d" % seed, k, LADDER_FLANK, LADDER_FLANK, LADDER_FLANK, LADDER_FLANK)


def widest_of(cs, params):
    o, ret, infos = extend_overlap(cs.q, cs.t, cs.q0, cs.t0, cs.notes["k"], *params)
    return max(infos[0].widest, infos[1].widest)


def ladder_search(rungs=LADDER_RUNGS, seeds=range(9100, 9200), xmax=4000):
    """For every rung the first (pair seed, x) with exactly that widest antidiagonal: bisection on x per pair (the width grows with x, not
    strictly), then a scan of the neighbourhood."""
    found = {}
    for s in seeds:
        cs = ladder_pair(s)
        memo = {}

        def w(x):
            if x not in memo:
                memo[x] = widest_of(cs, (1, -1, -1, x))
            return memo[x]

        for r in rungs:
            if r in found:
                continue
            lo, hi = 1, xmax
            if w(hi) < r:
                continue
            while hi - lo > 1:
                mid = (lo + hi) // 2
                if w(mid) >= r:
                    hi = mid
                else:
                    lo = mid
            for x in range(max(1, hi - 6), hi + 7):
                if w(x) == r:
                    found[r] = (s, x)
                    break
        if len(found) == len(rungs):
            break
    return found


def fam_ladder(k=17):
    """-> [(rung, Case, params)]: one pair per rung, each with its own x-drop, in the four orientations (the reverse complement leaves the
    recurrence as it is and the exchange transposes it: tests/test_xdrop_planted_cpu.py checks that every variant still has the rung's
    width)."""
    out = []
    for r in LADDER_RUNGS + LADDER_CLEAR:
        s, x = LADDER[r]
        cs = ladder_pair(s, k)
        cs.name = "rung-%d" % r
        cs.notes["rung"] = r
        out += [(r, v, (1, -1, -1, x)) for v in orientations(cs)]
    return out


def mixed(rng, k, scale=1):
    """A small mixed set: related reads with errors, clean related reads, unrelated reads, a repeat, corner seeds, a rejected seed."""
    s = scale
    cs = [related(rng, "related-5pc", k, 300 * s, 350 * s, 280 * s, 400 * s, 0.05), related(rng, "related-15pc", k, 400 * s, 300 * s, 380 * s, 330 * s, 0.15),
          related(rng, "related-clean", k, 250 * s, 260 * s, 300 * s, 200 * s, 0.0), unrelated(rng, "unrelated", k, 330 * s, 380 * s, 360 * s, 340 * s),
          related(rng, "contained", k, 60, 90, 400 * s, 420 * s, 0.02), related(rng, "q-starts-at-seed", k, 0, 300, 50, 320, 0.03),
          related(rng, "t-ends-at-seed", k, 200, 100, 220, 0, 0.03)]
    hp = b"A" * (k + 150)
    cs.append(Case("homopolymer", hp, hp + b"A" * 40, 30, 55, k=k))
    cs.append(Case("rejected-not-shared", cs[0].q, cs[0].t, cs[0].q0 + 1, cs[0].t0, k=k))
    return cs


def fam_scores(k=17):
    """One mixed set (reads long enough for bands beyond 512 columns) under the score sets of SCORE_PARAMS."""
    rng = np.random.default_rng(7006)
    out = []
    for c in mixed(rng, k, scale=2):
        out += orientations(c)
    return out


# mat = 0; mis = 0; -gap > dropoff (antidiagonal 1 starts undef); dropoff = 0 with gap = 0; x-drops that never trim (the whole rectangle);
# mis / gap below INT_MIN / (2 * max(cols, rows)) (replaced by min_err, per extension); gap just above and at the smallest clamp of the set
SCORE_PARAMS = [(0, -1, -1, 15), (1, 0, -1, 15), (1, -1, -20, 15), (1, -1, 0, 0), (1, -1, -1, 0), (1, -1, -1, 1 << 30), (1, -1, -1, INT_MAX),
                (1, -2000000000, -1, 15), (1, -1, -2000000000, 15), (1, -3000000, -3000000, 1000), (2, INT_MIN, INT_MIN, 40), (1, -1, -1300000, 2000000),
                (3, -5, -4, 60)]
SCORE_CLAMP_PARAMS = SCORE_PARAMS[7:12]

K_VALUES = (3, 5, 17, 31, 33, 63, 95)


def fam_k(k):
    rng = np.random.default_rng(7100 + k)
    out = []
    for c in mixed(rng, k):
        out += orientations(c)
    return out


K_PARAMS = [P_DEFAULT, (2, -3, -2, 25)]


def fam_hint(k=17):
    """numshared on both sides of aln_wide_hint's default (6): the same narrow-band and wide-band pairs with 2, 6, 7 and 20 shared k-mers."""
    rng = np.random.default_rng(7007)
    base = [related(rng, "related-3pc", k, 500, 600, 450, 700, 0.03), unrelated(rng, "unrelated", k, 500, 600, 450, 700),
            related(rng, "related-12pc", k, 700, 800, 750, 700, 0.12)]
    out = []
    for ns in (2, 6, 7, 20):
        for c in base:
            for v in orientations(c):
                out.append(Case("%s/ns%d" % (v.name, ns), v.q, v.t, v.q0, v.t0, ns, **v.notes))
    return out


HINT_PARAMS = [P_DEFAULT, (1, -1, -1, 90), (1, -1, -1, 600)]


def fam_long(k=17):
    """Reads of 70 000 ... 100 000 bases: a near-identical pair (tens of thousands of antidiagonals in a narrow band) and an unrelated pair
    under a large x-drop (a band far beyond every register tier, in scratch rows sized by the longest read).  Too large for the Python
    restatement: compared oracle against reference vectors, and engine against oracle."""
    rng = np.random.default_rng(7008)
    a = related(rng, "long-near-identical", k, 40000, 50000, 38000, 45000, 0.002)
    b = unrelated(rng, "long-unrelated", k, 30000, 40000, 35000, 36000)
    return orientations(a) + orientations(b)


LONG_PARAMS = [P_DEFAULT, (1, -1, -1, 60)]


def asymmetric(k=17):
    """Pairs whose two seed positions are far apart AND whose reads differ in length: aligned from the mirrored entry B(j, i) without the
    swap of its two positions they cannot give the same result (the row-shard path takes half of the pairs from that entry)."""
    rng = np.random.default_rng(7009)
    cs = []
    for i in range(12):
        ql, tl = int(rng.integers(20, 200)), int(rng.integers(900, 1500))
        cs.append(related(rng, "asym-%d" % i, k, ql, int(rng.integers(2000, 2300)), tl, int(rng.integers(50, 300)), 0.04))
    out = []
    for c in cs:
        out += orientations(c)
    return out


# ---- the registry ------------------------------------------------------------------------------------------------------------------
FAMILY_NAMES = ("rejected", "edges", "ratio", "ties", "indel", "ladder", "scores") + tuple("k%d" % k for k in K_VALUES) + ("hint", "long", "asymmetric")
PYTHON_SKIPS = ("long",)          # too large for the restatement: oracle against reference vectors only
_cache = {}


def family(name):
    """-> (k, [(params, cases), ...]): every group is one alignment call over one planted read set."""
    if name in _cache:
        return _cache[name]
    if name == "ladder":
        byx = {}
        for r, cs, p in fam_ladder():
            byx.setdefault(p, []).append(cs)
        out = (17, [(p, byx[p]) for p in sorted(byx)])
    elif name[0] == "k" and name[1:].isdigit():
        k = int(name[1:])
        cs = fam_k(k)
        out = (k, [(p, cs) for p in K_PARAMS])
    else:
        gen, params = dict(rejected=(fam_rejected, [P_DEFAULT]), edges=(fam_edges, [P_DEFAULT, (1, -1, -1, 100)]), ratio=(fam_ratio, RATIO_PARAMS),
                           ties=(fam_ties, TIES_PARAMS), indel=(fam_indel, INDEL_PARAMS), scores=(fam_scores, SCORE_PARAMS), hint=(fam_hint, HINT_PARAMS),
                           long=(fam_long, LONG_PARAMS), asymmetric=(asymmetric, [P_DEFAULT, (1, -1, -1, 100)]))[name]
        cs = gen()
        out = (17, [(p, cs) for p in params])
    _cache[name] = out
    return out


_memo = {}


def restated(cs, k, params):
    """extend_overlap of a case, remembered (families repeat pairs under other names)."""
    key = (cs.q, cs.t, cs.q0, cs.t0, k, params)
    if key not in _memo:
        _memo[key] = extend_overlap(cs.q, cs.t, cs.q0, cs.t0, k, *params)
    return _memo[key]


def case_crc(cs):
    import zlib
    return zlib.crc32(cs.q + b"|" + cs.t) & 0xFFFFFFFF


def panel_records(rows, cols, vals, row_lo, row_hi):
    """The planted triples as the column panel of rows [row_lo, row_hi) (elba_dist_set_panel): every column that has an entry in one of these
    rows, whole, as records (column id, read << 32 | pos), a column's entries contiguous and ordered by (read, pos)."""
    inside = (rows >= row_lo) & (rows < row_hi)
    keep = np.isin(cols, np.unique(cols[inside]))
    r, c, v = rows[keep], cols[keep], vals[keep].astype(np.int64)
    order = np.lexsort((v, r, c))
    rec = np.stack([c[order], (r[order] << 32) | v[order]], axis=1).astype(np.int64)
    return np.ascontiguousarray(rec)
